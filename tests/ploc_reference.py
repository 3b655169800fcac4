"""Reference for the device builder's locally-ordered clustering (mi3pt_device_build_bvh_ex, method 1), written from the law in
include/mi3pt.h and nothing else: numpy and plain Python only, nothing here looks at the device.

Leaves and order are the linear builder's first half (tests/lbvh_reference.py: triangle_boxes, centroids, quantise, interleave, a
stable sort).  Then the clusters: the distance of two is the half area of the union of their boxes in fp32, (ex ey + ey ez) + ez ex, a
NaN counting as +inf; the key of a pair of positions a < b is (d, b - a, a & 1, a); a search iteration gives every position its
least-keyed partner within `radius` positions, a forced iteration (after `max_search_iterations` search iterations) the partner i ^ 1;
mutual pairs merge into the lower position, the survivors keep their order; the records are numbered in pre-order.

build() is vectorised over the candidate offsets (40 000 triangles in under a second), build_scalar() is the same law one pair at a
time, for small n.  Both return (nodes, search_iterations, forced_iterations).  No test lives in this file.
"""
import numpy as np

import lbvh_reference as lr
from mi3pt_host import layout

INF = np.float32(np.inf)


def sorted_leaves(tris):
    """(order, mn, mx): the triangle at every sorted position, and the boxes of the triangles in that order"""
    mn, mx = lr.triangle_boxes(tris)
    keys = lr.morton_keys(tris)
    order = np.array(sorted(range(len(keys)), key=keys.__getitem__), np.int64)          # stable
    return order, mn[order], mx[order]


def distance(mn_a, mx_a, mn_b, mx_b):
    """d of the law for rows of boxes, and the union (mn, mx)"""
    mn, mx = lr.fmin_signed(mn_a, mn_b), lr.fmax_signed(mx_a, mx_b)
    with np.errstate(all="ignore"):
        e = (mx - mn).astype(np.float32)
        x, y, z = e[..., 0], e[..., 1], e[..., 2]
        a = (((x * y).astype(np.float32) + (y * z).astype(np.float32)).astype(np.float32) + (z * x).astype(np.float32)).astype(np.float32)
    return np.where(a == a, a, INF).astype(np.float32), mn, mx


def _search(mn, mx, radius):
    """nn(i) of a search iteration for every position, C > 1"""
    C = len(mn)
    idx = np.arange(C)
    best_d = np.full(C, INF, np.float32)
    best_k = np.zeros(C, np.int64)
    best_a = np.zeros(C, np.int64)
    nn = np.full(C, -1, np.int64)

    def offer(sel, d, k, a, j):
        """candidates (d, k, a) with partner j for the positions sel: taken where the key is below the best so far"""
        bd, bk, ba = best_d[sel], best_k[sel], best_a[sel]
        tie = (d == bd) & (k == bk)
        win = (nn[sel] < 0) | (d < bd) | (tie & (((a & 1) < (ba & 1)) | (((a & 1) == (ba & 1)) & (a < ba))))
        s = sel[win]
        best_d[s], best_k[s], best_a[s], nn[s] = d[win], k, a[win], j[win]

    for k in range(1, min(radius, C - 1) + 1):              # ascending: at equal d an earlier (smaller) offset stays
        d, _, _ = distance(mn[:C - k], mx[:C - k], mn[k:], mx[k:])          # d[a] of the pair (a, a + k)
        lo = idx[:C - k]
        offer(lo + k, d, k, lo, lo)                         # the pair seen from its upper position ...
        offer(lo, d, k, lo, lo + k)                         # ... and from its lower one
    return nn


def _pairing(C):
    nn = np.arange(C) ^ 1
    nn[nn >= C] = -1
    return nn


class _Tree:
    """temporary ids: leaf p (sorted position) is p, internal nodes follow from n in the order they are made"""

    def __init__(self, order, mn, mx):
        n = len(order)
        self.n, self.order = n, order
        self.left, self.right = np.full(2 * n - 1, -1, np.int64), np.full(2 * n - 1, -1, np.int64)
        self.leaves = np.ones(2 * n - 1, np.int64)
        self.mn, self.mx = np.zeros((2 * n - 1, 3), np.float32), np.zeros((2 * n - 1, 3), np.float32)
        self.mn[:n], self.mx[:n] = mn, mx
        self.made = n

    def records(self, root):
        n = self.n
        nodes = np.zeros(2 * n - 1, layout.BVH_NODE)
        index = np.zeros(2 * n - 1, np.int64)
        work = [(int(root), 0)]
        while work:
            t, x = work.pop()
            index[t] = x
            if t >= n:
                l, r = int(self.left[t]), int(self.right[t])
                m = int(self.leaves[l])
                nodes["left"][x], nodes["right"][x] = x + 1, x + 2 * m
                work.append((r, x + 2 * m))
                work.append((l, x + 1))
        nodes["min"][index], nodes["max"][index] = self.mn, self.mx
        leaf = index[:n]
        nodes["isLeaf"][leaf] = 1
        nodes["left"][leaf] = nodes["right"][leaf] = -1
        nodes["triangleIndex"][index[n:]] = -1
        nodes["triangleIndex"][leaf] = self.order
        return nodes


def build(tris, radius=16, max_search_iterations=1024):
    """the law, vectorised: (nodes, search_iterations, forced_iterations)"""
    assert 1 <= radius <= 64 and 0 <= max_search_iterations <= 65535 and len(tris) >= 1
    order, mn, mx = sorted_leaves(tris)
    tree = _Tree(order, mn, mx)
    ids = np.arange(len(order))
    searched = forced = 0
    while len(ids) > 1:
        C = len(ids)
        if searched < max_search_iterations:
            nn, searched = _search(mn, mx, radius), searched + 1
        else:
            nn, forced = _pairing(C), forced + 1
        idx = np.arange(C)
        mutual = (nn >= 0) & (nn[np.maximum(nn, 0)] == idx)
        a = np.flatnonzero(mutual & (nn > idx))
        b = nn[a]
        assert len(a) >= 1
        _, umn, umx = distance(mn[a], mx[a], mn[b], mx[b])
        new = tree.made + np.arange(len(a))
        tree.made += len(a)
        tree.left[new], tree.right[new] = ids[a], ids[b]
        tree.leaves[new] = tree.leaves[ids[a]] + tree.leaves[ids[b]]
        tree.mn[new], tree.mx[new] = umn, umx
        mn, mx, ids = mn.copy(), mx.copy(), ids.copy()
        mn[a], mx[a], ids[a] = umn, umx, new
        keep = np.ones(C, bool)
        keep[b] = False
        mn, mx, ids = mn[keep], mx[keep], ids[keep]
    return tree.records(ids[0]), searched, forced


def _f(x):
    return np.float32(x)


def _fmin(x, y):
    """fminf: a NaN operand is dropped, -0 orders below +0"""
    if x != x:
        return y
    if y != y:
        return x
    if x == y:
        return y if np.signbit(y) else x
    return x if x < y else y


def _fmax(x, y):
    if x != x:
        return y
    if y != y:
        return x
    if x == y:
        return x if np.signbit(y) else y
    return x if x > y else y


def _union(p, q):
    return ([_fmin(p[0][c], q[0][c]) for c in range(3)], [_fmax(p[1][c], q[1][c]) for c in range(3)])


def _distance_scalar(p, q):
    mn, mx = _union(p, q)
    with np.errstate(all="ignore"):
        ex, ey, ez = _f(mx[0] - mn[0]), _f(mx[1] - mn[1]), _f(mx[2] - mn[2])
        a = _f(_f(_f(ex * ey) + _f(ey * ez)) + _f(ez * ex))
    return a if a == a else INF


def build_scalar(tris, radius=16, max_search_iterations=1024):
    """the law, one pair at a time: clusters are (box, subtree), a subtree a triangle index or a (left, right, box) triple"""
    order, mn, mx = sorted_leaves(tris)
    clusters = [(([_f(v) for v in mn[p]], [_f(v) for v in mx[p]]), int(order[p])) for p in range(len(order))]
    searched = forced = 0
    while len(clusters) > 1:
        C = len(clusters)
        nn = [None] * C
        if searched < max_search_iterations:
            searched += 1
            for i in range(C):
                best = None
                for j in range(max(0, i - radius), min(C, i + radius + 1)):
                    if j == i:
                        continue
                    a, b = min(i, j), max(i, j)
                    key = (float(_distance_scalar(clusters[a][0], clusters[b][0])), b - a, a & 1, a)
                    if best is None or key < best[0]:
                        best = (key, j)
                nn[i] = best[1]
        else:
            forced += 1
            for i in range(C):
                nn[i] = (i ^ 1) if (i ^ 1) < C else None
        out = []
        for i in range(C):
            j = nn[i]
            if j is not None and nn[j] == i:
                if i < j:
                    box = _union(clusters[i][0], clusters[j][0])
                    out.append((box, (clusters[i][1], clusters[j][1], box)))
                continue                                      # the upper position of a merged pair is removed
            out.append(clusters[i])
        assert len(out) < C
        clusters = out
    # pre-order records
    n = len(order)
    nodes = np.zeros(2 * n - 1, layout.BVH_NODE)

    def count(t):
        return 1 if isinstance(t, int) else count(t[0]) + count(t[1])

    work = [(clusters[0][1], 0)]
    while work:
        t, x = work.pop()
        if isinstance(t, int):
            p = list(order).index(t)
            nodes[x] = (mn[p], mx[p], 1, -1, -1, t)
            continue
        m = count(t[0])
        nodes[x] = (t[2][0], t[2][1], 0, x + 1, x + 2 * m, -1)
        work.append((t[1], x + 2 * m))
        work.append((t[0], x + 1))
    return nodes, searched, forced
