"""Reference for the device-built linear BVH (mi3pt_device_build_bvh), written from the header comment of csrc/pt_lbvh.hip and the
arithmetic the library is compiled with (fp32, no contraction, correctly rounded division): numpy and plain Python only.

Per triangle the NaN-ignoring box of its three vertices and the centroid fl(fl(0.5 mn) + fl(0.5 mx)); the bounds of the non-NaN
centroids; per axis t = (c - lo) / extent (0 unless extent > 0), clamped to [0, 1] with NaN -> 0, q = uint(min(t 2^21, 2^21 - 1));
the 63-bit key interleaves x, y, z with x highest; a stable sort by key; the binary radix tree over (key << 32 | sorted position),
built top-down and numbered in pre-order; boxes united bottom-up with fmin / fmax, where -0 counts as below +0 (fmin_signed /
fmax_signed: the refit's lo / hi on everything but a NaN).  first_difference compares boxes as values, first_word_difference as words
(the zeros and subnormals of tests/box_law_cases.py).  Nothing here looks at the device.  No test
lives in this file; check_tree is the structural check both LBVH test files share, and the input classes they share are below it.
"""
from bisect import bisect_left

import numpy as np

from mi3pt_host import layout

BITS = 21                        # per axis
CELLS = np.float32(1 << BITS)
PAD_OFFSETS = (12, 44)           # the two padding words of a 48-byte node record (after min, after triangleIndex)


def fmin_signed(x, y):
    """fminf with the zero rule spelled out: of two equal operands -- +0 and -0 compare equal -- the negative one, so -0 wins a minimum
    whatever the order (the refit's lo, include/mi3pt.h, on everything but a NaN; C leaves fminf(+0, -0) open).  NaNs as np.fmin."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x == y, np.where(np.signbit(y), y, x), np.fmin(x, y)).astype(np.float32)


def fmax_signed(x, y):
    """fmaxf; of two equal operands the positive one: +0 wins a maximum whatever the order"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x == y, np.where(np.signbit(y), x, y), np.fmax(x, y)).astype(np.float32)


def triangle_boxes(tris):
    """(mn, mx): n x 3 fp32 each; a NaN coordinate is ignored unless all three vertices have it (fminf / fmaxf); -0 < +0."""
    a, b, c = (np.asarray(tris[k], np.float32) for k in ("aPosition", "bPosition", "cPosition"))
    return fmin_signed(fmin_signed(a, b), c), fmax_signed(fmax_signed(a, b), c)


def centroids(mn, mx):
    half = np.float32(0.5)
    with np.errstate(all="ignore"):
        return (half * mn).astype(np.float32) + (half * mx).astype(np.float32)


def quantise(cen):
    """n x 3 cell numbers in [0, 2^21 - 1] (Python-int friendly uint64)."""
    n = len(cen)
    q = np.zeros((n, 3), np.uint64)
    with np.errstate(all="ignore"):
        for k in range(3):
            c = cen[:, k]
            ok = c[~np.isnan(c)]
            lo, hi = (ok.min(), ok.max()) if len(ok) else (np.float32(np.nan), np.float32(np.nan))
            extent = np.float32(hi - lo)
            if extent > 0:
                t = ((c - lo).astype(np.float32) / extent).astype(np.float32)
            else:
                t = np.zeros(n, np.float32)
            t = np.fmin(np.fmax(t, np.float32(0)), np.float32(1))
            t[np.isnan(t)] = 0
            q[:, k] = np.fmin((t * CELLS).astype(np.float32), np.float32((1 << BITS) - 1)).astype(np.uint64)
    return q


def interleave(qx, qy, qz):
    """bit b of x, y, z -> bits 3b + 2, 3b + 1, 3b of the key (uint64 arrays), one bit at a time"""
    key = np.zeros(len(qx), np.uint64)
    one = np.uint64(1)
    for b in range(BITS):
        key |= ((qx >> np.uint64(b)) & one) << np.uint64(3 * b + 2)
        key |= ((qy >> np.uint64(b)) & one) << np.uint64(3 * b + 1)
        key |= ((qz >> np.uint64(b)) & one) << np.uint64(3 * b)
    return key


def morton_keys(tris):
    """The key of every triangle, in triangle order, as Python ints."""
    q = quantise(centroids(*triangle_boxes(tris)))
    return interleave(q[:, 0], q[:, 1], q[:, 2]).tolist()


def reference_nodes(tris):
    """The (2n - 1) node records the builder has to write for these triangle records."""
    n = len(tris)
    assert n >= 1
    mn, mx = triangle_boxes(tris)
    keys = morton_keys(tris)
    order = sorted(range(n), key=keys.__getitem__)                    # stable: equal keys keep ascending triangle index
    code = [(keys[t] << 32) | pos for pos, t in enumerate(order)]     # strictly ascending
    total = 2 * n - 1
    left, right, tri, level = [-1] * total, [-1] * total, [-1] * total, [0] * total
    work = [(0, 0, n - 1, 0)]                                         # (index, first position, last position, level)
    while work:
        idx, lo, hi, lev = work.pop()
        level[idx] = lev
        if lo == hi:
            tri[idx] = order[lo]
            continue
        bit = (code[lo] ^ code[hi]).bit_length() - 1
        first_set = ((code[lo] >> bit) | 1) << bit                    # the smallest code of this range's prefix with `bit` set
        split = bisect_left(code, first_set, lo, hi + 1)              # positions lo .. split - 1 have the bit clear
        left[idx], right[idx] = idx + 1, idx + 2 * (split - lo)
        work.append((right[idx], split, hi, lev + 1))
        work.append((left[idx], lo, split - 1, lev + 1))
    nodes = np.zeros(total, layout.BVH_NODE)                          # (padding words: 0)
    nodes["left"], nodes["right"], nodes["triangleIndex"] = left, right, tri
    level = np.array(level)
    leaf = nodes["triangleIndex"] >= 0
    nodes["isLeaf"] = leaf
    nodes["min"][leaf], nodes["max"][leaf] = mn[nodes["triangleIndex"][leaf]], mx[nodes["triangleIndex"][leaf]]
    for lev in range(int(level.max()) - 1, -1, -1):                   # children first
        sel = np.flatnonzero((level == lev) & (nodes["isLeaf"] == 0))
        l, r = nodes["left"][sel], nodes["right"][sel]
        nodes["min"][sel] = fmin_signed(nodes["min"][l], nodes["min"][r])
        nodes["max"][sel] = fmax_signed(nodes["max"][l], nodes["max"][r])
    return nodes


def depth(nodes):
    """Levels of the tree: nodes on the longest path from the root to a leaf (a single leaf: 1)."""
    level = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):                                       # a child comes after its parent
        if nodes["isLeaf"][i] != 1:
            level[nodes["left"][i]] = level[nodes["right"][i]] = level[i] + 1
    return int(level.max()) + 1


def leaves_in_order(nodes):
    """triangleIndex of the leaves from left to right"""
    out, work = [], [0]
    while work:
        i = work.pop()
        if nodes["isLeaf"][i] == 1:
            out.append(int(nodes["triangleIndex"][i]))
        else:
            work.append(int(nodes["right"][i]))
            work.append(int(nodes["left"][i]))
    return out


def padding_words(nodes):
    return np.ascontiguousarray(nodes).view(np.uint8).reshape(len(nodes), 48)[:, [o + k for o in PAD_OFFSETS for k in range(4)]]


def check_tree(nodes, tris, boxes=True):
    """A proper binary tree over the triangles in the order mi3pt_upload_bvh wants.  boxes=False leaves the box checks out: they
    compare with NaN-propagating minima, which an input with NaN vertices cannot meet."""
    n = len(tris)
    assert len(nodes) == 2 * n - 1
    leaf = nodes["isLeaf"] == 1
    assert leaf.sum() == n and sorted(nodes["triangleIndex"][leaf].tolist()) == list(range(n))
    inner = np.flatnonzero(~leaf)
    idx = np.arange(len(nodes))
    assert (nodes["left"][inner] > idx[inner]).all() and (nodes["right"][inner] > idx[inner]).all()
    assert (nodes["left"][leaf] == -1).all() and (nodes["right"][leaf] == -1).all() and (nodes["triangleIndex"][inner] == -1).all()
    # every node except the root has exactly one parent
    refs = np.concatenate([nodes["left"][inner], nodes["right"][inner]])
    assert sorted(refs.tolist()) == list(range(1, len(nodes)))
    if not boxes:
        return
    # boxes: leaves bound their triangle exactly, inner nodes are the union of their children
    p = np.stack([tris["aPosition"], tris["bPosition"], tris["cPosition"]], 1)[nodes["triangleIndex"][leaf]]
    assert np.array_equal(nodes["min"][leaf], p.min(1)) and np.array_equal(nodes["max"][leaf], p.max(1))
    l, r = nodes["left"][inner], nodes["right"][inner]
    assert np.array_equal(nodes["min"][inner], np.minimum(nodes["min"][l], nodes["min"][r]))
    assert np.array_equal(nodes["max"][inner], np.maximum(nodes["max"][l], nodes["max"][r]))


def first_difference(got, want, equal_nan=False):
    """None when the two node arrays agree (integer fields and padding bit for bit, boxes as fp32 values), else a description of the
    first node that differs."""
    if len(got) != len(want):
        return f"{len(got)} nodes, reference {len(want)}"
    bad = np.zeros(len(want), bool)
    for f in ("isLeaf", "left", "right", "triangleIndex"):
        bad |= got[f] != want[f]
    bad |= (padding_words(got) != padding_words(want)).any(1)
    for f in ("min", "max"):
        ne = got[f] != want[f]
        if equal_nan:
            ne &= ~(np.isnan(got[f]) & np.isnan(want[f]))
        bad |= ne.any(1)
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    return (f"{int(bad.sum())} of {len(want)} nodes differ; first at {i}:\n  device    {got[i]} pad {padding_words(got)[i].tolist()}"
            f"\n  reference {want[i]} pad {padding_words(want)[i].tolist()}")


def first_word_difference(got, want):
    """None when the two node arrays hold the same twelve 32-bit words in every record -- the boxes too, so +0 is not -0 -- else a
    description of the first word that differs.  For inputs without a NaN (the words of a NaN box are not pinned)."""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1).view("<u4").reshape(-1, 12)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1).view("<u4").reshape(-1, 12)
    if g.shape != w.shape:
        return f"{g.shape[0]} nodes, reference {w.shape[0]}"
    bad = np.argwhere(g != w)
    if not len(bad):
        return None
    i, k = (int(v) for v in bad[0])
    return (f"{len(set(bad[:, 0].tolist()))} of {len(w)} nodes differ in {len(bad)} words; first at node {i}, word {k}: "
            f"device {g[i, k]:#010x}, reference {w[i, k]:#010x}")


# ---- the input classes both test files use (positions: n x 3 vertices x 3 coordinates, float64 that fp32 holds exactly or rounds)

def pack(pos):
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    return layout.pack_triangles(pos, np.tile([0.0, 0.0, 1.0], (n, 3, 1)), np.zeros(n, int))


def random_triangles(n, seed=None):
    """rng.normal triangles scaled by 0.05 about rng.uniform(-1, 1) centres"""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    return rng.uniform(-1, 1, (n, 1, 3)) + 0.05 * rng.normal(size=(n, 3, 3))


def degenerate(layout_name, n=300):
    """centroids in the plane z = 0 / on the line y = z = 0 / at the origin: on those axes every box is [-e, +e]"""
    rng = np.random.default_rng(7)
    cen = rng.uniform(-1, 1, (n, 3))
    cen[:, {"plane": slice(2, 3), "line": slice(1, 3), "point": slice(0, 3)}[layout_name]] = 0.0
    e = rng.uniform(0.01, 0.1, (n, 3))
    return np.stack([cen - e, cen + e * np.array([1.0, -1.0, 1.0]), cen + e], 1)


def repeated(distinct, copies, seed=3):
    """`distinct` random triangles, each `copies` times, interleaved (0 1 2 .. 0 1 2 ..): runs of equal keys"""
    return np.tile(random_triangles(distinct, seed), (copies, 1, 1))


def chain():
    """65 point-like triangles whose keys are 0, every single bit 2^0 .. 2^62 and all ones: the deepest tree distinct keys allow"""
    pts = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)]
    for k in range(3):
        for j in range(BITS):
            p = [0.0, 0.0, 0.0]
            p[k] = 2.0 ** j / 2.0 ** BITS
            pts.append(tuple(p))
    pts = np.array(pts)
    pts = pts[np.random.default_rng(5).permutation(len(pts))]
    return np.repeat(pts[:, None, :], 3, 1)


def grid(cells=8, seed=11):
    """One small triangle in every cell of a cells^3 grid (integer corner plus a jitter below 0.01), shuffled.
    Returns (positions, the integer cell of every triangle)."""
    rng = np.random.default_rng(seed)
    ijk = np.stack(np.meshgrid(*[np.arange(cells)] * 3, indexing="ij"), -1).reshape(-1, 3)
    ijk = ijk[rng.permutation(len(ijk))]
    return ijk[:, None, :] + rng.uniform(0.0, 0.01, (len(ijk), 3, 3)), ijk


def range_extremes(n=64, axes=3):
    """coordinates up to 3e38 with mixed signs on the first `axes` axes (hi - lo overflows there), ordinary ones on the others"""
    rng = np.random.default_rng(13)
    pos = random_triangles(n, 17)
    big = rng.uniform(-3e38, 3e38, (n, 3, 3))
    big[0, :, :] = 3e38
    big[1, :, :] = -3e38
    pos[:, :, :axes] = big[:, :, :axes]
    return pos


def non_finite():
    """64 ordinary triangles, one with a single NaN vertex, one with all nine coordinates NaN (index 65)"""
    pos = random_triangles(66, 19)
    pos[64, 1, :] = np.nan
    pos[65] = np.nan
    return pos
