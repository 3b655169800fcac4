"""The law of mi3pt_device_refit_bvh (include/mi3pt.h) in plain Python, written from the header comment alone: the boxes of a tree of
48-byte records re-fitted, bottom-up, to 112-byte triangle records; every other word carried bit for bit.

    lo(x, y) = (y < x || (y == x && signbit(y))) ? y : x          hi(x, y) = (y > x || (y == x && !signbit(y))) ? y : x
    leaf:      min = lo(lo(a, b), c), max = hi(hi(a, b), c)       a, b, c = the positions of triangle record `triangleIndex`
    internal:  min = lo(min(left), min(right)), max = hi(max(left), max(right))      always left then right

Two forms: refit_scalar walks the tree node by node with Python floats holding fp32 values (min / max never round, so no arithmetic
leaves fp32); refit_vectorised does the leaves at once and the internal nodes level by level from the deepest, for trees of tens of
thousands of nodes.  bvh_cost is mi3pt_host_bvh_cost in float64.  No test lives here."""
import numpy as np

from mi3pt_host import layout

F = np.float32


def lo(x, y):
    """fp32 scalars"""
    x, y = F(x), F(y)
    return y if (y < x or (y == x and np.signbit(y))) else x


def hi(x, y):
    x, y = F(x), F(y)
    return y if (y > x or (y == x and not np.signbit(y))) else x


def lo_v(x, y):
    """elementwise on fp32 arrays (comparisons with a NaN are false: a NaN y is dropped, a NaN x kept)"""
    with np.errstate(invalid="ignore"):
        take = (y < x) | ((y == x) & np.signbit(y))
    return np.where(take, y, x).astype(F)


def hi_v(x, y):
    with np.errstate(invalid="ignore"):
        take = (y > x) | ((y == x) & ~np.signbit(y))
    return np.where(take, y, x).astype(F)


def _records(nodes):
    # (a copy of the BYTES: copying a structured array leaves its padding words, 3 and 11, behind)
    return np.ascontiguousarray(nodes).view(np.uint8).reshape(-1).copy().view(layout.BVH_NODE)


def _triangles(tris):
    return np.ascontiguousarray(tris).view(np.uint8).reshape(-1).view(layout.TRIANGLE)


def refit_scalar(nodes, tris):
    """One node at a time, children before parents (an explicit stack: a chain of 62 levels is no recursion problem, but why recurse)."""
    out, tris = _records(nodes), _triangles(tris)
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        if out["isLeaf"][i] != 1:
            stack.append(int(out["left"][i]))
            stack.append(int(out["right"][i]))
    for i in reversed(order):                      # every node after both of its children
        if out["isLeaf"][i] == 1:
            t = tris[int(out["triangleIndex"][i])]
            a, b, c = t["aPosition"], t["bPosition"], t["cPosition"]
            for k in range(3):
                out["min"][i][k] = lo(lo(a[k], b[k]), c[k])
                out["max"][i][k] = hi(hi(a[k], b[k]), c[k])
        else:
            l, r = int(out["left"][i]), int(out["right"][i])
            for k in range(3):
                out["min"][i][k] = lo(out["min"][l][k], out["min"][r][k])
                out["max"][i][k] = hi(out["max"][l][k], out["max"][r][k])
    return out


def levels(nodes):
    """depth of every node below node 0 (-1: the root does not reach it)"""
    left, right, leaf = nodes["left"], nodes["right"], nodes["isLeaf"] == 1
    depth = np.full(len(nodes), -1, np.int64)
    depth[0] = 0
    front, d = np.array([0]), 0
    while len(front):
        inner = front[~leaf[front]]
        front = np.concatenate([left[inner], right[inner]]).astype(np.int64)
        d += 1
        depth[front] = d
    return depth


def refit_vectorised(nodes, tris):
    out, tris = _records(nodes), _triangles(tris)
    depth = levels(out)
    leaf = (out["isLeaf"] == 1) & (depth >= 0)
    t = tris[out["triangleIndex"][leaf]]
    a, b, c = t["aPosition"], t["bPosition"], t["cPosition"]
    mn, mx = out["min"].copy(), out["max"].copy()
    mn[leaf] = lo_v(lo_v(a, b), c)
    mx[leaf] = hi_v(hi_v(a, b), c)
    for d in range(int(depth.max()), -1, -1):
        at = np.flatnonzero((depth == d) & ~leaf)
        l, r = out["left"][at], out["right"][at]
        mn[at] = lo_v(mn[l], mn[r])
        mx[at] = hi_v(mx[l], mx[r])
    out["min"], out["max"] = mn, mx
    return out


def bvh_cost(nodes):
    """mi3pt_host_bvh_cost: area = 2 * ((x*y + x*z) + y*z) of max - min in double, all records added in index order, over node 0's"""
    n = _records(nodes)
    e = n["max"].astype(np.float64) - n["min"].astype(np.float64)
    x, y, z = e[:, 0], e[:, 1], e[:, 2]
    area = 2.0 * ((x * y + x * z) + y * z)
    total = np.cumsum(area)[-1]                    # (cumsum adds one after the other; np.sum adds pairwise)
    return 0.0 if area[0] == 0.0 else float(total / area[0])


def first_difference(got, want):
    """None, or where two record arrays first differ word for word"""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1).view("<u4").reshape(-1, 12)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1).view("<u4").reshape(-1, 12)
    if g.shape != w.shape:
        return f"{g.shape[0]} records, want {w.shape[0]}"
    bad = np.argwhere(g != w)
    if not len(bad):
        return None
    i, k = (int(v) for v in bad[0])
    return f"{len(set(bad[:, 0].tolist()))} records differ; first: record {i} word {k}: {g[i, k]:#010x}, want {w[i, k]:#010x}"


def moved_demo(slide=0.6, turn_deg=30.0):
    """The demo scene (main.ts:36-75) with its box slid by `slide` along x and turned by `turn_deg` about y: same triangle count, index i
    the same surface element."""
    import math
    from mi3pt_host import scenes
    q = scenes.quaternion_from_axis_angle((0.0, 1.0, 0.0), math.radians(turn_deg))
    parts = [scenes._ground_plane(),
             scenes.flatten_mesh(scenes.box_geometry(0.8, 0.8, 0.8), scenes.compose_matrix(position=(slide, 0.4, 0.5), quaternion=q), 1),
             scenes.flatten_mesh(scenes.sphere_geometry(0.5, 32, 32), scenes.compose_matrix(position=(0.0, 0.5, -0.5)), 0)]
    return scenes.Scene(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                        np.concatenate([p[2] for p in parts]), [scenes.WHITE, scenes.RED], "demo-moved")


def chain(internal=62):
    """A chain: `internal` internal nodes, each with a leaf on the left and the rest of the chain on the right, two leaves at the end --
    internal + 1 levels; the thread of a bottom leaf climbs the whole height.  Boxes as uploaded are wrong on purpose (zero): the refit
    has to produce every one.  (nodes, triangles)"""
    ntri = internal + 1
    rng = np.random.default_rng(internal)
    pos = rng.normal(size=(ntri, 3, 3)) + np.arange(ntri)[:, None, None] * 0.5
    tris = layout.pack_triangles(pos, np.tile([0.0, 0.0, 1.0], (ntri, 3, 1)), np.zeros(ntri, int))
    nodes = np.zeros(2 * ntri - 1, layout.BVH_NODE)
    nodes["left"], nodes["right"], nodes["triangleIndex"] = -1, -1, -1
    for k in range(internal):
        i = 2 * k
        nodes["left"][i], nodes["right"][i] = i + 1, i + 2
        nodes["isLeaf"][i + 1], nodes["triangleIndex"][i + 1] = 1, k
    last = 2 * internal
    nodes["isLeaf"][last], nodes["triangleIndex"][last] = 1, internal
    return nodes, tris
