"""Irregular BVHs: node buffers mi3pt_upload_bvh accepts (children after their parents, leaves that name uploaded triangles) that
no builder of this project makes -- a leaf as root, internal nodes without a child, subtrees with two parents, triangles with two
leaves, nodes the root never reaches, isLeaf values other than 0 and 1, boxes that are NaN, infinite, inverted or empty.  The
reference's walk (raytrace.wgsl:154-211) gives each of them a defined image; the context decides from them which walk may run
(tree_proper, leaf_cap, cull_stack_ok, wide_ok, cwide_ok, cw8_ok, the sky cut).

Inputs only: no GPU, no pytest, no test lives here.  tests/test_irregular_trees.py shows on the CPU that every case is what it says and
can be told from the builder's tree by the oracle; tests/test_gpu_irregular_trees.py renders them.

Every tree of cases() satisfies the upload's preconditions (precondition_violations: what bounds every walk on the device); the
trees of refused() each break one of them and are never rendered.  Node arrays are edited through the structured dtype and grown
with _append (np.concatenate of node arrays would drop the record padding: stride 40)."""
import functools

import numpy as np

import ptcommon as pc
from mi3pt_host import layout, scenes


class _Camera:
    """the demo camera (main.ts:38-39), what a case's camera keywords override"""
    camera = dict(position=(0.0, 1.0, 4.0), target=(0.0, 0.0, 0.0), fov=45.0, focalDistance=1.0, aperture=0.0)

    @staticmethod
    def camera_direction():
        d = np.array([0.0, -1.0, -4.0])
        return d / np.sqrt(float(d @ d))


CAMERA = _Camera
# the names of cases() and of refused(), spelt out: what the tests are parametrised over (building the cases needs the library)
CASE_NAMES = ("missing children", "shared subtrees", "shared coincident sheets", "doubly owned triangles", "doubly owned triangles, union boxes",
              "isLeaf other than 0 and 1", "unreachable leaves", "unreachable internal node", "bad boxes", "bad boxes on leaves",
              "bad boxes on internal nodes", "leaf root", "two triangles", "three triangles")
REFUSED_NAMES = ("child equal to its parent", "child before its parent", "child beyond the buffer", "unreachable node with a backward link",
                 "reachable leaf with a negative triangle", "unreachable leaf with a negative triangle", "leaf beyond the triangles")
# bound_cases(): comb trees on either side of the deferred-leaf bound (internal entries of the reference's order against the LDS slots)
# and of the culling walks' stack bound
BOUND_NAMES = ("comb 19", "comb 20", "comb 55", "comb 56")
DEMO_VIEW = {}                                                   # the demo camera: floor, box and sphere below, sky above
# the cases whose reachable part is the builder's tree, node for node: the oracle must NOT tell them from it
UNREACHABLE = ("unreachable leaves", "unreachable internal node")
# the builder's own trees of two and three triangles: irregular only in being tiny (a root with two leaves; a root with a leaf and a node)
BUILDER_MADE = ("two triangles", "three triangles")
# refused(): turned away by check_scene at submit / render_aovs / the probes (a state error); all others by the upload itself
REFUSED_AT_SUBMIT = ("leaf beyond the triangles",)


def uniforms(cam_kw, w, h, frame=2, bounces=4, **more):
    """The raytrace uniform block of a case's camera."""
    return pc.rt_uniforms(CAMERA, w, h, frame=frame, bounces=bounces, **dict(cam_kw, **more))


def precondition_violations(nodes, triangles, nmats):
    """What mi3pt_upload_bvh, mi3pt_upload_triangles and the scene check ask of the buffers, in plain numpy: a list of texts, empty when
    the scene may be rendered.  Every child index of a non-leaf node negative, or greater than its parent's and inside the buffer; every
    isLeaf == 1 node with 0 <= triangleIndex < triangles; every material index inside the material buffer."""
    out = []
    if nodes.dtype != layout.BVH_NODE or nodes.strides != (48,):
        return [f"node records: dtype / stride {nodes.dtype.itemsize} / {nodes.strides}"]
    n, nt = len(nodes), len(triangles)
    if n == 0:
        return ["no nodes"]
    idx = np.arange(n)
    leaf = nodes["isLeaf"] == 1
    for side in ("left", "right"):
        c = nodes[side].astype(np.int64)
        bad = ~leaf & (c >= 0) & ((c <= idx) | (c >= n))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            out.append(f"{int(bad.sum())} {side} links not after their parent or outside the buffer, first: node {i} -> {int(c[i])}")
    ti = nodes["triangleIndex"].astype(np.int64)
    bad = leaf & ((ti < 0) | (ti >= nt))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        out.append(f"{int(bad.sum())} leaves name no uploaded triangle, first: node {i} -> {int(ti[i])} of {nt}")
    mi = triangles["materialIndex"].astype(np.int64)
    bad = (mi < 0) | (mi >= nmats)
    if bad.any():
        out.append(f"{int(bad.sum())} triangles name no uploaded material")
    return out


def _append(nodes, count):
    """`nodes` with `count` zeroed records behind it (isLeaf 0, children -1: internal nodes without children until they are filled in)"""
    out = np.zeros(len(nodes) + count, layout.BVH_NODE)
    out[:len(nodes)] = nodes
    out["left"][len(nodes):] = -1
    out["right"][len(nodes):] = -1
    out["triangleIndex"][len(nodes):] = -1
    return out


def _put_leaf(nodes, i, tri, mn, mx):
    nodes["min"][i], nodes["max"][i] = mn, mx
    nodes["isLeaf"][i], nodes["left"][i], nodes["right"][i], nodes["triangleIndex"][i] = 1, -1, -1, tri


def _put_node(nodes, i, left, right, mn, mx, is_leaf=0):
    nodes["min"][i], nodes["max"][i] = mn, mx
    nodes["isLeaf"][i], nodes["left"][i], nodes["right"][i], nodes["triangleIndex"][i] = is_leaf, left, right, -1


def _spoil_boxes(nodes, picks):
    """Seven kinds of box that are no box, dealt in turn: one NaN coordinate, all NaN, (-inf, +inf) on every axis (every ray passes),
    min = +inf (none does), max = -inf, min and max swapped, max := min (an empty box: a point)."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for k, i in enumerate(picks):
        kind = k % 7
        mn, mx = nodes["min"][i].copy(), nodes["max"][i].copy()
        if kind == 0:
            mn[k % 3] = nan
        elif kind == 1:
            mn[:], mx[:] = nan, nan
        elif kind == 2:
            mn[:], mx[:] = -inf, inf
        elif kind == 3:
            mn[:] = inf
        elif kind == 4:
            mx[:] = -inf
        elif kind == 5:
            mn, mx = mx, mn
        else:
            mx = mn.copy()
        nodes["min"][i], nodes["max"][i] = mn, mx


def _hand_made(positions, material_index, materials):
    pos = np.array(positions, np.float64)
    e1, e2 = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    tris = layout.pack_triangles(pos, np.repeat(nrm[:, None, :], 3, 1), np.array(material_index))
    return tris, layout.pack_materials(materials), pos.astype(np.float32)


RED_LIGHT = dict(color=(0.9, 0.1, 0.1), roughness=1.0, metalness=0.0, specularColor=(1, 1, 1), emissive=(1.0, 0.1, 0.05), emissiveIntensity=2.0)
GREEN_LIGHT = dict(color=(0.1, 0.9, 0.1), roughness=1.0, metalness=0.0, specularColor=(1, 1, 1), emissive=(0.05, 1.0, 0.1), emissiveIntensity=3.0)


@functools.lru_cache(maxsize=None)
def demo():
    sc = scenes.demo_scene()
    sc.build_bvh()
    return sc


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (nodes, triangles, material bytes, camera keywords) in the reference's layouts.  Built once; callers do not write into them."""
    d = demo()
    base, tris, mats = d.nodes, d.triangles, d.material_bytes
    n = len(base)
    leaves, internal = np.flatnonzero(base["isLeaf"] == 1), np.flatnonzero(base["isLeaf"] != 1)
    out = {}

    # ---- 300 internal nodes lose the left child, the right child or both (the top four levels keep theirs: most of the scene stays)
    rng = np.random.default_rng(11)
    nodes = base.copy()
    for i, kind in zip(rng.choice(internal[internal >= 16], 300, replace=False), rng.integers(0, 3, 300)):
        if kind != 1:
            nodes["left"][i] = -1
        if kind != 0:
            nodes["right"][i] = -1
    out["missing children"] = (nodes, tris, mats, DEMO_VIEW)

    # ---- 300 right links redirected to a LATER node whose two children are leaves: that node has two (or more) parents, what the link
    # named before is no longer reached.  The shared nodes hold no link themselves, so the walk grows by three visits per redirection.
    rng = np.random.default_rng(12)
    nodes = base.copy()
    twigs = np.array([i for i in internal if base["isLeaf"][base["left"][i]] == 1 and base["isLeaf"][base["right"][i]] == 1])
    others = np.setdiff1d(internal, twigs)
    for i in rng.choice(others[(others >= 4) & (others < twigs.max())], 300, replace=False):
        nodes["right"][i] = rng.choice(twigs[twigs > i])
    out["shared subtrees"] = (nodes, tris, mats, DEMO_VIEW)

    # ---- a shared subtree whose two leaves are coincident copies with different lights: the reference tests the right leaf first and
    # keeps it (a later equal t does not replace a hit), on the first visit and on both revisits
    pos = [[(-2.0, 0.0, 2.0), (2.0, 0.0, 2.0), (0.0, 0.0, -3.0)],           # 0: floor
           [(-0.8, 0.1, 0.0), (0.8, 0.1, 0.0), (0.0, 1.5, 0.0)],            # 1: panel, red light
           [(-0.8, 0.1, 0.0), (0.8, 0.1, 0.0), (0.0, 1.5, 0.0)],            # 2: the same panel, green light
           [(-0.3, 0.3, 0.8), (0.5, 0.3, 0.8), (0.1, 0.9, 0.8)]]            # 3: a small triangle in front of it
    t4, m4, p32 = _hand_made(pos, [0, 1, 2, 0], [scenes.WHITE, RED_LIGHT, GREEN_LIGHT])
    box = lambda *ts: (p32[list(ts)].reshape(-1, 3).min(0), p32[list(ts)].reshape(-1, 3).max(0))
    nodes = _append(np.zeros(0, layout.BVH_NODE), 8)
    _put_node(nodes, 0, 1, 5, *box(0, 1, 2, 3))
    _put_node(nodes, 1, 2, 3, *box(0, 1, 2, 3))
    _put_leaf(nodes, 2, 0, *box(0))
    _put_node(nodes, 3, 4, 5, *box(1, 2, 3))
    _put_leaf(nodes, 4, 3, *box(3))
    _put_node(nodes, 5, 6, 7, *box(1, 2))                                     # the shared node: parents 0 and 3
    _put_leaf(nodes, 6, 2, *box(2))
    _put_leaf(nodes, 7, 1, *box(1))                                           # (the builder's tree of these triangles tests the green copy first)
    out["shared coincident sheets"] = (nodes, t4, m4, DEMO_VIEW)

    # ---- 100 leaves renamed to another leaf's triangle (their own is lost, the other one has two owners); the leaves of the red box
    # (triangles 2 .. 13) are among them, so that the loss shows from the demo camera
    rng = np.random.default_rng(13)
    nodes = base.copy()
    leaf_of = np.zeros(len(tris), int)
    leaf_of[base["triangleIndex"][leaves]] = leaves
    renamed = np.unique(np.concatenate([leaf_of[2:14], rng.choice(leaves, 88, replace=False)]))
    donors = rng.choice(np.setdiff1d(leaves, renamed), len(renamed), replace=False)
    nodes["triangleIndex"][renamed] = base["triangleIndex"][donors]
    out["doubly owned triangles"] = (nodes, tris, mats, DEMO_VIEW)

    # ---- ... and with the union of the two boxes on both owners: the same rays reach both, the second test of the triangle is a tie
    rng = np.random.default_rng(14)
    nodes = base.copy()
    pairs = rng.choice(leaves, 200, replace=False).reshape(100, 2)
    for a, b in pairs:
        nodes["triangleIndex"][b] = base["triangleIndex"][a]
        mn, mx = np.minimum(base["min"][a], base["min"][b]), np.maximum(base["max"][a], base["max"][b])
        nodes["min"][a], nodes["max"][a], nodes["min"][b], nodes["max"][b] = mn, mx, mn, mx
    out["doubly owned triangles, union boxes"] = (nodes, tris, mats, DEMO_VIEW)

    # ---- isLeaf other than 0 and 1: anything but 1 is an internal node (raytrace.wgsl:180) -- 90 leaves become internal nodes without
    # children (their triangle is lost), 60 internal nodes carry a 3 and stay what they are
    rng = np.random.default_rng(15)
    nodes = base.copy()
    for k, i in enumerate(rng.choice(leaves, 90, replace=False)):
        nodes["isLeaf"][i] = (2, -1, 0)[k % 3]
    nodes["isLeaf"][rng.choice(internal, 60, replace=False)] = 3
    out["isLeaf other than 0 and 1"] = (nodes, tris, mats, DEMO_VIEW)

    # ---- nodes the root never reaches, behind the un-edited tree.  Leaves only: each names a triangle that a reachable leaf owns (the
    # floor, the red box, part of the sphere) with a box that is nowhere near it, empty, inverted, huge, NaN or infinite
    rng = np.random.default_rng(16)
    named = np.concatenate([np.arange(14), rng.choice(np.arange(14, len(tris)), 26, replace=False)])
    nodes = _append(base, len(named))
    for k, t in enumerate(named):
        c = rng.uniform(40.0, 50.0, 3).astype(np.float32)
        mn, mx = [(c, c + np.float32(0.01)), (c, c), (c + np.float32(1.0), c), (np.float32(-60.0) + 0 * c, np.float32(60.0) + 0 * c),
                  (c * np.float32(np.nan), c), (c - np.float32(np.inf), c + np.float32(np.inf))][k % 6]
        _put_leaf(nodes, n + k, int(t), mn, mx)
    out["unreachable leaves"] = (nodes, tris, mats, DEMO_VIEW)
    # ... and an internal node with two leaves behind it, boxes around the whole scene
    nodes = _append(base, 3)
    _put_node(nodes, n, n + 1, n + 2, base["min"][0] - np.float32(1.0), base["max"][0] + np.float32(1.0))
    _put_leaf(nodes, n + 1, 0, base["min"][0], base["max"][0])
    _put_leaf(nodes, n + 2, 5, base["min"][0] - np.float32(1.0), base["max"][0])
    out["unreachable internal node"] = (nodes, tris, mats, DEMO_VIEW)

    # ---- boxes that are NaN, infinite, inverted or empty (the root keeps its own): on any node, on leaves only, on internal nodes only
    for name, seed, pool in (("bad boxes", 18, np.arange(1, n)), ("bad boxes on leaves", 19, leaves), ("bad boxes on internal nodes", 20, internal[internal >= 1])):
        rng = np.random.default_rng(seed)
        nodes = base.copy()
        _spoil_boxes(nodes, rng.choice(pool, 120, replace=False))
        out[name] = (nodes, tris, mats, DEMO_VIEW)

    # ---- a leaf as root: one triangle, a box with room around it (more rays test the triangle than under the builder's tight box)
    t1, m1, p32 = _hand_made([[(-1.2, 0.0, 0.0), (1.2, 0.0, -0.5), (0.0, 1.6, -0.2)]], [0], [RED_LIGHT])
    nodes = _append(np.zeros(0, layout.BVH_NODE), 1)
    _put_leaf(nodes, 0, 0, p32[0].min(0) - np.float32(0.25), p32[0].max(0) + np.float32(0.25))
    out["leaf root"] = (nodes, t1, m1, DEMO_VIEW)

    # ---- the builder's own smallest trees with an internal root
    rng = np.random.default_rng(21)
    for name, k in zip(BUILDER_MADE, (2, 3)):
        p = rng.normal(size=(k, 3, 3)) * 0.8 + np.array([0.0, 0.6, 0.0])
        sc = scenes.Scene(p, np.tile(np.array([0.0, 0.0, 1.0]), (k, 3, 1)), np.arange(k) % 2, [scenes.WHITE, RED_LIGHT], name)
        sc.build_bvh()
        out[name] = (sc.nodes, sc.triangles, sc.material_bytes, DEMO_VIEW)
    return out


def _comb(depth):
    """A proper tree with an internal root that is DEEP in the walks' sense: a spine of `depth` internal nodes, each with an internal side
    branch of two leaves (left) and the rest of the spine (right), two leaves at the end.  The reference's order stacks one side branch
    per level.  (nodes, triangles)"""
    ntri = 2 * depth + 2
    pos = np.array([[[0.25 + 0.3 * (t % 2), -0.4, -40.0 + t // 2], [0.5 + 0.3 * (t % 2), -0.4, -40.0 + t // 2], [0.35 + 0.3 * (t % 2), 0.5, -40.0 + t // 2]]
                    for t in range(ntri)])
    tris = layout.pack_triangles(pos, np.tile(np.array([0.0, 0.0, 1.0]), (ntri, 3, 1)), np.zeros(ntri, int))
    nodes = _append(np.zeros(0, layout.BVH_NODE), 2 * ntri - 1)
    box = lambda k0, k1: ((-1.0, -1.0, -40.1 + k0), (1.0, 1.0, -39.9 + k1))
    i = 0
    for k in range(depth):
        _put_node(nodes, i, i + 1, i + 4, *box(k, depth))
        _put_node(nodes, i + 1, i + 2, i + 3, *box(k, k))
        _put_leaf(nodes, i + 2, 2 * k, *box(k, k))
        _put_leaf(nodes, i + 3, 2 * k + 1, *box(k, k))
        i += 4
    _put_node(nodes, i, i + 1, i + 2, *box(depth, depth))
    _put_leaf(nodes, i + 1, 2 * depth, *box(depth, depth))
    _put_leaf(nodes, i + 2, 2 * depth + 1, *box(depth, depth))
    assert i + 3 == len(nodes)
    return nodes, tris


@functools.lru_cache(maxsize=None)
def bound_cases():
    """name -> (nodes, triangles): proper trees with an internal root around the two stack bounds the compile decides by (CPU tests only;
    tests/test_gpu_culling.py renders such trees)"""
    return {name: _comb(int(name.split()[1])) for name in BOUND_NAMES}


@functools.lru_cache(maxsize=None)
def refused():
    """name -> (nodes, triangles, fragment of the message) for what must be turned away (REFUSED_AT_SUBMIT: by the scene check of a
    submit, the uploads themselves pass).  The upload is stricter than the reference's walk: a backward link or a negative triangle
    index is refused in a node the root never reaches, too."""
    d = demo()
    base, tris = d.nodes, d.triangles
    n = len(base)
    leaves, internal = np.flatnonzero(base["isLeaf"] == 1), np.flatnonzero(base["isLeaf"] != 1)
    order = "BVH child index must be greater than its parent's and inside the buffer"
    negative = "leaf node with negative triangleIndex"
    out = {}
    nodes = base.copy()
    nodes["left"][0] = 0
    out["child equal to its parent"] = (nodes, tris, order)
    nodes = base.copy()
    nodes["right"][internal[40]] = 3
    out["child before its parent"] = (nodes, tris, order)
    nodes = base.copy()
    nodes["right"][internal[-1]] = n
    out["child beyond the buffer"] = (nodes, tris, order)
    nodes = _append(base, 1)
    _put_node(nodes, n, 0, -1, base["min"][0], base["max"][0])
    out["unreachable node with a backward link"] = (nodes, tris, order)
    nodes = base.copy()
    nodes["triangleIndex"][leaves[9]] = -2
    out["reachable leaf with a negative triangle"] = (nodes, tris, negative)
    nodes = _append(base, 1)
    _put_leaf(nodes, n, -1, base["min"][0], base["max"][0])
    out["unreachable leaf with a negative triangle"] = (nodes, tris, negative)
    nodes = base.copy()
    nodes["triangleIndex"][leaves[7]] = len(tris) + 5
    out["leaf beyond the triangles"] = (nodes, tris, "BVH references a triangle index beyond the triangle buffer")
    return out
