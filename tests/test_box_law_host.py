"""The host SAH builder (mi3pt_host_build_bvh_f64, csrc/pt_host_scene.cpp) held to the refit's law on the inputs of
tests/box_law_cases.py, without a device: what the builder writes is a fixed point of the law, word for word -- which is the promise
"re-fitting an unchanged scene returns the uploaded bytes" (include/mi3pt.h) seen from the builder's side -- the reference's own builder,
executed under Node, writes the same words, and the two restatements of the law agree on every new case and every shaped tree.
Every comparison is of 32-bit words; nothing here has a tolerance."""
import importlib.util
import os

import numpy as np
import pytest

import box_law_cases as blc
import refit_reference as rr
from mi3pt_host import capi, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PZ, NZ = blc.PZ, blc.NZ
CARRIED = [3, 7, 8, 9, 10, 11]


def _generator():
    spec = importlib.util.spec_from_file_location("make_host_vectors", os.path.join(ROOT, "tests", "golden", "make_host_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pack(pos):
    n = len(pos)
    return layout.pack_triangles(pos, np.tile([0.0, 0.0, 1.0], (n, 3, 1)), np.zeros(n, int))


def _fixed_point_sets():
    sets = {"zeros": blc.zeros().positions, "subnormals": blc.subnormals().positions}
    for name, pos in _generator().triangle_sets().items():
        sets.setdefault(name, pos)
    return sets


FIXED_POINT_NAMES = ("zeros", "subnormals", "demo", "soup", "grid", "tall", "pair", "single", "triple")


def _words(nodes):
    return np.ascontiguousarray(nodes).view(np.uint8).reshape(-1).view("<u4").reshape(-1, 12)


@pytest.mark.parametrize("name", FIXED_POINT_NAMES)
def test_the_built_tree_is_a_fixed_point_of_the_law(built, name):
    """host build -> the law on the same vertices -> the same words.  Before the builder formed its boxes with the law's lo / hi it
    kept the FIRST of two equal operands (std::min / std::max): on `zeros` a leaf of x = (+0, -0, +0) had min.x 0x00000000 where the
    law, and Math.min, say 0x80000000."""
    sets = _fixed_point_sets()
    assert set(FIXED_POINT_NAMES) == set(sets)
    pos = np.ascontiguousarray(sets[name], np.float64)
    for threads in (1, 4):
        nodes = capi.host_build_bvh_f64(pos, threads)
        assert len(nodes) == 2 * len(pos) - 1
        want = rr.refit_scalar(nodes, _pack(pos))
        diff = rr.first_difference(nodes, want)
        assert diff is None, f"{name}, {threads} thread(s): {diff}"
    # the fp32 entry point gives the same tree from the packed records (these positions are fp32 values)
    if name in ("zeros", "subnormals"):
        assert capi.host_build_bvh(_pack(pos)).tobytes() == nodes.tobytes()


def test_zeros_meet_the_builder_where_it_forms_boxes(built):
    """what the `zeros` set is arranged for, read off the built tree: leaf boxes with either zero as a bound; the two-input case
    (both children leaves, as given) with a +0 leaf on the left of a -0 leaf and the other way round; unions of a leaf and a subtree
    -- what a sweep's prefix and suffix boxes hold -- in both orders too.  Both zero words among the internal minima and maxima."""
    z = blc.zeros()
    nodes = capi.host_build_bvh_f64(z.positions)
    leaf = nodes["isLeaf"] == 1
    inner = np.flatnonzero(~leaf)
    l, r = nodes["left"][inner], nodes["right"][inner]
    for k in range(3):
        mn, mx = nodes["min"][:, k].view("<u4"), nodes["max"][:, k].view("<u4")
        for w in (mn, mx):
            assert {PZ, NZ} <= set(w[leaf].tolist()) and {PZ, NZ} <= set(w[inner].tolist()), k
        two = leaf[l] & leaf[r]
        deep = ~two
        for sel in (two, deep):
            assert ((mn[l] == PZ) & (mn[r] == NZ) & sel).any() and ((mn[l] == NZ) & (mn[r] == PZ) & sel).any(), k
            assert ((mx[l] == PZ) & (mx[r] == NZ) & sel).any() and ((mx[l] == NZ) & (mx[r] == PZ) & sel).any(), k
        # a union of unlike zeros is [-0, +0] whichever side they came from
        mixed = ((mn[l] == PZ) & (mn[r] == NZ)) | ((mn[l] == NZ) & (mn[r] == PZ))
        assert (mn[inner][mixed] == NZ).all()
        mixed = ((mx[l] == PZ) & (mx[r] == NZ)) | ((mx[l] == NZ) & (mx[r] == PZ))
        assert (mx[inner][mixed] == PZ).all()


def test_topology_does_not_depend_on_the_signs_of_zeros(built):
    """words 7 - 10 (isLeaf, left, right, triangleIndex) of the tree built from `zeros` and from the same positions with every -0
    made +0 (x + 0.0: the absolute value of the ZEROS -- of every coordinate it would be another scene, the set has negative
    coordinates): the sort keys, the axis rule and the sweep's areas see values, and +0 == -0"""
    z = blc.zeros()
    unsigned = z.positions + 0.0
    assert (unsigned == z.positions).all() and not np.signbit(unsigned[unsigned == 0]).any()
    assert np.signbit(z.positions[z.positions == 0]).sum() == 3 * 50          # per component: 8 + 12 + 30 of its 100 zeros are -0
    for threads in (1, 4):
        a, b = _words(capi.host_build_bvh_f64(z.positions, threads)), _words(capi.host_build_bvh_f64(unsigned, threads))
        assert (a[:, 7:11] == b[:, 7:11]).all()
        assert (a[:, [3, 11]] == 0).all()
        assert (a[:, :7] != b[:, :7]).any()                   # (the boxes do differ: -0 bounds against +0 bounds)


def test_the_reference_builder_writes_the_laws_words_on_zeros(built):
    """tests/golden/host_vectors.npz, `zeros`: the reference's buildBVH run under Node over three's Vector3 / Box3 (Math.min /
    Math.max).  Its records are a fixed point of the law, they hold zeros of both signs as bounds, and the native builder writes the
    same bytes (tests/test_reference_host_vectors.py compares every set; this ties the three together on this one)."""
    z = blc.zeros()
    vec = np.load(os.path.join(ROOT, "tests", "golden", "host_vectors.npz"))
    ref = np.frombuffer(vec["bvh_zeros_nodes"].tobytes(), layout.BVH_NODE)
    assert len(ref) == 2 * len(z) - 1
    for fn in (rr.refit_scalar, rr.refit_vectorised):
        diff = rr.first_difference(fn(ref, z.triangles()), ref)
        assert diff is None, diff
    for k in range(3):
        assert {PZ, NZ} <= set(ref["min"][:, k].view("<u4").tolist()) and {PZ, NZ} <= set(ref["max"][:, k].view("<u4").tolist())
    got = capi.host_build_bvh_f64(z.positions)
    assert got.tobytes() == ref.tobytes(), rr.first_difference(got, ref)


def _shaped_trees(case):
    """name -> (nodes, triangles): the host-built tree, its mirror image, the two chains over the first 63 triangles, each also with
    stamped padding words"""
    built_nodes = capi.host_build_bvh_f64(case.build_positions)
    tris, first = case.triangles(), case.triangles(63)
    out = {"built": (built_nodes, tris), "mirrored": (blc.mirrored(built_nodes), tris),
           "chain_right": (blc.chain_right(62), first), "zigzag": (blc.zigzag(62), first),
           "mirrored zigzag": (blc.mirrored(blc.zigzag(62)), first)}
    for seed, name in enumerate(list(out)):
        out[name + ", stamped"] = (blc.stamped(out[name][0], 100 + seed), out[name][1])
    return out


@pytest.mark.parametrize("name", ("zeros", "subnormals", "non_finite"))
def test_law_restatements_agree_and_carry(built, name):
    """refit_scalar == refit_vectorised, word for word, NaN payloads included; words 3 and 7 - 11 are the uploaded record's"""
    case = blc.all_cases()[name]
    for shape, (nodes, tris) in _shaped_trees(case).items():
        assert capi.host_scene_compile(nodes, tris)["tree_proper"], shape
        a, b = rr.refit_scalar(nodes, tris), rr.refit_vectorised(nodes, tris)
        diff = rr.first_difference(a, b)
        assert diff is None, f"{name}, {shape}: {diff}"
        w0, w1 = _words(nodes), _words(a)
        assert (w0[:, CARRIED] == w1[:, CARRIED]).all(), shape
        if "stamped" in shape:
            assert (w1[:, 3] != 0).any() and (w1[:, 11] != 0).any()
        # the law only selects: every bound of a leaf is one of its triangle's words, every bound of a parent one of its children's
        leaf = a["isLeaf"] == 1
        t = case.words[a["triangleIndex"][leaf]]
        for f, cols in (("min", slice(0, 3)), ("max", slice(4, 7))):
            assert (w1[leaf, cols][:, None, :] == t).any(1).all(), (shape, f)
            l, r = a["left"][~leaf], a["right"][~leaf]
            assert ((w1[~leaf, cols] == w1[l, cols]) | (w1[~leaf, cols] == w1[r, cols])).all(), (shape, f)


def test_python_host_refits_the_unchanged_zeros_scene_to_itself(monkeypatch, built):
    """RaytracePass.updateScene under `refit = true` (tests/test_refit_host.py's stand-in context, whose device_refit_bvh answers with
    the law's records): the `zeros` scene submitted again, unchanged.  The re-fitted records are the built ones, so the cost ratio is
    1.0 exactly and the host's copy of the tree keeps its bytes."""
    import test_refit_host as trf
    import test_reproject_host as trh
    from mi3pt_host import scenes
    z = blc.zeros()
    r, scene, cam, _, _ = trh._renderer(monkeypatch, trf.RefitContext)
    n = len(z)
    scene.content = scenes.Scene(z.positions, np.tile([0.0, 0.0, 1.0], (n, 3, 1)), np.zeros(n, int), [scenes.WHITE])
    r.refit = True
    r.frames = 3
    for _ in range(3):
        r.render(scene, cam)
    first = np.ascontiguousarray(scene.content.nodes).tobytes()
    assert first == capi.host_build_bvh_f64(z.positions).tobytes() and r.lastRefitCostRatio is None
    before = len(r.ctx.calls)
    scene.needsUpdate = True
    r.update(scene, cam)
    assert trf._names(r.ctx.calls[before:]) == ["upload_triangles", "device_refit_bvh", "upload_bvh", "upload_materials"]
    assert r.lastRefitCostRatio == 1.0
    assert np.ascontiguousarray(scene.content.nodes).tobytes() == first
    sent = [c[1] for c in r.ctx.calls[before:] if c[0] == "upload_bvh"][0]
    assert np.ascontiguousarray(sent).tobytes() == first


def test_shapers_give_what_they_say(built):
    z = blc.zeros()
    nodes = capi.host_build_bvh_f64(z.positions)
    m = blc.mirrored(nodes)
    inner = nodes["isLeaf"] != 1
    assert (m["left"][inner] == nodes["right"][inner]).all() and (m["right"][inner] == nodes["left"][inner]).all()
    assert (m["left"][inner] > m["right"][inner]).any() and (m["left"][inner] > np.flatnonzero(inner)).all()
    assert blc.mirrored(m).tobytes() == np.ascontiguousarray(nodes).tobytes()
    for shape in (blc.chain_right(62), blc.zigzag(62)):
        assert len(shape) == 125 and (shape["isLeaf"] != 1).sum() == 62
        assert sorted(shape["triangleIndex"][shape["isLeaf"] == 1].tolist()) == list(range(63))
        assert rr.levels(shape).max() == 62
    cr, zz, ch = blc.chain_right(62), blc.zigzag(62), rr.chain(62)[0]
    leaf_right = lambda t: [bool(t["isLeaf"][t["right"][i]] == 1) for i in np.flatnonzero(t["isLeaf"] != 1)]
    leaf_left = lambda t: [bool(t["isLeaf"][t["left"][i]] == 1) for i in np.flatnonzero(t["isLeaf"] != 1)]
    assert all(leaf_right(cr)) and leaf_left(cr) == [False] * 61 + [True]
    assert all(leaf_left(ch)) and leaf_left(zz)[:4] == [True, False, True, False]
    for t in (cr, zz):
        i = np.flatnonzero(t["isLeaf"] != 1)
        assert (t["left"][i] > t["right"][i]).any()
    # an all-NaN leaf on the left of one union and on the right of another, in the host-built tree and in its mirror image
    nf = blc.non_finite()
    tree = capi.host_build_bvh_f64(nf.build_positions)
    nan_tris = set(blc.all_nan_leaves(nf).tolist())
    for t in (tree, blc.mirrored(tree)):
        i = np.flatnonzero(t["isLeaf"] != 1)
        is_nan_leaf = np.array([t["isLeaf"][j] == 1 and int(t["triangleIndex"][j]) in nan_tris for j in range(len(t))])
        assert is_nan_leaf[t["left"][i]].any() and is_nan_leaf[t["right"][i]].any()
