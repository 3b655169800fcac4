"""tests/irregular_trees.py on the CPU: every case satisfies the upload's preconditions, compiles, IS what its name says, and can be
told from the builder's tree of the same triangles by the oracle (image bits, box tests or triangle tests) -- so that a walk which
ignored the irregularity would be caught on the device (tests/test_gpu_irregular_trees.py).  And the compile's decisions against a
plain restatement of what they mean (the digests of tests/test_scene_compile.py say that a decision has not changed, not that it is
right): tree_proper, leaf_cap > 0, cull_stack_ok from a small recursive walk of the records; cwide_ok / cw8_ok off wherever a
reachable box is not finite or does not contain its children's.  No GPU."""
import numpy as np
import pytest

import irregular_trees as it
import ptcommon as pc
from mi3pt_host import capi, layout

# csrc/pt_kernels.h: the LDS slots of a lane's stack, and the culling walks' bound (64 - SM_CULL_LEAF_CAP)
SM_LDS_DEPTH = 24
SM_CULL_STACK_MAX = 56
W = H = 48

CASES = sorted(it.CASE_NAMES)
REFUSED = sorted(it.REFUSED_NAMES)


def _is_leaf(nodes, i):
    return int(nodes["isLeaf"][i]) == 1


def reference_walk(nodes):
    """The reference's walk with every box hit (raytrace.wgsl:160-200: pop; a leaf is tested; otherwise push left, then right, each
    if >= 0).  Returns (visits per node, owners per triangle, a reached internal node lacks a child, the largest number of entries
    on the stack, the largest number of INTERNAL entries on it)."""
    n = len(nodes)
    visits = np.zeros(n, int)
    owners = {}
    missing = False
    stack = [0]
    worst = worst_internal = 0
    while stack:
        worst = max(worst, len(stack))
        worst_internal = max(worst_internal, sum(not _is_leaf(nodes, i) for i in stack))
        i = stack.pop()
        visits[i] += 1
        if _is_leaf(nodes, i):
            t = int(nodes["triangleIndex"][i])
            owners[t] = owners.get(t, 0) + 1
            continue
        for side in ("left", "right"):
            c = int(nodes[side][i])
            if c < 0:
                missing = True
            else:
                stack.append(c)
    return visits, owners, missing, worst, worst_internal


def any_order_bound(nodes, node=0, occupancy=1):
    """The largest number of internal entries a near-first walk can stack whatever child it descends first: a child is on top with
    all its internal siblings still below it (proper trees only)."""
    kids = [int(nodes[s][node]) for s in ("left", "right")]
    kids = [c for c in kids if not _is_leaf(nodes, c)]
    worst = occupancy
    for c in kids:
        worst = max(worst, any_order_bound(nodes, c, occupancy - 1 + len(kids)))
    return worst


def restated(nodes):
    visits, owners, missing, worst, worst_internal = reference_walk(nodes)
    proper = bool((visits <= 1).all() and all(v == 1 for v in owners.values()) and not missing and worst < 64)
    defer = proper and worst_internal <= SM_LDS_DEPTH - 4
    cull = proper and not _is_leaf(nodes, 0) and any_order_bound(nodes) <= SM_CULL_STACK_MAX
    return dict(tree_proper=proper, defer=defer, cull_stack_ok=cull, reached=visits > 0, visits=visits, owners=owners, missing=missing)


def boxes_admit_compression(nodes, reached):
    """every reachable box finite, every reachable internal box around its children's"""
    for i in np.flatnonzero(reached):
        mn, mx = nodes["min"][i], nodes["max"][i]
        if not (np.isfinite(mn).all() and np.isfinite(mx).all()):
            return False
        if _is_leaf(nodes, i):
            continue
        for side in ("left", "right"):
            c = int(nodes[side][i])
            if c >= 0 and not ((mn <= nodes["min"][c]).all() and (mx >= nodes["max"][c]).all()):
                return False
    return True


@pytest.fixture(scope="module")
def compiled(built):
    return {name: capi.host_scene_compile(nodes, tris, want_eight_wide=True) for name, (nodes, tris, _, _) in it.cases().items()}


@pytest.fixture(scope="module")
def oracle_runs(orc, env):
    """name -> (the oracle on the case's tree, the oracle on the builder's tree of the same triangles): (image, counters) each"""
    out = {}
    for name, (nodes, tris, mats, cam) in it.cases().items():
        u = it.uniforms(cam, W, H).tobytes()
        pos = np.stack([tris["aPosition"], tris["bPosition"], tris["cPosition"]], 1).astype(np.float64)
        # (the demo scene's tree is built from its float64 vertices: the builder's tree of the demo cases is that one)
        built_tree = it.demo().nodes if tris is it.demo().triangles else capi.host_build_bvh_f64(pos)
        out[name] = (orc.raytrace(orc.OracleScene(tris, mats, nodes, env), u, W, H),
                     orc.raytrace(orc.OracleScene(tris, mats, built_tree, env), u, W, H))
    return out


def test_the_names_are_the_cases(built):
    assert set(it.cases()) == set(it.CASE_NAMES) and len(set(it.CASE_NAMES)) == len(it.CASE_NAMES)
    assert set(it.refused()) == set(it.REFUSED_NAMES) and set(it.bound_cases()) == set(it.BOUND_NAMES)
    assert set(it.UNREACHABLE + it.BUILDER_MADE) <= set(it.CASE_NAMES) and set(it.REFUSED_AT_SUBMIT) <= set(it.REFUSED_NAMES)


@pytest.mark.parametrize("name", CASES)
def test_case_meets_the_uploads_preconditions_and_is_what_it_says(built, name):
    nodes, tris, mats, _ = it.cases()[name]
    assert it.precondition_violations(nodes, tris, len(mats)) == []
    assert nodes.dtype == layout.BVH_NODE and nodes.strides == (48,) and tris.dtype.itemsize == 112
    r = restated(nodes)
    base = it.demo().nodes
    leaf = nodes["isLeaf"] == 1
    box_ok = np.isfinite(nodes["min"]).all(1) & np.isfinite(nodes["max"]).all(1) & (nodes["min"] < nodes["max"]).any(1) & (nodes["min"] <= nodes["max"]).all(1)
    if name == "missing children":
        assert r["missing"] and (~r["reached"]).sum() > 300
    elif name in ("shared subtrees", "shared coincident sheets"):
        assert (r["visits"] > 1).any() and not r["missing"]
        assert max(r["owners"].values()) > 1              # the shared subtree's triangles are tested on every visit
    elif name.startswith("doubly owned"):
        assert (r["visits"] <= 1).all() and sum(v == 2 for v in r["owners"].values()) >= 90
    elif name == "isLeaf other than 0 and 1":
        assert set(np.unique(nodes["isLeaf"])) == {-1, 0, 1, 2, 3} and r["missing"]
    elif name in it.UNREACHABLE:
        assert r["reached"][:len(base)].all() and not r["reached"][len(base):].any() and r["tree_proper"]
        assert nodes[:len(base)].tobytes() == base.tobytes()
        assert leaf[len(base):].all() == (name == "unreachable leaves")
    elif name.startswith("bad boxes"):
        bad = ~box_ok
        assert bad.sum() == 120 and not bad[0] and r["tree_proper"]
        assert np.isnan(nodes["min"][bad]).any() and np.isinf(nodes["max"][bad]).any()
        if name != "bad boxes":
            assert (leaf[bad]).all() == (name == "bad boxes on leaves") and (leaf[bad]).any() == (name == "bad boxes on leaves")
    elif name == "leaf root":
        assert len(nodes) == 1 and leaf[0]
    else:
        assert name in it.BUILDER_MADE and not leaf[0] and r["tree_proper"]


@pytest.mark.parametrize("name", CASES)
def test_the_compiles_decisions_against_their_restatement(compiled, name):
    nodes, tris, mats, _ = it.cases()[name]
    got, want = compiled[name], restated(nodes)
    assert bool(got["tree_proper"]) == want["tree_proper"]
    assert (got["leaf_cap"] > 0) == want["defer"]
    assert bool(got["cull_stack_ok"]) == want["cull_stack_ok"]
    assert got["max_tri_ref"] < len(tris) and got["max_mat_ref"] < len(mats)
    if not want["cull_stack_ok"]:
        assert not (got["analysed"] or got["wide_ok"] or got["cwide_ok"] or got["cw8_ok"])       # no culling walk without its stack bound
    if not boxes_admit_compression(nodes, want["reached"]):
        assert not got["cwide_ok"] and not got["cw8_ok"]
    if name in it.UNREACHABLE + it.BUILDER_MADE:
        # the builder's tree, reachable node for reachable node: what it is offered, these are offered
        assert got["wide_ok"] and got["cwide_ok"] and got["cw8_ok"]


@pytest.mark.parametrize("name", CASES)
def test_the_compressed_walks_records_carry_the_reachable_leaf_boxes(compiled, name):
    """Variant 13 runs the leaf's exact box test from the 64-byte record of the leaf's triangle (csrc/pt_kernels.h: TriPacket64 -- a,
    e1, e2, the leaf's box, a flag).  The box must be the box of the leaf the ROOT REACHES, bit for bit, whatever other node of the
    buffer names the same triangle; a triangle without a reachable leaf keeps an inert record (an empty box)."""
    nodes, tris, _, _ = it.cases()[name]
    rec = capi.host_walk_buffer(nodes, tris, capi.WALK_TRI64)
    if not compiled[name]["cwide_ok"]:
        assert len(rec) == 0
        return
    assert len(rec) == len(tris)
    words = rec.view(np.uint32).reshape(len(tris), 16)
    reached = restated(nodes)["reached"]
    owned = np.zeros(len(tris), bool)
    for i in np.flatnonzero(reached & (nodes["isLeaf"] == 1)):
        t = int(nodes["triangleIndex"][i])
        owned[t] = True
        want = np.concatenate([nodes["min"][i], nodes["max"][i]]).view(np.uint32)
        assert (words[t, 9:15] == want).all(), f"triangle {t}: the record's box is not the box of its leaf, node {i}"
        assert (words[t, 0:3] == tris["aPosition"][t].view(np.uint32)).all()
    boxes = words[~owned, 9:15].view(np.float32)
    assert (boxes[:, 0:3] > boxes[:, 3:6]).all()


def test_the_two_stack_bounds_on_proper_trees_with_an_internal_root(built):
    """tree_proper alone does not decide leaf_cap > 0 and cull_stack_ok: comb trees one level below and one above each bound (a wrong
    constant in the restatement, or in the compile, shows here and nowhere among the cases)"""
    seen = set()
    for name, (nodes, tris) in it.bound_cases().items():
        assert it.precondition_violations(nodes, tris, 1) == []
        got, want = capi.host_scene_compile(nodes, tris), restated(nodes)
        assert want["tree_proper"] and got["tree_proper"] and not _is_leaf(nodes, 0)
        assert (got["leaf_cap"] > 0) == want["defer"], name
        assert bool(got["cull_stack_ok"]) == want["cull_stack_ok"], name
        seen.add((want["defer"], want["cull_stack_ok"]))
    assert seen == {(True, True), (False, True), (False, False)}, seen


def test_the_cases_reach_both_sides_of_every_decision(compiled):
    seen = {k: set() for k in ("tree_proper", "cull_stack_ok", "wide_ok", "cwide_ok", "cw8_ok")}
    for got in compiled.values():
        for k in seen:
            seen[k].add(got[k])
    for k in seen:
        assert seen[k] == {0, 1}, (k, seen[k])
    assert {c["leaf_cap"] > 0 for c in compiled.values()} == {False, True}
    # a proper tree that is refused the compressed packets but keeps the exact wide ones (what `auto` then runs: variant 10)
    assert any(c["wide_ok"] and not c["cwide_ok"] for c in compiled.values())


@pytest.mark.parametrize("name", CASES)
def test_each_case_can_fail(oracle_runs, name):
    """The oracle on the case's tree against the oracle on the builder's tree of the same triangles: different image bits, box tests or
    triangle tests -- a walk that treated the tree as a builder's would be seen.  Unreachable nodes must change nothing at all, and the
    builder's own small trees are the builder's."""
    (img, cnt), (bimg, bcnt) = oracle_runs[name]
    texels = int((~((img == bimg) | (np.isnan(img) & np.isnan(bimg)))).any(-1).sum())
    print(f"{name}: {texels} texels differ, box tests {cnt['box_tests']} vs {bcnt['box_tests']}, triangle tests {cnt['tri_tests']} vs {bcnt['tri_tests']}")
    assert cnt["stack_overflows"] == 0
    if name in it.UNREACHABLE + it.BUILDER_MADE:
        assert texels == 0 and cnt == bcnt
    else:
        assert texels > 0 or cnt["box_tests"] != bcnt["box_tests"] or cnt["tri_tests"] != bcnt["tri_tests"]
    if name in ("doubly owned triangles", "shared coincident sheets"):
        assert texels > 0          # a lost triangle / the tie's winner shows in the image itself


@pytest.mark.parametrize("name", CASES)
def test_the_view_has_sky_and_geometry(orc, env, name):
    """at least a tenth of the camera rays hit, and whole 8 x 8 tiles see nothing but sky (what the sky-tile path skips)"""
    nodes, tris, mats, cam = it.cases()[name]
    u = it.uniforms(cam, W, H, bounces=1).tobytes()
    _, cnt = orc.raytrace(orc.OracleScene(tris, mats, nodes, env), u, W, H)
    assert cnt["rays"] == W * H
    assert cnt["hits"] >= W * H // 10, cnt
    sc = orc.OracleScene(tris, mats, nodes, env)
    sky_tiles = 0
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            corners = [orc.camera_ray(u, (x + 0.5) / W, (y + 0.5) / H) for y in (ty, ty + 7) for x in (tx, tx + 7)]
            sky_tiles += all(orc.ray_scene(sc, r[:3], r[3:])[0][0] == 0.0 for r in corners)
    assert sky_tiles >= 4, sky_tiles


@pytest.mark.parametrize("name", REFUSED)
def test_refused_trees_break_one_precondition_and_the_compile_says_which(built, name):
    nodes, tris, message = it.refused()[name]
    assert len(it.precondition_violations(nodes, tris, 2)) == 1          # (the oracle is never run on these)
    if name in it.REFUSED_AT_SUBMIT:
        got = capi.host_scene_compile(nodes, tris)                       # the upload passes; the scene check of a submit refuses
        assert got["max_tri_ref"] >= len(tris) and not got["analysed"]
    else:
        with pytest.raises(capi.Mi3ptError) as e:
            capi.host_scene_compile(nodes, tris)
        assert e.value.code == 1 and message in e.value.message          # MI3PT_ERR_INVALID
