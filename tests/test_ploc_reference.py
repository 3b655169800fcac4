"""tests/ploc_reference.py on its own, without a device: the vectorised law against the scalar one, the tie rule, the forced pairing,
and what the law's trees are worth -- cost against the host SAH tree and the linear tree on the demo scene, the same image bits from the
oracle on all three, and the scene compile's verdict.  The figures asserted here follow from the law in include/mi3pt.h; none of them
is a measurement of the device code."""
import functools
import math

import numpy as np
import pytest

import lbvh_reference as lr
import ploc_reference as pr
import ptcommon as pc
from mi3pt_host import capi


@functools.lru_cache(maxsize=None)
def demo_tree(radius=16):
    from mi3pt_host import scenes
    return pr.build(scenes.demo_scene().triangles, radius)


@pytest.mark.parametrize("radius", [1, 2, 16])
def test_scalar_and_vectorised_agree(radius):
    for n in range(1, 41):
        tris = lr.pack(lr.random_triangles(n))
        nodes, searched, forced = pr.build(tris, radius)
        want, s, f = pr.build_scalar(tris, radius)
        assert (searched, forced) == (s, f), n
        diff = lr.first_word_difference(nodes, want)
        assert diff is None, f"n = {n}: {diff}"
        lr.check_tree(nodes, tris)
        assert not lr.padding_words(nodes).any() and forced == 0 and (searched >= 1) == (n > 1)


def test_one_and_two_triangles():
    tris = lr.pack(lr.random_triangles(1))
    nodes, searched, forced = pr.build(tris)
    assert (len(nodes), searched, forced) == (1, 0, 0)
    assert lr.first_word_difference(nodes, lr.reference_nodes(tris)) is None
    tris = lr.pack(lr.random_triangles(2))
    nodes, searched, forced = pr.build(tris)
    assert (len(nodes), searched, forced) == (3, 1, 0)
    assert lr.first_word_difference(nodes, lr.reference_nodes(tris)) is None            # two leaves in Morton order: the linear tree


@pytest.mark.parametrize("distinct,copies,iterations,levels", [(1, 4099, 13, 14), (5, 8000, 16, 17)])
def test_tie_rule_halves_runs_of_identical_boxes(distinct, copies, iterations, levels):
    """every distance in a run is the same: (b - a, a & 1) pairs (0,1), (2,3), ...; without it one pair merges per iteration -- 4 098
    iterations for the first"""
    tris = lr.pack(lr.repeated(distinct, copies))
    nodes, searched, forced = pr.build(tris)
    lr.check_tree(nodes, tris)
    assert (searched, forced, lr.depth(nodes)) == (iterations, 0, levels)


@pytest.mark.parametrize("radius,iterations,levels", [(1, 38, 39), (16, 9, 9)])
def test_chain(radius, iterations, levels):
    tris = lr.pack(lr.chain())
    nodes, searched, forced = pr.build(tris, radius)
    lr.check_tree(nodes, tris)
    assert (searched, forced, lr.depth(nodes)) == (iterations, 0, levels)
    want, s, f = pr.build_scalar(tris, radius)
    assert (s, f) == (searched, forced) and lr.first_word_difference(nodes, want) is None


@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 513])
def test_no_search_budget_gives_the_pairing_tree(n):
    tris = lr.pack(lr.random_triangles(n))
    nodes, searched, forced = pr.build(tris, 16, 0)
    lr.check_tree(nodes, tris)
    levels = math.ceil(math.log2(n)) + 1
    assert (searched, forced, lr.depth(nodes)) == (0, levels - 1, levels)
    assert lr.leaves_in_order(nodes) == pr.sorted_leaves(tris)[0].tolist()             # positions never cross


@pytest.mark.parametrize("budget", [1, 3])
def test_a_small_search_budget_is_used_up_first(budget):
    tris = lr.pack(lr.random_triangles(513))
    nodes, searched, forced = pr.build(tris, 16, budget)
    lr.check_tree(nodes, tris)
    assert searched == budget and forced >= 1
    small = lr.pack(lr.random_triangles(33))
    got, want = pr.build(small, 2, budget), pr.build_scalar(small, 2, budget)
    assert got[1:] == want[1:] and lr.first_word_difference(got[0], want[0]) is None


@pytest.mark.parametrize("name", ["grid", "plane", "line", "point", "extremes-xyz", "extremes-xy", "non-finite"])
def test_the_linear_builders_input_classes(name):
    pos = {"grid": lambda: lr.grid()[0], "plane": lambda: lr.degenerate("plane"), "line": lambda: lr.degenerate("line"),
           "point": lambda: lr.degenerate("point"), "extremes-xyz": lambda: lr.range_extremes(axes=3),
           "extremes-xy": lambda: lr.range_extremes(axes=2), "non-finite": lr.non_finite}[name]()
    tris = lr.pack(pos)
    nodes, searched, forced = pr.build(tris)
    lr.check_tree(nodes, tris, boxes=name != "non-finite")
    assert forced == 0 and 1 <= searched < len(tris)
    if len(tris) <= 100:                                                                 # +inf and NaN distances: ties go by position
        want, s, f = pr.build_scalar(tris)
        assert (s, f) == (searched, forced) and lr.first_difference(nodes, want, equal_nan=True) is None


def test_demo_scene_cost_against_both_other_trees(demo):
    """host_bvh_cost: 6.381 for this tree, 7.08 for the SAH tree, 11.005 for the linear tree"""
    nodes, searched, forced = demo_tree()
    lr.check_tree(nodes, demo.triangles)
    cost, sah, linear = (capi.host_bvh_cost(t) for t in (nodes, demo.nodes, lr.reference_nodes(demo.triangles)))
    print(f"host_bvh_cost: clustering {cost:.3f}, SAH {sah:.3f}, linear {linear:.3f}; {searched} search iterations, depth {lr.depth(nodes)}")
    assert (searched, forced, lr.depth(nodes)) == (37, 0, 21)
    assert abs(cost - 6.381) < 0.0005 and abs(linear - 11.005) < 0.0005
    assert cost < sah and cost < 0.6 * linear


def test_demo_scene_renders_the_same_bits_on_all_three_trees(orc, demo, env):
    w, h = 48, 32
    u = pc.rt_uniforms(demo, w, h, frame=2, bounces=4).tobytes()
    images = [orc.raytrace(orc.OracleScene(demo.triangles, demo.material_bytes, t, env), u, w, h)
              for t in (demo.nodes, lr.reference_nodes(demo.triangles), demo_tree()[0])]
    (sah, sah_cnt), (linear, linear_cnt), (ploc, ploc_cnt) = images
    assert pc.same_bits(ploc, sah), pc.describe_diff(ploc, sah)
    assert pc.same_bits(linear, sah), pc.describe_diff(linear, sah)
    for k in ("rays", "hits", "misses"):
        assert ploc_cnt[k] == sah_cnt[k] == linear_cnt[k]
    assert ploc_cnt["box_tests"] < sah_cnt["box_tests"] < linear_cnt["box_tests"]


def test_the_scene_compile_takes_the_tree_like_the_sah_tree(demo):
    got = capi.host_scene_compile(demo_tree()[0], demo.triangles)
    want = capi.host_scene_compile(demo.nodes, demo.triangles)
    assert got["tree_proper"] == 1 and got["cull_stack_ok"] == 1
    assert (want["tree_proper"], want["cull_stack_ok"]) == (1, 1)


def test_the_header_states_the_law_and_the_hosts_share_the_block_size(built):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)                              # a function added, nothing changed
    assert int(re.search(r"#define MI3PT_PLOC_SEARCH_BLOCK (\d+)\b", hdr).group(1)) == capi.PLOC_SEARCH_BLOCK
    assert capi.BVH_METHODS == {"lbvh": int(re.search(r"#define MI3PT_BVH_METHOD_LBVH (\d+)", hdr).group(1)),
                                "ploc": int(re.search(r"#define MI3PT_BVH_METHOD_PLOC (\d+)", hdr).group(1))}
    for phrase in ("K(a, b) = (d, b - a, a & 1, a)", "a = (e.x * e.y + e.y * e.z) + e.z * e.x", "nn(i) = i ^ 1"):
        assert phrase in hdr, phrase
    assert "mi3pt_device_build_bvh_ex" in capi.SYMBOLS
    import ctypes
    assert ctypes.sizeof(capi.BvhBuildParams) == 16 and ctypes.sizeof(capi.BvhBuildInfoStruct) == 12
    lib = capi.load_library()
    p = capi.BvhBuildParams(1, 16, 1024, 0)
    n = ctypes.c_size_t(7)
    assert lib.mi3pt_device_build_bvh_ex(None, ctypes.byref(p), None, 0, ctypes.byref(n), None) == 1 and n.value == 7      # a null context
