"""mi3pt_device_build_bvh_ex, method 1 (csrc/pt_ploc.hip) on the device: every tree word for word against the law in
tests/ploc_reference.py (lbvh_reference.first_word_difference; the NaN input as values), the iteration counts included.
Shapes: the smallest inputs; both sides of every edge of the neighbour search's block (B = capi.PLOC_SEARCH_BLOCK positions plus a halo
of `radius` on each side) at the smallest, a small, the default and the largest radius, and a radius beyond the input; runs of identical
boxes across blocks (the tie rule); the linear builder's other input classes; the forced pairing; many blocks, built three times (the
temporary ids come from an atomic counter and must not show); method 0; a render against the oracle on the same tree; and that the call
moves nothing of the context."""
import ctypes
import functools

import numpy as np
import pytest

import lbvh_reference as lr
import ploc_reference as pr
import ptcommon as pc
from mi3pt_host import capi, layout

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4          # include/mi3pt.h
B = capi.PLOC_SEARCH_BLOCK


@pytest.fixture(scope="module")
def ctx(built):
    with capi.Context(0) as c:
        yield c


def _check(ctx, tris, radius=16, budget=1024, equal_nan=False):
    """build on the device; the records and both counts are the law's"""
    want, searched, forced = pr.build(tris, radius, budget)
    ctx.upload_triangles(tris)
    nodes, info = ctx.device_build_bvh("ploc", radius, budget)
    what = f"n = {len(tris)}, radius {radius}, budget {budget}"
    diff = lr.first_difference(nodes, want, equal_nan=True) if equal_nan else lr.first_word_difference(nodes, want)
    assert diff is None, f"{what}: {diff}"
    assert (info.search_iterations, info.forced_iterations) == (searched, forced), what
    assert info.build_ms > 0 and float(info) == info.build_ms
    return nodes


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_small_inputs(ctx, n):
    tris = lr.pack(lr.random_triangles(n))
    lr.check_tree(_check(ctx, tris), tris)


@pytest.mark.parametrize("radius", [1, 2, 16, 64])
def test_block_and_halo_edges(ctx, radius):
    r = radius
    sizes = [B - r - 1, B - r, B - 1, B, B + 1, B + r, B + r + 1, 2 * B - 1, 2 * B, 2 * B + 1]
    assert len(set(sizes)) >= 8
    for n in sizes:
        _check(ctx, lr.pack(lr.random_triangles(n)), radius)


@pytest.mark.parametrize("n,radius", [(2, 64), (17, 16), (17, 17), (40, 64), (64, 64), (65, 64)])
def test_a_radius_that_reaches_past_the_input(ctx, n, radius):
    _check(ctx, lr.pack(lr.random_triangles(n)), radius)


@pytest.mark.parametrize("distinct,copies,iterations", [(1, 4099, 13), (5, 8000, 16)])
def test_ties_across_blocks(ctx, distinct, copies, iterations):
    tris = lr.pack(lr.repeated(distinct, copies))
    nodes = _check(ctx, tris)
    assert lr.depth(nodes) == iterations + 1


@pytest.mark.parametrize("name", ["grid", "chain", "chain-radius-1", "plane", "line", "point", "extremes-xyz", "extremes-xy"])
def test_the_linear_builders_input_classes(ctx, name):
    pos = {"grid": lambda: lr.grid()[0], "chain": lr.chain, "chain-radius-1": lr.chain, "plane": lambda: lr.degenerate("plane"),
           "line": lambda: lr.degenerate("line"), "point": lambda: lr.degenerate("point"),
           "extremes-xyz": lambda: lr.range_extremes(axes=3), "extremes-xy": lambda: lr.range_extremes(axes=2)}[name]()
    tris = lr.pack(pos)
    lr.check_tree(_check(ctx, tris, radius=1 if name.endswith("radius-1") else 16), tris)


def test_non_finite_vertices(ctx):
    """an all-NaN box has the distance +inf to everything: its ties go by position, nothing hangs or faults"""
    tris = lr.pack(lr.non_finite())
    nodes = _check(ctx, tris, equal_nan=True)
    lr.check_tree(nodes, tris, boxes=False)
    nan_leaf = int(np.flatnonzero(nodes["triangleIndex"] == 65)[0])
    assert np.isnan(nodes["min"][nan_leaf]).all() and np.isnan(nodes["max"][nan_leaf]).all()
    assert not np.isnan(nodes["min"][0]).any() and not np.isnan(nodes["max"][0]).any()


@pytest.mark.parametrize("budget", [0, 1, 3])
def test_forced_pairing_after_the_search_budget(ctx, budget):
    tris = lr.pack(lr.random_triangles(513))
    nodes = _check(ctx, tris, budget=budget)
    lr.check_tree(nodes, tris)
    if budget == 0:
        assert lr.depth(nodes) == 11                          # ceil(log2 513) + 1


@functools.lru_cache(maxsize=None)
def _many():
    tris = lr.pack(lr.random_triangles(40000))
    return tris, pr.build(tris)


def test_many_blocks_and_the_atomics_do_not_show(ctx):
    tris, (want, searched, forced) = _many()
    first = _check(ctx, tris)
    second, _ = ctx.device_build_bvh("ploc")
    with capi.Context(0) as fresh:
        fresh.upload_triangles(tris)
        third, info = fresh.device_build_bvh("ploc")
    assert first.tobytes() == second.tobytes() == third.tobytes() == np.ascontiguousarray(want).tobytes()
    assert (info.search_iterations, info.forced_iterations) == (searched, forced)


def _ex_raw(lib, handle, params, buf, capacity, count=True, info=True):
    n, got = ctypes.c_size_t(12345), capi.BvhBuildInfoStruct(-1.0, 77, 77)
    rc = lib.mi3pt_device_build_bvh_ex(handle, ctypes.byref(params) if params is not None else None,
                                       buf.ctypes.data_as(ctypes.c_void_p) if buf is not None else None, capacity,
                                       ctypes.byref(n) if count else None, ctypes.byref(got) if info else None)
    return rc, n.value, got, lib.mi3pt_last_error().decode()


def test_method_0_is_the_linear_builder(ctx, demo):
    for tris in (demo.triangles, lr.pack(lr.random_triangles(513))):
        ctx.upload_triangles(tris)
        want, _ = ctx.device_build_bvh()
        buf = np.zeros(len(want) * 48, np.uint8)
        # (method 0 reads neither parameter)
        rc, n, info, msg = _ex_raw(ctx.lib, ctx.handle, capi.BvhBuildParams(0, 0, -1, 0), buf, buf.nbytes)
        assert rc == 0 and n == len(want), msg
        assert buf.tobytes() == np.ascontiguousarray(want).tobytes()
        assert info.build_ms > 0 and (info.search_iterations, info.forced_iterations) == (0, 0)
        named, info = ctx.device_build_bvh("lbvh")
        assert named.tobytes() == np.ascontiguousarray(want).tobytes() and info > 0


@pytest.mark.parametrize("variant", [0, 7], ids=["shipped-walk", "reference-counter-walk"])
def test_demo_scene_renders_like_the_oracle_on_this_tree(ctx, orc, demo, env, variant):
    """frames 2 - 4 at 64 x 64, 4 bounces: the accumulation image, bit for bit.  Against the oracle on THIS tree, not the golden fixture:
    two triangles hit at the same t may resolve differently from the SAH tree."""
    w = h = 64
    pc.upload_scene(ctx, demo, env)
    nodes, info = ctx.device_build_bvh("ploc")
    want_nodes, searched, forced = pr.build(demo.triangles)
    assert lr.first_word_difference(nodes, want_nodes) is None and (info.search_iterations, info.forced_iterations) == (searched, forced)
    ctx.upload_bvh(nodes)
    ctx.set_tile(0, 1, 8)
    ctx.resize(w, h)
    osc = orc.OracleScene(demo.triangles, demo.material_bytes, nodes, env)
    mean = np.zeros((h, w, 4), np.float32)
    try:
        ctx.set_kernel_variant(variant)
        ctx.reset()
        ctx.reset_counters()
        total = dict.fromkeys(capi.COUNTER_NAMES, 0)
        for frame in (2, 3, 4):
            u, a = pc.rt_uniforms(demo, w, h, frame=frame, bounces=4), pc.acc_uniforms(w, h, frame)
            pc.gpu_frame(ctx, u, a, capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE)
            sample, ocnt = orc.raytrace(osc, u.tobytes(), w, h)
            mean = orc.accumulate(a.tobytes(), w, h, sample, mean)
            for k, v in ocnt.items():
                total[k] = total.get(k, 0) + v
        got, cnt = ctx.read_texture(capi.TEX_ACCUMULATION), ctx.counters()
    finally:
        ctx.set_kernel_variant(0)
        ctx.upload_bvh(demo.nodes)
    assert pc.same_bits(got, mean), pc.describe_diff(got, mean)
    pc.check_counters(cnt, total, culled=variant == 0, what="clustering tree")
    assert cnt["stack_overflows"] == 0 and cnt["hits"] > 100


def _queue_two(ctx, sc, first_frame, w, h):
    for k in range(2):
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=first_frame + k).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, first_frame + k).tobytes())
        ctx.submit(capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE)


@pytest.mark.parametrize("variant", [7, 0], ids=["reference-counter-walk", "shipped-walk"])
def test_the_call_changes_no_state(ctx, demo, env, variant):
    """The shape of tests/test_gpu_refit.py::test_the_call_changes_no_state: frames 2, 3 are rendered and read; frames 4, 5 are queued and
    the build comes while they wait (it launches them first); frames 6, 7 are submitted after it, with nothing uploaded.  The same run
    without the call: every image, every counter that is a function of the job, and the launch record agree at every stage."""
    w, h = 48, 32
    want_nodes = pr.build(demo.triangles)[0]

    def observe():
        return ctx.read_texture(capi.TEX_ACCUMULATION), ctx.counters(), ctx.last_launch()

    def run(call):
        ctx.set_kernel_variant(variant)
        pc.upload_scene(ctx, demo, env)
        ctx.set_tile(0, 1, 8)
        ctx.resize(w, h)
        ctx.reset_counters()
        _queue_two(ctx, demo, 2, w, h)
        stages = [observe()]
        _queue_two(ctx, demo, 4, w, h)
        if call:
            nodes, _ = ctx.device_build_bvh("ploc")
            assert lr.first_word_difference(nodes, want_nodes) is None
        stages.append(observe())
        _queue_two(ctx, demo, 6, w, h)
        stages.append(observe())
        return stages

    try:
        with_call, without = run(True), run(False)
    finally:
        ctx.set_kernel_variant(0)
    compared = capi.COUNTER_NAMES if variant == 7 else tuple(k for k in capi.COUNTER_NAMES if k not in pc.WALK_COUNTERS)
    for k, ((img_a, cnt_a, launch_a), (img_b, cnt_b, launch_b)) in enumerate(zip(with_call, without)):
        assert pc.same_bits(img_a, img_b), f"stage {k}: " + pc.describe_diff(img_a, img_b)
        for name in compared:
            assert cnt_a[name] == cnt_b[name], f"stage {k}: counter {name}: {cnt_a[name]} with the call, {cnt_b[name]} without"
        assert launch_a == launch_b, f"stage {k}"
    rays = [stage[1]["rays"] for stage in with_call]
    assert rays[2] > rays[1] > rays[0] > 0
    assert not pc.same_bits(with_call[1][0], with_call[2][0])


def test_entry_point_failures_leave_the_context_usable(ctx):
    lib = ctx.lib
    tris = lr.pack(lr.random_triangles(17))
    want = pr.build(tris)[0]
    need = 33 * 48
    buf = np.full(need, 0xa5, np.uint8)
    good = capi.BvhBuildParams(1, 16, 1024, 0)
    ctx.upload_triangles(tris)

    def refused(params, capacity=need, b=buf, count=True, code=ERR_INVALID, text=""):
        rc, n, info, msg = _ex_raw(lib, ctx.handle, params, b, capacity, count=count)
        assert rc == code and text in msg, (rc, msg)
        assert (buf == 0xa5).all() and n == 12345 and (info.build_ms, info.search_iterations) == (-1.0, 77)

    refused(None, text="null argument")
    refused(good, b=None, text="null argument")
    refused(good, count=False, text="null argument")
    refused(capi.BvhBuildParams(2, 16, 1024, 0), text="unknown method")
    refused(capi.BvhBuildParams(-1, 16, 1024, 0), text="unknown method")
    refused(capi.BvhBuildParams(1, 0, 1024, 0), text="radius")
    refused(capi.BvhBuildParams(1, 65, 1024, 0), text="radius")
    refused(capi.BvhBuildParams(1, 16, -1, 0), text="max_search_iterations")
    refused(capi.BvhBuildParams(1, 16, 65536, 0), text="max_search_iterations")
    refused(capi.BvhBuildParams(1, 16, 1024, 1), text="flags")
    refused(capi.BvhBuildParams(0, 16, 1024, 1), text="flags")
    refused(good, capacity=need - 1, text="node buffer too small")
    with pytest.raises(ValueError):
        ctx.device_build_bvh("sah")
    with pytest.raises(capi.Mi3ptError) as e:
        ctx.device_build_bvh("ploc", radius=65)
    assert e.value.code == ERR_INVALID
    with capi.Context(0) as fresh:
        rc, n, info, msg = _ex_raw(lib, fresh.handle, good, buf, need)
        assert rc == ERR_STATE and "no triangles uploaded" in msg and n == 12345 and (buf == 0xa5).all()
    # exactly enough, the largest budget, no info wanted: fine
    rc, n, info, msg = _ex_raw(lib, ctx.handle, capi.BvhBuildParams(1, 16, 65535, 0), buf, need, info=False)
    assert rc == 0 and n == 33, msg
    assert lr.first_word_difference(buf.view(layout.BVH_NODE), want) is None
    _check(ctx, tris)


def test_a_group_builds_on_member_zero(demo):
    want, searched, forced = pr.build(demo.triangles)
    with capi.Context(devices=[0, 0]) as group:
        group.upload_triangles(demo.triangles)
        nodes, info = group.device_build_bvh("ploc")
    assert lr.first_word_difference(nodes, want) is None and (info.search_iterations, info.forced_iterations) == (searched, forced)
