"""The device-built linear BVH (mi3pt_device_build_bvh, csrc/pt_lbvh.hip): an alternative tree in
the reference's 48-byte node records.  Checked for structure (every triangle under exactly one
leaf, children after their parent, parent boxes = union of the children), against the oracle on the
SAME tree (bit-identical, counters included), and against the reference's SAH tree: the reference
walk has no culling, so the image may only differ where two triangles tie in t.

The builder is deterministic, so its whole output is also held, node for node, to the plain CPU construction of
tests/lbvh_reference.py: integer fields and padding bit for bit, boxes as fp32 values, no tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import lbvh_reference as lr
import ptcommon as pc
from mi3pt_host import capi, layout, scenes

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4          # include/mi3pt.h


_check_tree = lr.check_tree


def _build(ctx, tris):
    ctx.upload_triangles(tris)
    nodes, ms = ctx.device_build_bvh()
    return nodes


def _same_as_reference(nodes, tris, equal_nan=False, want=None):
    want = lr.reference_nodes(tris) if want is None else want
    diff = lr.first_difference(nodes, want, equal_nan)
    if diff:
        print(diff)
    assert diff is None, diff
    return want


@pytest.mark.parametrize("ntris", [1, 2, 3, 17])
def test_tiny_inputs(gpu_ctx, ntris):
    rng = np.random.default_rng(ntris)
    pos = rng.normal(size=(ntris, 3, 3))
    tris = layout.pack_triangles(pos, np.tile([0.0, 0.0, 1.0], (ntris, 3, 1)), np.zeros(ntris, int))
    gpu_ctx.upload_triangles(tris)
    nodes, ms = gpu_ctx.device_build_bvh()
    _check_tree(nodes, tris)
    _same_as_reference(nodes, tris)


def test_demo_scene_renders_identically(gpu_ctx, orc, demo, env):
    ctx = gpu_ctx
    pc.upload_scene(ctx, demo, env)
    nodes, ms = ctx.device_build_bvh()
    assert ms > 0
    _check_tree(nodes, demo.triangles)
    _same_as_reference(nodes, demo.triangles)
    w, h = 160, 96
    ctx.set_tile(0, 1, 8)
    ctx.resize(w, h)
    u = pc.rt_uniforms(demo, w, h, frame=2, bounces=6)

    def render():
        ctx.reset()
        ctx.reset_counters()
        pc.gpu_frame(ctx, u)
        return ctx.read_texture(capi.TEX_OUTPUT), ctx.counters()

    sah_img, sah_cnt = render()
    ctx.upload_bvh(nodes)
    img, cnt = render()
    want, ocnt = orc.raytrace(orc.OracleScene(demo.triangles, demo.material_bytes, nodes, env), u.tobytes(), w, h)
    assert pc.same_bits(img, want), pc.describe_diff(img, want)
    pc.check_counters(cnt, ocnt, culled=True, what="device-built tree")       # default walk: culls by distance
    # same closest hits as with the reference's tree: same rays, hits and image (no exact ties in this view)
    assert (cnt["rays"], cnt["hits"], cnt["misses"]) == (sah_cnt["rays"], sah_cnt["hits"], sah_cnt["misses"])
    assert pc.same_bits(img, sah_img), pc.describe_diff(img, sah_img)
    assert cnt["stack_overflows"] == 0
    ctx.upload_bvh(demo.nodes)
    ctx.resize(64, 64)


def test_large_mesh_builds_and_renders(gpu_ctx, orc, env):
    sc = scenes.dragon_class_scene()
    ctx = gpu_ctx
    ctx.upload_triangles(sc.triangles)
    ctx.upload_materials(sc.material_bytes)
    ctx.upload_environment(env)
    nodes, ms = ctx.device_build_bvh()
    assert ms < 200.0                               # milliseconds on 870 k triangles (the SAH build: ~0.3 s on 256 host threads)
    _check_tree(nodes, sc.triangles)
    ctx.upload_bvh(nodes)
    w, h = 256, 144
    ctx.set_tile(0, 1, 8)
    ctx.resize(w, h)
    u = pc.rt_uniforms(sc, w, h, frame=2, bounces=4)
    ctx.reset_counters()
    pc.gpu_frame(ctx, u)
    img, cnt = ctx.read_texture(capi.TEX_OUTPUT), ctx.counters()
    assert cnt["stack_overflows"] == 0 and cnt["hits"] > 1000
    band, _ = orc.raytrace(orc.OracleScene(sc.triangles, sc.material_bytes, nodes, env), u.tobytes(), w, h, 9, (h + 7) // 8, 8)
    assert pc.same_bits(img[72:80], band), pc.describe_diff(img[72:80], band)
    ctx.resize(64, 64)


@pytest.mark.parametrize("ntris", [1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513])
def test_block_edges_match_reference(gpu_ctx, ntris):
    """k_lbvh_hierarchy runs n - 1 threads, k_lbvh_emit 2n - 1 and the others n, in blocks of 256"""
    tris = lr.pack(lr.random_triangles(ntris))
    nodes = _build(gpu_ctx, tris)
    _check_tree(nodes, tris)
    _same_as_reference(nodes, tris)


@pytest.mark.parametrize("kind", ["plane", "line", "point"])
def test_degenerate_extents_match_reference(gpu_ctx, kind):
    """one, two, three axes without extent: `extent > 0` is false there and every key is equal in those bits"""
    tris = lr.pack(lr.degenerate(kind))
    cen = lr.centroids(*lr.triangle_boxes(tris))
    flat = {"plane": [2], "line": [1, 2], "point": [0, 1, 2]}[kind]
    assert (cen[:, flat] == 0).all() and all(np.ptp(cen[:, k]) > 0 for k in range(3) if k not in flat)
    _same_as_reference(_build(gpu_ctx, tris), tris)


@pytest.mark.parametrize("distinct,copies", [(5, 8000), (1, 4099)])
def test_equal_keys_across_blocks_match_reference(gpu_ctx, distinct, copies):
    """long runs of equal keys, told apart by sorted position only, in the order a stable sort leaves them"""
    tris = lr.pack(lr.repeated(distinct, copies))
    assert len(set(lr.morton_keys(tris))) == distinct
    _same_as_reference(_build(gpu_ctx, tris), tris)


def test_deepest_tree_matches_reference(gpu_ctx):
    """keys 0, 2^0 .. 2^62 and all ones: 64 levels, the longest searches of the hierarchy kernel and climbs of the emit kernel"""
    tris = lr.pack(lr.chain())
    want = lr.reference_nodes(tris)
    assert lr.depth(want) == 64
    _same_as_reference(_build(gpu_ctx, tris), tris, want=want)


def test_many_blocks_match_reference_and_repeat(gpu_ctx):
    """65 537 triangles: a sort and a fit over many blocks; two builds are byte-identical whatever order the fit's atomics arrive in"""
    tris = lr.pack(lr.random_triangles(65537))
    first = _build(gpu_ctx, tris)
    second = _build(gpu_ctx, tris)
    assert first.tobytes() == second.tobytes()
    _same_as_reference(first, tris)


@pytest.mark.parametrize("axes", [3, 2], ids=["xyz", "xy"])
def test_range_extremes_match_reference(gpu_ctx, axes):
    """coordinates up to 3e38 of both signs: hi - lo overflows to +inf, t is 0 or NaN -> 0 on those axes"""
    tris = lr.pack(lr.range_extremes(axes=axes))
    cen = lr.centroids(*lr.triangle_boxes(tris))
    with np.errstate(over="ignore"):
        assert np.isfinite(cen).all() and all(np.isinf(cen[:, k].max() - cen[:, k].min()) for k in range(axes))
    assert len(set(lr.morton_keys(tris))) == (1 if axes == 3 else 64)
    _same_as_reference(_build(gpu_ctx, tris), tris)


def test_non_finite_vertices_match_reference(gpu_ctx):
    """mi3pt_upload_triangles takes NaN positions.  A NaN vertex is ignored by its triangle's box; an all-NaN triangle has a NaN
    box, stays out of the bounds, gets key 0, and its NaN reaches no other node: fminf / fmaxf drop it at the first union."""
    tris = lr.pack(lr.non_finite())
    nodes = _build(gpu_ctx, tris)
    _check_tree(nodes, tris, boxes=False)
    _same_as_reference(nodes, tris, equal_nan=True)
    nan_leaf = int(np.flatnonzero(nodes["triangleIndex"] == 65)[0])
    on_path, parent = {nan_leaf}, {}
    for i in np.flatnonzero(nodes["isLeaf"] == 0):
        parent[int(nodes["left"][i])] = parent[int(nodes["right"][i])] = int(i)
    x = nan_leaf
    while x in parent:
        x = parent[x]
        on_path.add(x)
    assert 0 in on_path
    off_path = np.array([i for i in range(len(nodes)) if i not in on_path])
    assert not np.isnan(nodes["min"][off_path]).any() and not np.isnan(nodes["max"][off_path]).any()
    assert np.isnan(nodes["min"][nan_leaf]).all() and np.isnan(nodes["max"][nan_leaf]).all()


def _build_raw(lib, handle, buf, capacity, count=True, ms=True):
    n, t = ctypes.c_size_t(12345), ctypes.c_float()
    rc = lib.mi3pt_device_build_bvh(handle, buf.ctypes.data_as(ctypes.c_void_p), capacity,
                                    ctypes.byref(n) if count else None, ctypes.byref(t) if ms else None)
    return rc, n.value, lib.mi3pt_last_error().decode()


def test_entry_point_failures_leave_the_context_usable(gpu_ctx):
    lib = gpu_ctx.lib
    tris = lr.pack(lr.random_triangles(17))
    want = lr.reference_nodes(tris)
    need = 33 * 48

    def builds_17(ctx):
        _same_as_reference(_build(ctx, tris), tris, want=want)

    builds_17(gpu_ctx)
    # capacity one byte short: refused, the buffer untouched
    buf = np.full(need, 0xa5, np.uint8)
    rc, n, msg = _build_raw(lib, gpu_ctx.handle, buf, need - 1)
    assert rc == ERR_INVALID and "node buffer too small" in msg
    assert (buf == 0xa5).all() and n == 12345
    builds_17(gpu_ctx)
    # no count pointer
    rc, n, msg = _build_raw(lib, gpu_ctx.handle, buf, need, count=False)
    assert rc == ERR_INVALID and (buf == 0xa5).all()
    builds_17(gpu_ctx)
    # exactly enough, and no time wanted: fine
    rc, n, msg = _build_raw(lib, gpu_ctx.handle, buf, need, ms=False)
    assert rc == 0 and n == 33 and lr.first_difference(buf.view(layout.BVH_NODE), want) is None
    # a context that has no triangles
    with capi.Context(0) as fresh:
        rc, n, msg = _build_raw(lib, fresh.handle, buf, need)
        assert rc == ERR_STATE and "no triangles uploaded" in msg and n == 12345
        builds_17(fresh)
