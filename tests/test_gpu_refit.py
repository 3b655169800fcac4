"""mi3pt_device_refit_bvh (csrc/pt_refit.hip) on the device: every comparison word for word against the law in tests/refit_reference.py.
Shapes: the smallest trees (one leaf that is the root; three nodes), both sides of the 256-thread block boundary (one thread per node:
255 / 257 and 511 / 513 records), unchanged and moved scenes on the host-built and the device-built tree, a chain one thread climbs from
the bottom to the root, zeros of both signs on both sides of a union -- and that the call moves nothing of the context."""
import ctypes
import functools

import numpy as np
import pytest

import ptcommon as pc
import refit_reference as rr
import test_refit_reference as cpu
from mi3pt_host import capi, layout, scenes

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = 1, 4          # include/mi3pt.h
W, H = 48, 32


@pytest.fixture(scope="module")
def ctx(built):
    """a context of this module's own: the refusals need to know what was uploaded, and in which order"""
    with capi.Context(0) as c:
        yield c


def _refit(ctx, nodes, tris, then=None):
    """upload the tree, then the triangles (then `then`, the moved triangles, alone); re-fit"""
    ctx.upload_bvh(nodes)
    ctx.upload_triangles(tris)
    if then is not None:
        ctx.upload_triangles(then)
    got, ms = ctx.device_refit_bvh()
    assert ms > 0 and len(got) == len(nodes)
    return got


def _same(got, want):
    diff = rr.first_difference(got, want)
    assert diff is None, diff


def _first_triangles(mesh, count, seed):
    """the first `count` triangles of a flattened mesh as a scene with its own host-built tree, and the same triangles with every vertex
    displaced"""
    pos, nrm, _ = mesh
    assert len(pos) >= count
    sc = scenes.Scene(pos[:count], nrm[:count], np.zeros(count, int), [scenes.WHITE])
    sc.build_bvh()
    moved = np.array(pos[:count]) + np.random.default_rng(seed).normal(scale=0.05, size=(count, 3, 3))
    return sc, layout.pack_triangles(moved, nrm[:count], np.zeros(count, int))


@functools.lru_cache(maxsize=None)
def _meshes():
    identity = scenes.compose_matrix()
    return {"sphere": scenes.flatten_mesh(scenes.sphere_geometry(0.5, 16, 10), identity, 0),          # 288 triangles
            "plane": scenes.flatten_mesh(scenes.plane_geometry(2.0, 2.0, 12, 12), identity, 0)}         # 288 triangles


@pytest.mark.parametrize("ntris", [1, 2])
def test_smallest_trees(ctx, ntris):
    """one triangle: a single leaf that is the root, no internal node, the climb must not start; two: three nodes, one union"""
    nodes, tris = cpu.cases()[f"{ntris} triangle(s)"]
    assert len(nodes) == 2 * ntris - 1 and (nodes["isLeaf"][0] == 1) == (ntris == 1)
    _same(_refit(ctx, nodes, tris), nodes)
    moved = tris.copy()
    for v in ("aPosition", "bPosition", "cPosition"):
        moved[v] = tris[v] * np.float32(1.5) + np.float32(0.25)
    _same(_refit(ctx, nodes, tris, then=moved), rr.refit_scalar(nodes, moved))


@pytest.mark.parametrize("mesh,ntris", [("sphere", 128), ("plane", 129), ("sphere", 255), ("plane", 256), ("sphere", 257)])
def test_block_boundaries(ctx, mesh, ntris):
    """one thread per record in blocks of 256: 255 | 257 records (128, 129 triangles) and 511 | 513 (256, 257); 255 triangles: 509"""
    sc, moved = _first_triangles(_meshes()[mesh], ntris, ntris)
    assert len(sc.nodes) == 2 * ntris - 1
    _same(_refit(ctx, sc.nodes, sc.triangles), sc.nodes)
    want = rr.refit_vectorised(sc.nodes, moved)
    assert want.tobytes() != sc.nodes.tobytes()
    _same(_refit(ctx, sc.nodes, sc.triangles, then=moved), want)
    _same(want, rr.refit_scalar(sc.nodes, moved))


def test_unchanged_demo_scene_gives_the_uploaded_bytes_back(ctx, demo):
    got = _refit(ctx, demo.nodes, demo.triangles)
    assert got.tobytes() == np.ascontiguousarray(demo.nodes).tobytes(), rr.first_difference(got, demo.nodes)


def test_unchanged_device_built_tree_gives_the_uploaded_bytes_back(ctx, demo):
    """pre-order numbering (the host builder's is breadth-first); its boxes are exact unions too"""
    ctx.upload_triangles(demo.triangles)
    lbvh, _ = ctx.device_build_bvh()
    assert lbvh["right"][0] != 2 and (lbvh["left"][lbvh["isLeaf"] != 1] == np.flatnonzero(lbvh["isLeaf"] != 1) + 1).all()
    got = _refit(ctx, lbvh, demo.triangles)
    assert got.tobytes() == np.ascontiguousarray(lbvh).tobytes(), rr.first_difference(got, lbvh)
    moved = rr.moved_demo().triangles
    _same(_refit(ctx, lbvh, demo.triangles, then=moved), rr.refit_vectorised(lbvh, moved))


def test_moved_demo_scene(ctx, demo):
    """the box slid by 0.6 and turned by 30 degrees; the triangles uploaded alone"""
    moved = rr.moved_demo(0.6, 30.0).triangles
    want = rr.refit_vectorised(demo.nodes, moved)
    assert want.tobytes() != np.ascontiguousarray(demo.nodes).tobytes()
    _same(_refit(ctx, demo.nodes, demo.triangles, then=moved), want)


def test_displaced_blob(ctx):
    """about 20 k triangles, every vertex displaced: many blocks, climbs of every length"""
    verts, faces = scenes.displaced_blob(100)
    normals = scenes._smooth_normals(verts, faces)
    sc = scenes.Scene(verts[faces], normals[faces], np.zeros(len(faces), int), [scenes.WHITE])
    assert len(sc.triangles) == 19800
    sc.build_bvh()
    shaken = verts + np.random.default_rng(3).normal(scale=0.02, size=verts.shape)
    moved = layout.pack_triangles(shaken[faces], normals[faces], np.zeros(len(faces), int))
    want = rr.refit_vectorised(sc.nodes, moved)
    assert (want["min"] != sc.nodes["min"]).any(1).sum() > 30000
    first = _refit(ctx, sc.nodes, sc.triangles, then=moved)
    _same(first, want)
    second, _ = ctx.device_refit_bvh()                     # whatever order the arrivals came in
    assert second.tobytes() == first.tobytes()


def test_chain_tree(ctx):
    """62 internal nodes, each with one leaf child, 63 levels: the thread of a bottom leaf climbs the whole height.  One level more and
    the tree is no longer proper (the reference's 64-entry stack): refused"""
    nodes, tris = rr.chain(62)
    flags = capi.host_scene_compile(nodes, tris)
    assert flags["tree_proper"] and len(nodes) == 125
    _same(_refit(ctx, nodes, tris), rr.refit_scalar(nodes, tris))
    deeper, more = rr.chain(63)
    assert not capi.host_scene_compile(deeper, more)["tree_proper"]
    ctx.upload_bvh(deeper)
    ctx.upload_triangles(more)
    with pytest.raises(capi.Mi3ptError) as e:
        ctx.device_refit_bvh()
    assert e.value.code == ERR_STATE and "proper" in e.value.message


def test_zero_coordinates(ctx):
    """+0 / -0 inside a leaf and on both sides of a union"""
    nodes, tris = cpu.zero_case()
    want = rr.refit_scalar(nodes, tris)
    assert {0, 0x80000000} == set(want["min"][:, 0].view("<u4").tolist()) == set(want["max"][:, 0].view("<u4").tolist())
    _same(_refit(ctx, nodes, tris), want)


def test_repeated_calls_return_the_same_bytes(ctx, demo):
    moved = rr.moved_demo(0.3, 10.0).triangles
    first = _refit(ctx, demo.nodes, demo.triangles, then=moved)
    second, _ = ctx.device_refit_bvh()
    assert first.tobytes() == second.tobytes()
    _same(first, rr.refit_vectorised(demo.nodes, moved))
    # ... and another scene in between leaves nothing behind
    nodes, tris = rr.chain(62)
    _refit(ctx, nodes, tris)
    third = _refit(ctx, demo.nodes, demo.triangles, then=moved)
    assert third.tobytes() == first.tobytes()


def _queue_two(ctx, sc, first_frame):
    """two sample frames with their accumulate steps, submitted and left in the frame queue"""
    for k in range(2):
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, W, H, frame=first_frame + k).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, first_frame + k).tobytes())
        ctx.submit(capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE)


def _observe(ctx):
    """the mean, the counters, the last launch (reading launches the queue)"""
    return ctx.read_texture(capi.TEX_ACCUMULATION), ctx.counters(), ctx.last_launch()


@pytest.mark.parametrize("variant", [7, 0], ids=["reference-counter-walk", "shipped-walk"])
@pytest.mark.parametrize("scene", ["consistent", "stale tree"])
def test_the_call_changes_no_state(ctx, demo, env, scene, variant):
    """Frames 2, 3 are rendered and read; frames 4, 5 are queued and the call comes while they wait (it launches them first, as a
    read-back would); frames 6, 7 are submitted AFTER the call, with nothing uploaded.  The same run without the call, from the same
    uploads: every image, every counter and the launch record are the same at every stage.  Twice: on the demo scene as built, and with
    the moved triangles under the old tree -- the state a host is in when it calls (stale boxes: the image is whatever it is, and the
    re-fitted records differ from what the context holds, so a call that wrote them back would show).
    The counters: under kernel variant 7, which executes exactly the reference's tests, all eight are compared.  Under the shipped walk
    the box- and triangle-test counters are no function of the job -- what the culling walk skips goes by the wave's other lanes, and the
    jobs reach the waves through a ticket queue: tests/test_gpu_aov.py::test_no_trace_in_the_sample_path has the measured spread of
    repeated identical jobs -- so the six counters that are a function of the job are compared there."""
    moved = rr.moved_demo(0.6, 30.0)
    sc = demo if scene == "consistent" else moved

    def run(call):
        ctx.set_kernel_variant(variant)
        pc.upload_scene(ctx, demo, env)
        if sc is moved:
            ctx.upload_triangles(moved.triangles)
        ctx.set_tile(0, 1, 8)
        ctx.resize(W, H)
        ctx.reset_counters()
        _queue_two(ctx, sc, 2)
        stages = [_observe(ctx)]
        _queue_two(ctx, sc, 4)
        if call:
            nodes, _ = ctx.device_refit_bvh()
            _same(nodes, rr.refit_vectorised(demo.nodes, sc.triangles))
        stages.append(_observe(ctx))
        _queue_two(ctx, sc, 6)                           # rendering after the call, the result not uploaded
        stages.append(_observe(ctx))
        return stages

    try:
        with_call, without = run(True), run(False)
    finally:
        ctx.set_kernel_variant(0)
    compared = capi.COUNTER_NAMES if variant == 7 else tuple(k for k in capi.COUNTER_NAMES if k not in pc.WALK_COUNTERS)
    assert len(compared) == (8 if variant == 7 else 6)
    for k, ((img_a, cnt_a, launch_a), (img_b, cnt_b, launch_b)) in enumerate(zip(with_call, without)):
        assert pc.same_bits(img_a, img_b), f"stage {k}: " + pc.describe_diff(img_a, img_b)
        for name in compared:
            assert cnt_a[name] == cnt_b[name], f"stage {k}: counter {name}: {cnt_a[name]} with the call, {cnt_b[name]} without"
        assert launch_a == launch_b, f"stage {k}"
    rays = [stage[1]["rays"] for stage in with_call]
    assert rays[2] > rays[1] > rays[0] > 0               # every stage rendered something
    assert not pc.same_bits(with_call[1][0], with_call[2][0])


def test_refitted_tree_renders_as_the_oracle_says(ctx, orc, demo, env):
    """upload the re-fitted records; two frames; the oracle on the same records, bit for bit, counters as tests/test_gpu_lbvh.py compares"""
    moved = rr.moved_demo(0.6, 30.0)
    pc.upload_scene(ctx, demo, env)
    ctx.upload_triangles(moved.triangles)
    nodes, _ = ctx.device_refit_bvh()
    ctx.upload_bvh(nodes)
    ctx.set_tile(0, 1, 8)
    ctx.resize(W, H)
    osc = orc.OracleScene(moved.triangles, moved.material_bytes, nodes, env)
    for frame in (2, 3):
        u = pc.rt_uniforms(moved, W, H, frame=frame, bounces=4)
        ctx.reset()
        ctx.reset_counters()
        pc.gpu_frame(ctx, u)
        img, cnt = ctx.read_texture(capi.TEX_OUTPUT), ctx.counters()
        want, ocnt = orc.raytrace(osc, u.tobytes(), W, H)
        assert pc.same_bits(img, want), pc.describe_diff(img, want)
        pc.check_counters(cnt, ocnt, culled=True, what="re-fitted tree")
        assert cnt["stack_overflows"] == 0 and cnt["hits"] > 100
    # the same closest hits as on the tree built for the moved scene: a tree decides only between equal t
    moved.build_bvh()
    ctx.upload_bvh(moved.nodes)
    ctx.reset()
    ctx.reset_counters()
    pc.gpu_frame(ctx, u)
    rebuilt, rcnt = ctx.read_texture(capi.TEX_OUTPUT), ctx.counters()
    assert (cnt["rays"], cnt["hits"], cnt["misses"]) == (rcnt["rays"], rcnt["hits"], rcnt["misses"])
    assert pc.same_bits(img, rebuilt), pc.describe_diff(img, rebuilt)
    assert capi.host_bvh_cost(nodes) / capi.host_bvh_cost(demo.nodes) >= 1.0


def _raw(lib, handle, buf, capacity, count=True):
    n, t = ctypes.c_size_t(12345), ctypes.c_float(-1.0)
    rc = lib.mi3pt_device_refit_bvh(handle, buf.ctypes.data_as(ctypes.c_void_p) if buf is not None else None, capacity,
                                    ctypes.byref(n) if count else None, ctypes.byref(t))
    return rc, n.value, lib.mi3pt_last_error().decode()


def test_refusals_leave_the_context_usable(demo):
    need = len(demo.nodes) * 48
    buf = np.full(need, 0xa5, np.uint8)
    with capi.Context(0) as fresh:
        lib = fresh.lib
        # before the uploads; with the tree alone; with the triangles alone
        rc, n, msg = _raw(lib, fresh.handle, buf, need)
        assert rc == ERR_STATE and "no BVH uploaded" in msg and n == 12345 and (buf == 0xa5).all()
        with pytest.raises(capi.Mi3ptError) as e:
            fresh.device_refit_bvh()
        assert e.value.code == ERR_STATE
        fresh.upload_bvh(demo.nodes)
        rc, n, msg = _raw(lib, fresh.handle, buf, need)
        assert rc == ERR_STATE and "no triangles uploaded" in msg and (buf == 0xa5).all()
        with capi.Context(0) as other:
            other.upload_triangles(demo.triangles)
            rc, n, msg = _raw(lib, other.handle, buf, need)
            assert rc == ERR_STATE and "no BVH uploaded" in msg
        # a tree naming a triangle beyond the count
        fresh.upload_triangles(demo.triangles[:1000])
        rc, n, msg = _raw(lib, fresh.handle, buf, need)
        assert rc == ERR_STATE and "beyond the triangle buffer" in msg and (buf == 0xa5).all() and n == 12345
        fresh.upload_triangles(demo.triangles)
        # a capacity one record short; null pointers
        rc, n, msg = _raw(lib, fresh.handle, buf, need - 48)
        assert rc == ERR_INVALID and "node buffer too small" in msg and (buf == 0xa5).all() and n == 12345
        assert _raw(lib, fresh.handle, None, need)[0] == ERR_INVALID
        assert _raw(lib, fresh.handle, buf, need, count=False)[0] == ERR_INVALID and (buf == 0xa5).all()
        # exactly enough, and it still works
        rc, n, msg = _raw(lib, fresh.handle, buf, need)
        assert rc == 0 and n == len(demo.nodes) and buf.tobytes() == np.ascontiguousarray(demo.nodes).tobytes()


def test_records_the_root_does_not_reach_are_refused(demo):
    """a proper tree followed by a record out of the root's reach: the upload takes it, the walks never see it, a bottom-up pass has no
    place for it"""
    nodes = np.zeros(len(demo.nodes) + 1, layout.BVH_NODE)
    nodes[:-1] = demo.nodes
    nodes["isLeaf"][-1], nodes["left"][-1], nodes["right"][-1], nodes["triangleIndex"][-1] = 1, -1, -1, 0
    assert capi.host_scene_compile(nodes, demo.triangles)["tree_proper"]          # (proper as far as any walk can tell)
    with capi.Context(0) as fresh:
        fresh.upload_bvh(nodes)
        fresh.upload_triangles(demo.triangles)
        with pytest.raises(capi.Mi3ptError) as e:
            fresh.device_refit_bvh()
        assert e.value.code == ERR_STATE and "does not reach" in e.value.message


def test_a_group_returns_member_zeros_records(demo):
    moved = rr.moved_demo(0.6, 30.0).triangles
    with capi.Context(devices=[0, 0]) as group:
        assert group.group_size == 2
        got = _refit(group, demo.nodes, demo.triangles, then=moved)
        _same(got, rr.refit_vectorised(demo.nodes, moved))
