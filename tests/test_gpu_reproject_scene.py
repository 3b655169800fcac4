"""The reprojection across a scene change on the GPU (mi3pt_keep_geometry, mi3pt_reproject_scene; csrc/pt_reproject_scene.hip) against its
numpy restatement tests/reproject_scene_reference.py, bit for bit (ptcommon.same_bits, no tolerance anywhere).  The reference is given
what the kernel is given: the device's own feature images of the two scenes and views, the kept and the current triangle records as they
were uploaded, the images written with mi3pt_write_texture / mi3pt_write_moments as the device returns them, and the camera frame of
mi3pt_host_view_frame."""
import ctypes

import numpy as np
import pytest

import moments_edge_cases as ec
import ptcommon as pc
import reproject_reference as rr
import reproject_scene_cases as cases
import reproject_scene_reference as rs
import test_gpu_reproject as tgr
from mi3pt_host import capi, scenes

pytestmark = pytest.mark.gpu
RT, ACC = capi.SUBMIT_RAYTRACE, capi.SUBMIT_ACCUMULATE
TEX = capi.TEX_ACCUMULATION
F = np.float32
SIZES = tgr.SIZES
TIGHT = dict(plane_tolerance=0.005, normal_cos_min=0.99, max_history=3, max_history_moved=1)


@pytest.fixture(scope="module")
def ctx(built):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def variants(demo):
    """name -> (the scene uploaded after mi3pt_keep_geometry, or None for no upload; the new view's (position, direction) of size (w, h),
    or None for the old view)"""
    cam = demo.camera
    orbit = rr.orbit(cam["position"], cam["target"], 2.0)
    moved_camera = (tuple(np.array(cam["position"]) + np.array(cases.TRANSLATION)), demo.camera_direction())
    return {"kept": (None, orbit), "box": (cases.box_moved(demo), None), "box and sphere": (cases.box_moved_sphere_squashed(demo), orbit),
            "translated": (cases.translated(demo), moved_camera), "same records": (demo, orbit)}


def _case(c, demo, variant, w, h, seed=1, rect=None, images=None, f16=False, **params):
    """the kept scene's features in the old view, the images, keep, the upload, the new view, the call.  Returns (device (A', M'),
    reference (A', M', info), written (A, M))"""
    new_scene, view = variant
    pc.upload_scene(c, demo)
    ua = tgr._uniforms(demo, w, h)
    c.reset()
    c.set_uniforms(capi.PASS_RAYTRACE, ua.tobytes())
    c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(*(rect or (w, h)), 2).tobytes())
    c.render_aovs(capi.AOV_ALL)
    old = tgr._features(c)
    acc, mo = images if images is not None else tgr._random_images(w, h, seed)
    c.write_texture(TEX, acc)
    c.write_moments(mo)
    acc, mo = c.read_texture(TEX), c.read_moments()
    c.keep_geometry(True)
    try:
        if new_scene is not None:
            pc.upload_scene(c, new_scene)
        c.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h, view).tobytes())
        c.reproject_scene(**params)
        got = c.read_texture(TEX), c.read_moments()
    finally:
        c.keep_geometry(False)
    new = tgr._features(c)
    current = demo if new_scene is None else new_scene
    want = rs.reproject_scene(acc, mo, capi.host_view_frame(ua.tobytes()), (F(w), F(h)), new, old, rect or (w, h), current.triangles, demo.triangles,
                              store_f16=f16, **params)
    return got, want, (acc, mo)


@pytest.mark.parametrize("name", ["kept", "box", "box and sphere", "translated"])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_device_equals_the_reference(ctx, demo, env, variants, w, h, name):
    tgr._configure(ctx, demo, env, w, h)
    got, want, _ = _case(ctx, demo, variants[name], w, h)
    tgr._same(got, want, f"{name}, {w} x {h}")
    info = want[2]
    hit = ctx.read_aov(capi.AOV_IDS)[..., 2] == 1
    tri = ctx.read_aov(capi.AOV_IDS)[..., 0]
    carried, moved = int((info["carried"] & hit).sum()), int(info["moved"].sum())
    print(f"{name}, {w} x {h}: {carried} of {int(hit.sum())} hit texels carried, {moved} moved, {int((info['carried'] & info['moved']).sum())} of them carried")
    assert not info["carried"][~hit].any() and carried > 0 and np.array_equal(info["moved"] | info["static"], hit)
    on_box = (tri >= cases.BOX.start) & (tri < cases.BOX.stop)
    if name == "kept":
        assert moved == 0 and want[1][..., 3].max() == 64
    if name == "box":
        assert np.array_equal(info["moved"], hit & on_box) and (info["carried"] & info["moved"]).sum() > 0.5 * moved
    if name == "box and sphere":
        assert np.array_equal(info["static"], hit & (tri < cases.GROUND.stop)) and (info["carried"] & info["moved"]).sum() > 0.5 * moved
    if name == "translated":
        # every texel's point is the one the old view saw at the same texel; 15 % of the random images' texels hold n = 0 and do not count
        # as taps: at worst the texel's own tap alone weighs, so 85 % carry -- 0.75 is twelve standard deviations below at 2 000 texels
        assert moved == hit.sum() and carried >= 0.75 * hit.sum()
    if name != "kept":
        assert want[1][..., 3][info["carried"] & info["moved"]].max() == 8
    # other parameters, shorter histories
    got, want, _ = _case(ctx, demo, variants[name], w, h, seed=2, **TIGHT)
    tgr._same(got, want, f"{name}, {w} x {h}, tight parameters")
    info = want[2]
    assert np.all(want[1][..., 3][info["carried"] & info["moved"]] == 1) and want[1][..., 3].max() == (3 if info["static"].any() else 1)


@pytest.mark.parametrize("w,h", SIZES)
def test_the_same_records_uploaded_again_equal_mi3pt_reproject(ctx, demo, env, variants, w, h):
    """kept geometry, the same records uploaded again (the hand-over: two buffers, every texel static), then mi3pt_reproject_scene; a
    second context runs mi3pt_reproject from the same images: mean and moments bit for bit"""
    tgr._configure(ctx, demo, env, w, h)
    got, want, _ = _case(ctx, demo, variants["same records"], w, h, seed=3, max_history_moved=1)
    tgr._same(got, want, f"the same records, {w} x {h}")
    with capi.Context(0) as other:
        tgr._configure(other, demo, env, w, h)
        plain, _, _ = tgr._case(other, demo, w, h, variants["same records"][1], seed=3)
    tgr._same(got, plain, f"mi3pt_reproject_scene against mi3pt_reproject, {w} x {h}")


@pytest.mark.parametrize("w,h", SIZES)
def test_f16_storage_a_rectangle_and_a_bound_image(ctx, demo, env, variants, w, h):
    variant = variants["box and sphere"]
    try:
        tgr._configure(ctx, demo, env, w, h, f16=True)
        got, want, _ = _case(ctx, demo, variant, w, h, f16=True)
        tgr._same(got, want, f"F16, {w} x {h}")
        assert pc.same_bits(got[0], got[0].astype(np.float16).astype(F))
        tgr._configure(ctx, demo, env, w, h)
        rect = (w - 9, h - 5)
        got, want, written = _case(ctx, demo, variant, w, h, rect=rect)
        tgr._same(got, want, f"rectangle {rect}, {w} x {h}")
        assert pc.same_bits(got[0][rect[1]:], written[0][rect[1]:]) and pc.same_bits(got[1][:, rect[0]:], written[1][:, rect[0]:])
        # a caller-owned accumulation image: the result is copied into it on the stream
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipFree.argtypes = [ctypes.c_void_p]
        bound, nbytes = ctypes.c_void_p(), h * w * 16
        assert hip.hipMalloc(ctypes.byref(bound), nbytes) == 0 and hip.hipMemset(bound, 0, nbytes) == 0 and hip.hipDeviceSynchronize() == 0
        ctx.bind_accumulation(bound.value, nbytes)
        try:
            got, want, _ = _case(ctx, demo, variant, w, h, rect=rect)
            tgr._same(got, want, f"bound image, {w} x {h}")
            host = np.empty((h, w, 4), F)
            assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), bound, nbytes, 2) == 0          # hipMemcpyDeviceToHost
            assert pc.same_bits(host, want[0])
        finally:
            ctx.bind_accumulation(None, 0)
            hip.hipFree(bound)
    finally:
        tgr._restore(ctx)


def test_features_mask_counters_and_timing_after_the_call(ctx, demo, env, variants):
    """After the call: the four feature images are the new scene's in the new view, the sample mask is gone, no counter and nothing
    mi3pt_debug_last_launch reports has moved; with timing on both passes report a time"""
    w, h = SIZES[1]
    new_scene, view = variants["box and sphere"]
    tgr._configure(ctx, demo, env, w, h)
    ctx.enable_timing(True)
    try:
        ctx.reset()
        ctx.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
        ctx.submit_frames(RT | ACC, 2)
        ctx.flush()
        mask = np.ones(((h + 7) // 8, (w + 7) // 8), np.uint8)
        mask[0] = 0
        ctx.set_sample_mask(mask)
        ctx.render_aovs(capi.AOV_ALL)
        old = tgr._features(ctx)
        acc, mo = ctx.read_texture(TEX), ctx.read_moments()
        ctx.keep_geometry(True)
        pc.upload_scene(ctx, new_scene)
        ctx.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h, view).tobytes())
        before = ctx.counters(), ctx.last_launch()
        ctx.reproject_scene()
        got = ctx.read_texture(TEX), ctx.read_moments()
        ctx.keep_geometry(False)
        assert ctx.pass_time_us(capi.PASS_REPROJECT) > 0 and ctx.pass_time_us(capi.PASS_AOV) > 0
        assert (ctx.counters(), ctx.last_launch()) == before
        assert ctx.read_sample_mask().all()
        want = rs.reproject_scene(acc, mo, capi.host_view_frame(tgr._uniforms(demo, w, h).tobytes()), (F(w), F(h)), tgr._features(ctx), old, (w, h),
                                  new_scene.triangles, demo.triangles)
        tgr._same(got, want, "after two sampled frames")
        after = {which: ctx.read_aov(which) for which in range(capi.AOV_COUNT)}
        ctx.render_aovs(capi.AOV_ALL)
        for which in range(capi.AOV_COUNT):
            assert np.array_equal(after[which].view(np.int32), ctx.read_aov(which).view(np.int32)), capi.AOV_NAMES[which]
    finally:
        ctx.enable_timing(False)


def test_a_second_keep_replaces_the_first_and_features_may_follow_it(demo, env, variants):
    """keep, upload (the hand-over), keep again (the handed-over buffer is freed: the moved scene is the previous geometry now), THEN the
    features -- no upload in between: accepted --, the demo scene uploaded again, the call: from the moved scene back to the demo's.  A
    context destroyed while it keeps a buffer frees it"""
    w, h = SIZES[1]
    moved = variants["box"][0]
    with capi.Context(0) as c:
        tgr._configure(c, demo, env, w, h)
        ua = tgr._uniforms(demo, w, h)
        c.set_uniforms(capi.PASS_RAYTRACE, ua.tobytes())
        c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
        c.keep_geometry(True)
        pc.upload_scene(c, moved)
        c.keep_geometry(True)
        c.render_aovs(capi.AOV_ALL)
        old = tgr._features(c)
        acc, mo = tgr._random_images(w, h, 4)
        c.write_texture(TEX, acc)
        c.write_moments(mo)
        acc, mo = c.read_texture(TEX), c.read_moments()
        pc.upload_scene(c, demo)
        c.reproject_scene()
        got = c.read_texture(TEX), c.read_moments()
        want = rs.reproject_scene(acc, mo, capi.host_view_frame(ua.tobytes()), (F(w), F(h)), tgr._features(c), old, (w, h), demo.triangles, moved.triangles)
        tgr._same(got, want, "from the moved scene back")
        assert want[2]["moved"].any() and (want[2]["carried"] & want[2]["moved"]).any()


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("max_history", [64, 1 << 24])
def test_value_edges(ctx, demo, env, variants, max_history, f16):
    """test_gpu_reproject.py::test_value_edges through this kernel: the finite catalogue of tests/moments_edge_cases.py at 50 x 37, the box
    and the sphere moved and the camera orbited, so that static and moved texels both gather edge taps; the moved texels' cap is 8"""
    w, h = SIZES[1]
    try:
        tgr._configure(ctx, demo, env, w, h, f16=f16)
        acc, mo, where = ec.placed(w, h, 12, finite=True)
        assert not ec.seam_sides(where, w, h)
        got, want, _ = _case(ctx, demo, variants["box and sphere"], w, h, images=(acc, mo), f16=f16, max_history=max_history, max_history_moved=8)
        what = f"max_history {max_history}, f16 {f16}"
        info = want[2]
        tgr.assert_value_branches(info, want[1], max_history, what, capped=max_history == 64)
        n_moved = want[1][..., 3][info["carried"] & info["moved"]]
        assert (n_moved == 8).any() and (n_moved < 8).any()
        tgr._same_or_nan(got, want, what)
    finally:
        tgr._restore(ctx)


def test_non_finite_images_complete_and_leave_the_outside_untouched(ctx, demo, env, variants):
    """... and inside the rectangle every texel is the reference's (a NaN where it has one)"""
    w, h = SIZES[0]
    tgr._configure(ctx, demo, env, w, h)
    rng = np.random.default_rng(9)
    acc, mo = tgr._random_images(w, h, 3)
    for img in (acc, mo):
        bad = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e38, -1.0], F), size=img.shape)
        img[...] = np.where(rng.random(img.shape) < 0.3, bad, img)
    rect = (w - 16, h - 8)
    got, want, _ = _case(ctx, demo, variants["box and sphere"], w, h, rect=rect, images=(acc, mo), max_history=1 << 24, max_history_moved=1 << 24)
    ctx.sync()
    for g, written in zip(got, (acc, mo)):
        assert pc.same_bits(g[rect[1]:], written[rect[1]:]) and pc.same_bits(g[:, rect[0]:], written[:, rect[0]:])
    assert np.all(got[0][:rect[1], :rect[0], 3] == 1)
    tgr._same_or_nan(got, want, "non-finite images")


def test_error_codes(ctx, demo, env, variants):
    lib = capi.load_library()
    w, h = SIZES[1]
    tgr._configure(ctx, demo, env, w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())

    def code(fn):
        with pytest.raises(capi.Mi3ptError) as e:
            fn()
        return e.value.code

    # no kept geometry; keep(0) followed by the call
    ctx.keep_geometry(False)
    ctx.render_aovs(capi.AOV_ALL)
    assert code(ctx.reproject_scene) == 4
    ctx.keep_geometry(True)
    ctx.reproject_scene()                          # (kept and current are one buffer)
    ctx.keep_geometry(False)
    assert code(ctx.reproject_scene) == 4
    # an upload between the feature render and keep, in either order
    ctx.render_aovs(capi.AOV_ALL)
    ctx.upload_triangles(demo.triangles)
    ctx.keep_geometry(True)
    assert code(ctx.reproject_scene) == 4
    ctx.render_aovs(capi.AOV_ALL)                  # keep, then the features, no upload in between: accepted
    ctx.reproject_scene()
    ctx.keep_geometry(True)
    ctx.upload_triangles(demo.triangles)
    ctx.render_aovs(capi.AOV_ALL)                  # (features of the geometry uploaded AFTER the keep)
    assert code(ctx.reproject_scene) == 4
    # the triangle count changed
    fewer = scenes.Scene(np.array(demo.positions)[:-1], np.array(demo.normals)[:-1], np.array(demo.material_index)[:-1], demo.materials)
    fewer.build_bvh()
    pc.upload_scene(ctx, demo)
    ctx.render_aovs(capi.AOV_ALL)
    ctx.keep_geometry(True)
    pc.upload_scene(ctx, fewer)
    assert code(ctx.reproject_scene) == 4
    pc.upload_scene(ctx, demo)
    ctx.reproject_scene()                          # (the count is the kept one again: the first upload after the keep was handed over)
    # the arguments
    ctx.render_aovs(capi.AOV_ALL)
    ctx.keep_geometry(True)
    assert lib.mi3pt_reproject_scene(ctx.handle, None) == 1
    for bad in (dict(plane_tolerance=-1.0), dict(plane_tolerance=float("nan")), dict(plane_tolerance=float("inf")),
                dict(normal_cos_min=1.5), dict(normal_cos_min=-1.5), dict(normal_cos_min=float("nan")),
                dict(max_history=0), dict(max_history=(1 << 24) + 1), dict(max_history_moved=0), dict(max_history_moved=(1 << 24) + 1),
                dict(max_history_moved=-3), dict(flags=1)):
        assert code(lambda: ctx.reproject_scene(**bad)) == 1, bad
    ctx.reproject_scene(plane_tolerance=0.0, normal_cos_min=-1.0, max_history=1 << 24, max_history_moved=1 << 24)
    # another resolution in the new view
    ctx.render_aovs(capi.AOV_ALL)
    ctx.keep_geometry(True)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, bounces=4, res=(w - 1, h)).tobytes())
    assert code(ctx.reproject_scene) == 4
    ctx.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h).tobytes())
    ctx.reproject_scene()
    # the mode and the image
    ctx.render_aovs(capi.AOV_ALL)
    ctx.keep_geometry(True)
    ctx.set_mean_by_count(False)
    assert code(ctx.reproject_scene) == 4
    ctx.set_mean_by_count(True)
    ctx.set_moments(False)
    assert code(ctx.reproject_scene) == 4
    ctx.keep_geometry(False)
    # keep without triangles; before resize; a rank of a tile split; a device group
    with capi.Context(0) as c:
        c.set_moments(True)
        c.set_mean_by_count(True)
        c.keep_geometry(False)
        assert code(lambda: c.keep_geometry(True)) == 4
        c.set_tile(0, 2, 8)
        pc.upload_scene(c, demo, env)
        c.keep_geometry(True)
        assert code(c.reproject_scene) == 4
        c.resize(w, h)
        c.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h).tobytes())
        c.render_aovs(capi.AOV_ALL)
        assert code(c.reproject_scene) == 4
    with capi.Context(devices=[0, 0]) as g:
        g.set_moments(True)
        g.set_mean_by_count(True)
        pc.upload_scene(g, demo, env)
        g.resize(w, h)
        g.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h).tobytes())
        g.render_aovs(capi.AOV_ALL)
        assert code(lambda: g.keep_geometry(True)) == 4
        assert code(g.reproject_scene) == 4
