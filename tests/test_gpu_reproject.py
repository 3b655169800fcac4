"""The reprojection on the GPU (mi3pt_reproject; csrc/pt_reproject.hip) against its numpy restatement tests/reproject_reference.py, bit for
bit (ptcommon.same_bits, no tolerance anywhere).  The reference is given what the kernel is given: the device's own feature images of
the two views, the images written with mi3pt_write_texture / mi3pt_write_moments as the device returns them, and the camera frame of
mi3pt_host_view_frame (tests/test_reproject_host.py holds that one to an independent computation)."""
import ctypes
import math

import numpy as np
import pytest

import moments_edge_cases as ec
import ptcommon as pc
import reproject_reference as rr
from mi3pt_host import capi

pytestmark = pytest.mark.gpu
RT, ACC = capi.SUBMIT_RAYTRACE, capi.SUBMIT_ACCUMULATE
TEX = capi.TEX_ACCUMULATION
F = np.float32
SIZES = [(64, 48), (50, 37)]
OLD = (("position", capi.AOV_POSITION), ("normal", capi.AOV_NORMAL), ("ids", capi.AOV_IDS))


@pytest.fixture(scope="module")
def ctx(built):
    c = capi.Context(0)
    yield c
    c.close()


def _configure(c, sc, env, w, h, f16=False):
    c.set_tile(0, 1, 8)
    c.set_storage(capi.STORAGE_F16 if f16 else capi.STORAGE_F32)
    c.set_moments(True)
    c.set_mean_by_count(True)
    pc.upload_scene(c, sc, env)
    c.resize(w, h)


def _restore(c):
    c.set_storage(capi.STORAGE_F32)


def _views(sc, w, h):
    """name -> (position, direction) of the views B of the issue"""
    cam = sc.camera
    p, t = np.array(cam["position"], np.float64), np.array(cam["target"], np.float64)
    d = np.array(sc.camera_direction(), np.float64)
    third = 2 * math.atan(w / h * math.tan(math.radians(cam["fov"]) / 2)) / 3        # a third of the horizontal field of view
    c, s = math.cos(third), math.sin(third)
    return {"identical": (tuple(p), tuple(d)),
            "orbit": rr.orbit(cam["position"], cam["target"], 2.0),
            "dolly": (tuple(p + 0.25 * (t - p)), tuple(d)),
            "pan": (tuple(p), (c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]))}


def _uniforms(sc, w, h, view=None, frame=2):
    if view is None:
        return pc.rt_uniforms(sc, w, h, frame=frame, bounces=4)
    return pc.rt_uniforms(sc, w, h, frame=frame, bounces=4, position=view[0], direction=view[1])


def _random_images(w, h, seed):
    """a seeded mean and moments image; n of 0, 1, 2 and 500 among the texels"""
    rng = np.random.default_rng(seed)
    acc = (rng.random((h, w, 4), dtype=F) * 4).astype(F)
    acc[..., 3] = 1
    mo = (rng.random((h, w, 4), dtype=F) * 50).astype(F)
    mo[..., 3] = rng.choice(np.array([0, 1, 2, 500], F), size=(h, w), p=[0.15, 0.15, 0.2, 0.5])
    return acc, mo


def _features(c):
    return {name: c.read_aov(which) for name, which in OLD}


def _case(c, sc, w, h, view, seed=1, rect=None, images=None, f16=False, **params):
    """view A's features, the images, view B, the call.  Returns (device (A', M'), reference (A', M', info), written (A, M))"""
    ua = _uniforms(sc, w, h)
    c.reset()
    c.set_uniforms(capi.PASS_RAYTRACE, ua.tobytes())
    c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(*(rect or (w, h)), 2).tobytes())
    c.render_aovs(capi.AOV_ALL)
    old = _features(c)
    acc, mo = images if images is not None else _random_images(w, h, seed)
    c.write_texture(TEX, acc)
    c.write_moments(mo)
    acc, mo = c.read_texture(TEX), c.read_moments()
    c.set_uniforms(capi.PASS_RAYTRACE, _uniforms(sc, w, h, view).tobytes())
    c.reproject(**params)
    got = c.read_texture(TEX), c.read_moments()
    new = _features(c)
    kw = {k: params[k] for k in ("plane_tolerance", "normal_cos_min", "max_history") if k in params}
    want = rr.reproject(acc, mo, capi.host_view_frame(ua.tobytes()), (F(w), F(h)), new, old, rect or (w, h), store_f16=f16, **kw)
    return got, want, (acc, mo)


def _same(got, want, what):
    assert pc.same_bits(got[0], want[0]), f"{what}: mean: " + pc.describe_diff(got[0], want[0])
    assert pc.same_bits(got[1], want[1]), f"{what}: moments: " + pc.describe_diff(got[1], want[1])


def _same_or_nan(got, want, what):
    """_same for images with non-finite texels (ptcommon.same_bits_or_nan): every texel is compared"""
    pc.assert_same_or_nan(got, want, what)


@pytest.mark.parametrize("name", ["identical", "orbit", "dolly", "pan"])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_device_equals_the_reference(ctx, demo, env, w, h, name):
    _configure(ctx, demo, env, w, h)
    view = _views(demo, w, h)[name]
    got, want, _ = _case(ctx, demo, w, h, view)
    _same(got, want, f"{name}, {w} x {h}")
    info = want[2]
    hit = ctx.read_aov(capi.AOV_IDS)[..., 2] == 1
    carried, restarted = int((info["carried"] & hit).sum()), int((info["restarted"] & hit).sum())
    print(f"{name}, {w} x {h}: {carried} of {int(hit.sum())} hit texels carried, {restarted} restart")
    assert not info["carried"][~hit].any() and carried > 0
    if name == "orbit":
        assert carried >= 0.5 * hit.sum() and restarted >= 0.01 * hit.sum()
    if name == "pan":
        assert restarted >= 0.25 * hit.sum()              # a third of the image is new
    # other parameters, a shorter history
    got, want, _ = _case(ctx, demo, w, h, view, seed=2, plane_tolerance=0.005, normal_cos_min=0.99, max_history=3)
    _same(got, want, f"{name}, {w} x {h}, tight parameters")
    assert want[1][..., 3].max() == 3


@pytest.mark.parametrize("w,h", SIZES)
def test_f16_storage_a_rectangle_and_a_bound_image(ctx, demo, env, w, h):
    view = _views(demo, w, h)["orbit"]
    try:
        _configure(ctx, demo, env, w, h, f16=True)
        got, want, _ = _case(ctx, demo, w, h, view, f16=True)
        _same(got, want, f"F16, {w} x {h}")
        assert pc.same_bits(got[0], got[0].astype(np.float16).astype(F))
        _configure(ctx, demo, env, w, h)
        rect = (w - 9, h - 5)
        got, want, written = _case(ctx, demo, w, h, view, rect=rect)
        _same(got, want, f"rectangle {rect}, {w} x {h}")
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
            got, want, _ = _case(ctx, demo, w, h, view, rect=rect)
            _same(got, want, f"bound image, {w} x {h}")
            host = np.empty((h, w, 4), F)
            assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), bound, nbytes, 2) == 0          # hipMemcpyDeviceToHost
            assert pc.same_bits(host, want[0])
        finally:
            ctx.bind_accumulation(None, 0)
            hip.hipFree(bound)
    finally:
        _restore(ctx)


def test_features_mask_counters_and_the_frames_that_follow(ctx, demo, env):
    """After the call: the four feature images are view B's, the sample mask is gone, no counter and nothing mi3pt_debug_last_launch reports
    has moved; three frames sampled on top equal a second context that is GIVEN the reference's (A', M') and renders the same frames"""
    w, h = SIZES[1]
    _configure(ctx, demo, env, w, h)
    view = _views(demo, w, h)["orbit"]
    ctx.reset()
    ctx.set_uniforms(capi.PASS_RAYTRACE, _uniforms(demo, w, h).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
    ctx.submit_frames(RT | ACC, 2)
    ctx.flush()
    mask = np.ones(((h + 7) // 8, (w + 7) // 8), np.uint8)
    mask[0] = 0
    ctx.set_sample_mask(mask)
    before = ctx.counters(), ctx.last_launch()
    got, want, _ = _case_keeping_state(ctx, demo, w, h, view)
    _same(got, want, "after two sampled frames")
    assert (ctx.counters(), ctx.last_launch()) == before
    assert ctx.read_sample_mask().all()
    after = {which: ctx.read_aov(which) for which in range(capi.AOV_COUNT)}
    ctx.render_aovs(capi.AOV_ALL)
    for which in range(capi.AOV_COUNT):
        assert np.array_equal(after[which].view(np.int32), ctx.read_aov(which).view(np.int32)), capi.AOV_NAMES[which]
    ub = _uniforms(demo, w, h, view, frame=70)
    ctx.set_uniforms(capi.PASS_RAYTRACE, ub.tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
    ctx.submit_frames(RT | ACC, 3)
    first = ctx.read_texture(TEX), ctx.read_moments()
    assert first[1][..., 3].max() == want[1][..., 3].max() + 3
    with capi.Context(0) as other:
        _configure(other, demo, env, w, h)
        other.write_texture(TEX, want[0])
        other.write_moments(want[1])
        other.set_uniforms(capi.PASS_RAYTRACE, ub.tobytes())
        other.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
        other.submit_frames(RT | ACC, 3)
        _same(first, (other.read_texture(TEX), other.read_moments()), "reproject + 3 frames")


def _case_keeping_state(c, sc, w, h, view):
    """_case without the reset: the mean and the moments are what the context sampled"""
    ua = _uniforms(sc, w, h)
    c.render_aovs(capi.AOV_ALL)
    old = _features(c)
    acc, mo = c.read_texture(TEX), c.read_moments()
    c.set_uniforms(capi.PASS_RAYTRACE, _uniforms(sc, w, h, view).tobytes())
    c.reproject()
    got = c.read_texture(TEX), c.read_moments()
    want = rr.reproject(acc, mo, capi.host_view_frame(ua.tobytes()), (F(w), F(h)), _features(c), old, (w, h))
    return got, want, (acc, mo)


def assert_value_branches(info, moments_after, max_history, what, capped=True):
    """on the reference alone: carried and restarted texels, and carried counts at the cap and below it (DESIGN.md "Pinned value range")"""
    n_new = moments_after[..., 3][info["carried"]]
    at_cap, below = int((n_new == max_history).sum()), int((n_new < max_history).sum())
    print(f"{what}: carried {int(info['carried'].sum())}, restarted {int(info['restarted'].sum())}, at the cap of {max_history} {at_cap}, below it {below}")
    assert info["carried"].any() and info["restarted"].any() and below > 0 and (at_cap > 0 or not capped)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("max_history", [64, 1 << 24])
@pytest.mark.parametrize("name", ["identical", "orbit"])
def test_value_edges(ctx, demo, env, name, max_history, f16):
    """the finite catalogue of tests/moments_edge_cases.py in the old view's images at 50 x 37 (35 tiles of 8 x 8, edge texels on both sides of
    every tile seam): counts on either side of `n0 >= 1` and `n0 >= 2`, M2 that the fmaxf clamps, counts at and above both caps, means
    at the ends of binary16.  Finite inputs, but not finite results (3e38 * bw sums overflow, inf * (n' - 1 = 0) is a NaN): compared
    with ptcommon.same_bits_or_nan, every texel"""
    w, h = SIZES[1]
    try:
        _configure(ctx, demo, env, w, h, f16=f16)
        acc, mo, where = ec.placed(w, h, 11, finite=True)
        assert not ec.seam_sides(where, w, h)
        got, want, _ = _case(ctx, demo, w, h, _views(demo, w, h)[name], images=(acc, mo), f16=f16, max_history=max_history)
        what = f"{name}, max_history {max_history}, f16 {f16}"
        assert_value_branches(want[2], want[1], max_history, what, capped=max_history == 64 or name == "identical")
        _same_or_nan(got, want, what)
    finally:
        _restore(ctx)


def test_non_finite_images_complete_and_leave_the_outside_untouched(ctx, demo, env):
    """... and inside the rectangle every texel is the reference's (a NaN where it has one).  Only the two images are non-finite: the
    feature images are rendered, no index depends on a written value"""
    w, h = SIZES[0]
    _configure(ctx, demo, env, w, h)
    rng = np.random.default_rng(9)
    acc, mo = _random_images(w, h, 3)
    for img in (acc, mo):
        bad = rng.choice(np.array([np.nan, np.inf, -np.inf, 1e38, -1.0], F), size=img.shape)
        img[...] = np.where(rng.random(img.shape) < 0.3, bad, img)
    rect = (w - 16, h - 8)
    got, want, _ = _case(ctx, demo, w, h, _views(demo, w, h)["orbit"], rect=rect, images=(acc, mo), max_history=1 << 24)
    ctx.sync()
    for g, written in zip(got, (acc, mo)):
        assert pc.same_bits(g[rect[1]:], written[rect[1]:]) and pc.same_bits(g[:, rect[0]:], written[:, rect[0]:])
    assert np.all(got[0][:rect[1], :rect[0], 3] == 1)
    _same_or_nan(got, want, "non-finite images")


def test_error_codes(ctx, demo, env):
    lib = capi.load_library()
    good = capi.ReprojectParams(0.02, 0.9, 64, 0)
    assert lib.mi3pt_reproject(None, ctypes.byref(good)) == 1
    w, h = SIZES[1]
    _configure(ctx, demo, env, w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, _uniforms(demo, w, h).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())

    def code(fn):
        with pytest.raises(capi.Mi3ptError) as e:
            fn()
        return e.value.code

    # the feature images: none since the resize, some, all but from different views
    assert code(ctx.reproject) == 4
    ctx.render_aovs((1 << capi.AOV_POSITION) | (1 << capi.AOV_ALBEDO))
    assert code(ctx.reproject) == 4
    ctx.set_uniforms(capi.PASS_RAYTRACE, _uniforms(demo, w, h, _views(demo, w, h)["orbit"]).tobytes())
    ctx.render_aovs((1 << capi.AOV_NORMAL) | (1 << capi.AOV_IDS))
    assert code(ctx.reproject) == 4
    ctx.render_aovs(capi.AOV_ALL)
    ctx.reproject()
    # the arguments
    assert lib.mi3pt_reproject(ctx.handle, None) == 1
    for bad in (dict(plane_tolerance=-1.0), dict(plane_tolerance=float("nan")), dict(plane_tolerance=float("inf")),
                dict(normal_cos_min=1.5), dict(normal_cos_min=-1.5), dict(normal_cos_min=float("nan")),
                dict(max_history=0), dict(max_history=(1 << 24) + 1), dict(flags=1)):
        assert code(lambda: ctx.reproject(**bad)) == 1, bad
    ctx.reproject(plane_tolerance=0.0, normal_cos_min=-1.0, max_history=1 << 24)
    # another resolution in the new view
    u = pc.rt_uniforms(demo, w, h, bounces=4, res=(w - 1, h))
    ctx.set_uniforms(capi.PASS_RAYTRACE, u.tobytes())
    assert code(ctx.reproject) == 4
    ctx.set_uniforms(capi.PASS_RAYTRACE, _uniforms(demo, w, h).tobytes())
    ctx.reproject()
    # the mode and the image
    ctx.set_mean_by_count(False)
    assert code(ctx.reproject) == 4
    ctx.set_mean_by_count(True)
    ctx.set_moments(False)
    assert code(ctx.reproject) == 4
    # before resize; a rank of a tile split; a device group
    with capi.Context(0) as c:
        c.set_moments(True)
        c.set_mean_by_count(True)
        assert code(c.reproject) == 4
        c.set_tile(0, 2, 8)
        pc.upload_scene(c, demo, env)
        c.resize(w, h)
        c.set_uniforms(capi.PASS_RAYTRACE, _uniforms(demo, w, h).tobytes())
        c.render_aovs(capi.AOV_ALL)
        assert code(c.reproject) == 4
    with capi.Context(devices=[0, 0]) as g:
        g.set_moments(True)
        g.set_mean_by_count(True)
        pc.upload_scene(g, demo, env)
        g.resize(w, h)
        g.set_uniforms(capi.PASS_RAYTRACE, _uniforms(demo, w, h).tobytes())
        g.render_aovs(capi.AOV_ALL)
        assert code(g.reproject) == 4


def test_the_pass_is_timed(ctx, demo, env):
    w, h = SIZES[0]
    _configure(ctx, demo, env, w, h)
    ctx.enable_timing(True)
    try:
        with pytest.raises(capi.Mi3ptError) as e:
            ctx.pass_time_us(capi.PASS_REPROJECT)
        assert e.value.code == 4
        _case(ctx, demo, w, h, _views(demo, w, h)["orbit"])
        assert ctx.pass_time_us(capi.PASS_REPROJECT) > 0 and ctx.pass_time_us(capi.PASS_AOV) > 0
    finally:
        ctx.enable_timing(False)
