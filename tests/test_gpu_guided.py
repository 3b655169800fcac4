"""The feature-guided a-trous de-noise (mi3pt_denoise_guided) on the GPU against tests/guided_reference.py: every comparison is bit for
bit (ptcommon.same_bits) -- no tolerance anywhere.  The features are the device's own read_aov of the demo scene (tests/test_gpu_aov.py
pins those to the oracle); unless said otherwise the accumulation is written with write_texture: seeded random values in [0, 4), alpha
included.  The conditions that keep a case from passing vacuously (taps rejected by the hit rule, weights on both sides of 0.5) are
asserted on the reference's statistics, never on the device's output."""
import ctypes
import os

import numpy as np
import pytest

import guided_reference as gr
import moments_edge_cases as ec
import ptcommon as pc
from mi3pt_host import capi

pytestmark = pytest.mark.gpu

NAMES = capi.AOV_NAMES
# sigma_color 4: with texels uniform in [0, 4) the squared colour distance of two texels is 8 on average, so exp(-d / 16) falls on
# both sides of 0.5 (chosen on the CPU with the oracle's features: 18 - 28 % below 0.5 at 64 x 64 and 100 x 52, levels 1 .. 5)
ALL_ON = (4.0, 0.35, 0.1, 0.05)
_features = {}
_references = {}


def _prepare(ctx, demo, env, w, h):
    """demo scene, whole image, the four feature images rendered; returns them (read back once per size)"""
    ctx.set_kernel_variant(0)
    ctx.set_tile(0, 1, 8)
    pc.upload_scene(ctx, demo, env)
    ctx.resize(w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h).tobytes())
    ctx.render_aovs(capi.AOV_ALL)
    if (w, h) not in _features:
        _features[(w, h)] = {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}
    return _features[(w, h)]


def _random_accum(w, h, seed=20261018):
    return (np.random.default_rng(seed).random((h, w, 4), dtype=np.float32) * np.float32(4)).astype(np.float32)


def _reference(orc, feat, accum, levels, sigmas, key=None):
    if key is not None and key in _references:
        return _references[key]
    out = gr.guided(orc, accum, feat["normal"], feat["position"], feat["albedo"], feat["ids"], levels, *sigmas)
    if key is not None:
        _references[key] = out
    return out


def _assert_not_vacuous(stats, what):
    print(f"{what}: {stats}")
    assert stats["rejected"] >= 0.02, f"{what}: the hit rule rejects {stats['rejected']:.3f} of the in-image taps"
    assert stats["below"] >= 0.10 and stats["above"] >= 0.10, f"{what}: counted off-centre taps below / above 0.5: {stats['below']:.3f} / {stats['above']:.3f}"


def _run(ctx, orc, demo, env, w, h, levels, sigmas):
    feat = _prepare(ctx, demo, env, w, h)
    accum = _random_accum(w, h)
    ctx.write_texture(capi.TEX_ACCUMULATION, accum)
    want, stats = _reference(orc, feat, accum, levels, sigmas, key=(w, h, levels, sigmas))
    ctx.denoise_guided(levels, *sigmas)
    got = ctx.read_guided()
    what = f"{w}x{h} levels {levels} sigmas {sigmas}"
    if w >= 64 and all(s > 0 for s in sigmas):
        _assert_not_vacuous(stats, what)
    assert got.shape == (h, w, 4) and got.dtype == np.float32
    assert pc.same_bits(got, want), what + ": " + pc.describe_diff(got, want)
    return got, want, stats


# 1 x 1 and 3 x 2: every off-centre tap is outside the image; 16 x 17 and 17 x 16: one texel past a block; 100 x 52: ragged; 33 x 33 and
# 64 x 64 at five levels: taps at +-32 reach across most of the image, stride classes of one or two texels; 264 x 260 = 16 * 16 + 8 by
# 16 * 16 + 4: every level has more than one 16 x 16 tile per stride class in both axes (five at stride 4, three at 8, two at 16), so
# blocks with u0, v0 > 0 and halos that cross two tiles of a class run, and at stride 16 the classes 8 .. 15 (4 .. 15 in y) are one
# texel shorter: their second tile finds no texel of theirs.  Four levels beside five tell stride 16 from stride 8
# (tests/test_guided_reference.py states the tile counts and the reference's statistics at this size without a device)
SIZES = [(1, 1, 3), (3, 2, 3), (16, 17, 3), (17, 16, 3), (100, 52, 3), (33, 33, 5), (64, 64, 5), (264, 260, 4), (264, 260, 5)]


@pytest.mark.parametrize("w,h,levels", SIZES, ids=[f"{w}x{h}-{n}-levels" for w, h, n in SIZES])
def test_sizes(gpu_ctx, orc, demo, env, w, h, levels):
    got, want, stats = _run(gpu_ctx, orc, demo, env, w, h, levels, ALL_ON)
    if (w, h) == (1, 1):
        assert stats["taps"] == levels                     # the centre tap alone, once per level


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_every_level_count(gpu_ctx, orc, demo, env, levels):
    _run(gpu_ctx, orc, demo, env, 64, 64, levels, ALL_ON)


SIGMA_CASES = [("color", (4.0, 0.0, 0.0, 0.0)), ("normal", (0.0, 0.35, 0.0, 0.0)), ("albedo", (0.0, 0.0, 0.1, 0.0)),
               ("plane", (0.0, 0.0, 0.0, 0.05)), ("all-on", ALL_ON), ("all-zero", (0.0, 0.0, 0.0, 0.0))]


@pytest.mark.parametrize("name,sigmas", SIGMA_CASES, ids=[c[0] for c in SIGMA_CASES])
def test_each_sigma_alone(gpu_ctx, orc, demo, env, name, sigmas):
    got, want, stats = _run(gpu_ctx, orc, demo, env, 100, 52, 3, sigmas)
    if name == "all-zero":
        assert stats["below"] == 0.0 and stats["above"] == 1.0       # every counted tap weighs h[dx] * h[dy]
    else:
        assert stats["below"] > 0.0, f"sigma_{name} alone changes no weight of this case"


EDGE_SIZE = (100, 52)
# sigma_color 0.18: a squared colour distance of 3 weighs exp(-92.6), a subnormal (tests/moments_edge_cases.py: subnormal_patches); the
# term tightens by 4 per level, so the plain texels around a patch never reach into it
SUBNORMAL_SIGMAS, SUBNORMAL_LEVELS = (ec.SUBNORMAL_SIGMA_PLAIN, 0.35, 0.1, 0.05), 3
NON_FINITE_AT = [(5, 9), (5, 60), (26, 35), (45, 9), (45, 85), (26, 90)]


def subnormal_accum(w, h):
    accum = _random_accum(w, h)
    ec.subnormal_patches(accum)
    return accum


def non_finite_accum(w, h):
    """the finite means of the catalogue six texels apart (0, -0, subnormals, the ends of binary16, 1e19 whose square is finite and 3e38
    whose square is not), and the six non-finite ones once each: every one of those spreads over 5 x 5 texels per level"""
    accum = _random_accum(w, h)
    ec.overlay(accum, np.zeros((h, w, 4), np.float32), 4, True, only=lambda name: name.startswith("mean="), pitch=6)
    ec.non_finite_means(accum, NON_FINITE_AT)
    return accum


def _run_written(ctx, orc, demo, env, accum, levels, sigmas, what):
    """_run with the accumulation given; the comparison is ptcommon.same_bits_or_nan"""
    h, w = accum.shape[:2]
    feat = _prepare(ctx, demo, env, w, h)
    ctx.write_texture(capi.TEX_ACCUMULATION, accum)
    want, stats = _reference(orc, feat, accum, levels, sigmas)
    ctx.denoise_guided(levels, *sigmas)
    got = ctx.read_guided()
    assert pc.same_bits_or_nan(got, want), what + ": " + pc.describe_diff(got, want)
    return got, want, stats


def test_subnormal_weights(gpu_ctx, orc, demo, env):
    """weights in the fp32 subnormal range: a build that flushes them, or an exp that cuts off early, gives 0 where the reference has 6e-42
    (tests/test_moments_edge_cases.py shows that on the reference alone)"""
    w, h = EDGE_SIZE
    _, want, stats = _run_written(gpu_ctx, orc, demo, env, subnormal_accum(w, h), SUBNORMAL_LEVELS, SUBNORMAL_SIGMAS, "subnormal weights")
    print(f"subnormal weights: {stats['subnormal']} counted taps; {stats}")
    assert stats["subnormal"] > 0 and np.isfinite(want).all()


def test_non_finite_colours(gpu_ctx, orc, demo, env):
    w, h = EDGE_SIZE
    _, want, stats = _run_written(gpu_ctx, orc, demo, env, non_finite_accum(w, h), 2, ALL_ON, "non-finite colours")
    share = float(np.isnan(want).any(axis=-1).mean())
    print(f"non-finite colours: a NaN in {share:.3f} of the texels; {stats['subnormal']} counted taps with a subnormal weight")
    assert 0 < share <= 0.5


def _sample_frames(ctx, demo, w, h, first, count):
    for f in range(first, first + count):
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=f, bounces=4).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, f).tobytes())
        ctx.submit(capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE)


def test_a_mean_of_four_device_frames_and_nothing_else_changes(gpu_ctx, orc, demo, env):
    """Four queued sample frames are in the mean the filter sees; two runs are byte-identical; the accumulation and the four feature
    images are byte-identical before and after; four more frames give the accumulation of a run that never called the filter."""
    ctx = gpu_ctx
    w = h = 64
    sigmas = (0.5, 0.35, 0.1, 0.05)                   # (half the hosts' 2 / sqrt(4 frames): 16 % of the weights below 0.5 instead of 10.3 %)

    def job(filtered):
        _prepare(ctx, demo, env, w, h)
        ctx.set_pipelining(True)
        ctx.reset_counters()
        _sample_frames(ctx, demo, w, h, 1, 4)
        out = None
        if filtered:
            ctx.denoise_guided(3, *sigmas)            # (the frames are still queued here: the call launches them)
            first = ctx.read_guided()
            before = ctx.read_texture(capi.TEX_ACCUMULATION)
            feat_before = {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}
            ctx.denoise_guided(3, *sigmas)
            second = ctx.read_guided()
            after = ctx.read_texture(capi.TEX_ACCUMULATION)
            feat_after = {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}
            out = (first, second, before, after, feat_before, feat_after)
        _sample_frames(ctx, demo, w, h, 5, 4)
        return ctx.read_texture(capi.TEX_ACCUMULATION), ctx.counters(), out

    plain_acc, plain_cnt, _ = job(False)
    acc, cnt, (first, second, before, after, feat_before, feat_after) = job(True)
    assert first.tobytes() == second.tobytes()
    assert before.tobytes() == after.tobytes()
    for name in NAMES:
        assert feat_before[name].tobytes() == feat_after[name].tobytes(), name
    assert before[..., :3].max() > 0.0 and not pc.same_bits(first, before)
    want, stats = _reference(orc, feat_before, before, 3, sigmas)
    _assert_not_vacuous(stats, "mean of four frames")
    assert pc.same_bits(first, want), pc.describe_diff(first, want)
    assert acc.tobytes() == plain_acc.tobytes(), pc.describe_diff(acc, plain_acc)
    for k in pc.PATH_COUNTERS:
        assert cnt[k] == plain_cnt[k], k


def test_present_draws_the_canvas_from_the_filtered_image(gpu_ctx, orc, demo, env):
    """MI3PT_GUIDED_PRESENT: float and RGBA8 canvas equal the oracle's fullscreen pass on the REFERENCE filtered image with `denoise`
    taken as 0 (the pass's own uniforms say 1), tone mapping and scaling as they are; without the flag the canvas is untouched."""
    ctx = gpu_ctx
    w, h = 100, 52
    feat = _prepare(ctx, demo, env, w, h)
    accum = _random_accum(w, h)
    ctx.write_texture(capi.TEX_ACCUMULATION, accum)
    want, _ = _reference(orc, feat, accum, 3, ALL_ON, key=(w, h, 3, ALL_ON))
    ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(w, h, 1.0, denoise=1, tonemapping=1).tobytes())
    ctx.denoise_guided(3, *ALL_ON)
    assert not ctx.read_canvas_rgba8().any()                          # (a fresh canvas: nothing drawn without the flag)
    ctx.denoise_guided(3, *ALL_ON, flags=capi.GUIDED_PRESENT)
    want_f, want_8 = orc.fullscreen(pc.fs_uniforms(w, h, 1.0, denoise=0, tonemapping=1).tobytes(), want)
    got_f, got_8 = ctx.read_texture(capi.TEX_CANVAS), ctx.read_canvas_rgba8()
    assert pc.same_bits(got_f, want_f), pc.describe_diff(got_f, want_f)
    assert np.array_equal(got_8.reshape(want_8.shape), want_8)
    plain_f, _ = orc.fullscreen(pc.fs_uniforms(w, h, 1.0, denoise=0, tonemapping=1).tobytes(), accum)
    assert not pc.same_bits(want_f, plain_f)
    # the next fullscreen submit shows the running mean again, with the pass's own de-noiser
    ctx.submit(capi.SUBMIT_FULLSCREEN)
    mean_f, _ = orc.fullscreen(pc.fs_uniforms(w, h, 1.0, denoise=1, tonemapping=1).tobytes(), accum)
    got_f = ctx.read_texture(capi.TEX_CANVAS)
    assert pc.same_bits(got_f, mean_f), pc.describe_diff(got_f, mean_f)


def test_states_and_errors(gpu_ctx, orc, demo, env):
    w = h = 16

    def code(fn, *a, **kw):
        with pytest.raises(capi.Mi3ptError) as e:
            fn(*a, **kw)
        return e.value.code

    with capi.Context(0) as ctx:
        pc.upload_scene(ctx, demo, env)
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h).tobytes())
        assert code(ctx.denoise_guided) == 4                             # before resize
        assert code(ctx.read_guided) == 4
        assert code(ctx.guided_device_ptr) == 4
        ctx.resize(w, h)
        assert code(ctx.denoise_guided) == 4                             # no feature image yet
        for k in range(capi.AOV_COUNT):                                   # any one of the four missing
            ctx.resize(w, h)
            ctx.render_aovs(capi.AOV_ALL & ~(1 << k))
            assert code(ctx.denoise_guided) == 4, NAMES[k]
        ctx.render_aovs(capi.AOV_ALL)
        assert code(ctx.read_guided) == 4                                # before the first filter
        assert code(ctx.guided_device_ptr) == 4
        assert code(ctx.pass_time_us, capi.PASS_GUIDED) == 4             # nothing timed
        assert code(ctx.set_uniforms, capi.PASS_GUIDED, b"\0" * 16) == 1  # no uniform block of its own
        for levels in (0, 6, -1):
            assert code(ctx.denoise_guided, levels) == 1
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            for name in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_plane"):
                assert code(ctx.denoise_guided, **{name: bad}) == 1, (name, bad)
        assert code(ctx.denoise_guided, flags=2) == 1
        assert code(ctx.denoise_guided, flags=0x80000001) == 1
        assert ctx.lib.mi3pt_denoise_guided(ctx.handle, None) == 1
        assert ctx.lib.mi3pt_denoise_guided(None, ctypes.byref(capi.GuidedParams(3, 1.0, 0.35, 0.1, 0.05, 0))) == 1
        ctx.denoise_guided(1, -0.0, 0.0, 0.0, 0.0)                       # -0 is 0: the term is off
        out = np.empty((h, w, 4), np.float32)
        ptr = out.ctypes.data_as(ctypes.c_void_p)
        assert ctx.lib.mi3pt_read_guided(ctx.handle, ptr, out.nbytes - 16) == 1      # wrong byte count
        assert ctx.lib.mi3pt_read_guided(ctx.handle, ptr, out.nbytes + 16) == 1
        assert ctx.lib.mi3pt_read_guided(ctx.handle, None, out.nbytes) == 1
        assert ctx.lib.mi3pt_guided_device_ptr(ctx.handle, None, None) == 1
        assert ctx.lib.mi3pt_read_guided(ctx.handle, ptr, out.nbytes) == 0
        ctx.resize(w, h)
        assert code(ctx.read_guided) == 4                                # a resize frees the image
        assert code(ctx.guided_device_ptr) == 4
        # a rank of a tile split: refused (the halo exchange is not built)
        ctx.set_tile(0, 2, 8)
        ctx.resize(w, h)
        ctx.render_aovs(capi.AOV_ALL)
        assert code(ctx.denoise_guided) == 4
        ctx.set_tile(0, 1, 8)
        ctx.resize(w, h)
        # the context still filters the right bits afterwards
        ctx.render_aovs(capi.AOV_ALL)
        feat = {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}
        accum = _random_accum(w, h, 3)
        ctx.write_texture(capi.TEX_ACCUMULATION, accum)
        ctx.denoise_guided(2, *ALL_ON)
        want, _ = _reference(orc, feat, accum, 2, ALL_ON)
        assert pc.same_bits(ctx.read_guided(), want)
    with capi.Context(devices=[0, 0]) as g:                              # a device group: refused
        pc.upload_scene(g, demo, env)
        g.resize(w, h)
        g.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h).tobytes())
        g.render_aovs(capi.AOV_ALL)
        assert code(g.denoise_guided) == 4
        assert code(g.read_guided) == 4
        assert code(g.guided_device_ptr) == 4


def test_device_pointer_and_pass_time(gpu_ctx, orc, demo, env):
    """mi3pt_guided_device_ptr holds the bytes of read_guided (copied back with hipMemcpy, as tests/test_gpu_aov.py reads its device
    pointers); with timing on the pass time is positive."""
    ctx = gpu_ctx
    w, h = 100, 52
    ctx.enable_timing(True)
    try:
        got, _, _ = _run(ctx, orc, demo, env, w, h, 3, ALL_ON)
        ctx.sync()
        assert ctx.pass_time_us(capi.PASS_GUIDED) > 0.0
    finally:
        ctx.enable_timing(False)
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ptr, nbytes = ctx.guided_device_ptr()
    assert ptr and nbytes == w * h * 16
    host = np.empty((h, w, 4), np.float32)
    assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ptr, nbytes, 2) == 0          # hipMemcpyDeviceToHost
    assert host.tobytes() == got.tobytes()


def test_renderer_renders_the_features_itself_and_scales_sigma_color(built, orc, demo, env):
    """Renderer.denoiseGuided(): the feature images are rendered when none are current (first call, new camera) and kept otherwise;
    sigmaColor None = 2 / sqrt(frames in the mean)."""
    from mi3pt_host import RaytracingCamera, RaytracingScene, Renderer
    r = Renderer.create()
    try:
        r.frames = 4
        r.scalingFactor = 1
        r.presentEveryFrame = False
        r.setUniforms("raytrace", {"maxBounces": 4, "envMapIntensity": 1.0})
        r.setUniforms("accumulate", {"enabled": 1})
        r.resize(64, 64)
        scene = RaytracingScene(demo, env)
        scene.needsUpdate = True
        cam = RaytracingCamera(45.0)
        for _ in range(4):
            r.render(scene, cam)
        assert r.frame == 5
        calls = []
        render_aovs = r.ctx.render_aovs
        r.ctx.render_aovs = lambda mask=capi.AOV_ALL: (calls.append(mask), render_aovs(mask))[1]
        r.denoiseGuided()
        got = r.readGuided()
        assert calls == [capi.AOV_ALL]
        feat = {name: r.readAov(name) for name in NAMES}
        want, _ = _reference(orc, feat, r.readAccumulation(), 3, (2.0 / np.sqrt(4.0), 0.35, 0.1, 0.05))
        assert pc.same_bits(got, want), pc.describe_diff(got, want)
        r.denoiseGuided(levels=1, sigmaColor=0.5)
        assert calls == [capi.AOV_ALL]                                    # still current
        cam2 = RaytracingCamera(45.0, position=(0.5, 1.2, 4.0))
        r.update(scene, cam2)
        r.denoiseGuided(levels=1, sigmaColor=0.5)
        assert calls == [capi.AOV_ALL, capi.AOV_ALL]                      # another camera: rendered again
        feat2 = {name: r.readAov(name) for name in NAMES}
        assert feat2["position"].tobytes() != feat["position"].tobytes()
        want2, _ = _reference(orc, feat2, r.readAccumulation(), 1, (0.5, 0.35, 0.1, 0.05))
        assert pc.same_bits(r.readGuided(), want2)
    finally:
        r.destroy()
