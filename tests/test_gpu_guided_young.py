"""MI3PT_GUIDED_YOUNG on the GPU (csrc/pt_guided.hip: k_guided_variance_young) against tests/guided_young_reference.py: the colour image
(read_guided) and the last level's variance (read_guided_variance) are compared bit for bit (ptcommon.same_bits) -- no tolerance
anywhere.  Modelled on tests/test_gpu_guided_variance.py: the features are the device's own read_aov of the demo scene, the accumulation
is written with write_texture (seeded, [0, 4)) and the moments with write_moments.  The kernel works on 32 x 8 tiles with a halo of 3; a
block without a young texel takes the light path (the 3 x 3 from global memory), any other stages its 38 x 14 records.  The conditions
that keep a case from passing vacuously are asserted on the reference's statistics, never on the device's output."""
import ctypes

import numpy as np
import pytest

import guided_young_reference as yr
import moments_edge_cases as ec
import moments_reference as mr
import ptcommon as pc
import reproject_reference as rr
from mi3pt_host import capi

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = capi.AOV_NAMES
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
TEX = capi.TEX_ACCUMULATION
SIGMAS = (2.0, 0.35, 0.1, 0.05)
VARIANCE = capi.GUIDED_VARIANCE
FLAGS = capi.GUIDED_VARIANCE | capi.GUIDED_YOUNG
TILE_W, TILE_H, HALO = 32, 8, 3
BELOW_FOUR = np.nextafter(F(4), F(0))
_features = {}
_references = {}


@pytest.fixture(scope="module")
def ctx(built):
    c = capi.Context(0)
    c.set_moments(True)
    yield c
    c.set_storage(capi.STORAGE_F32)
    c.close()


def _prepare(ctx, demo, env, w, h):
    ctx.set_kernel_variant(0)
    ctx.set_tile(0, 1, 8)
    ctx.set_storage(capi.STORAGE_F32)
    ctx.set_mean_by_count(False)
    ctx.set_moments(True)
    pc.upload_scene(ctx, demo, env)
    ctx.resize(w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h).tobytes())
    ctx.render_aovs(capi.AOV_ALL)
    if (w, h) not in _features:
        _features[(w, h)] = {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}
    return _features[(w, h)]


def _random_accum(w, h, seed=20261018):
    return (np.random.default_rng(seed).random((h, w, 4), dtype=F) * F(4)).astype(F)


def _moments(w, h, n, seed=20261019, scale=24.0):
    """seeded M2 in [0, 24) per channel where the count holds a variance (n >= 2), 0 elsewhere; n: one count or an (h, w) image"""
    m = (np.random.default_rng(seed).random((h, w, 4), dtype=F) * F(scale)).astype(F)
    m[..., 3] = n
    m[..., :3] = np.where(m[..., 3:] >= 2, m[..., :3], 0)
    return m


def _mixed_counts(w, h, seed=20261020):
    counts = np.array([0, 1, 1.5, 2, 3, BELOW_FOUR, 4, 64], F)
    return counts[np.random.default_rng(seed).integers(0, len(counts), (h, w))]


def _reference(orc, feat, accum, moments, levels, sigmas, key=None, fn=None):
    fn = fn or yr.guided_variance_young
    if key is not None and (fn.__name__, key) in _references:
        return _references[(fn.__name__, key)]
    out = fn(orc, accum, moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"], levels, *sigmas)
    if key is not None:
        _references[(fn.__name__, key)] = out
    return out


def _compare(ctx, want, want_var, what, w, h, same=pc.same_bits):
    got, got_var = ctx.read_guided(), ctx.read_guided_variance()
    assert got.shape == (h, w, 4) and got.dtype == np.float32 and got_var.shape == (h, w) and got_var.dtype == np.float32
    assert same(got, want), what + ": colour: " + pc.describe_diff(got, want)
    assert same(got_var, want_var), what + ": variance: " + pc.describe_diff(got_var, want_var)
    return got, got_var


def _run(ctx, orc, demo, env, w, h, levels, sigmas, moments, key_extra, accum=None, flags=FLAGS, same=pc.same_bits):
    feat = _prepare(ctx, demo, env, w, h)
    accum = _random_accum(w, h) if accum is None else accum
    ctx.write_texture(TEX, accum)
    ctx.write_moments(moments)
    want, want_var, stats = _reference(orc, feat, accum, moments, levels, sigmas, key=(w, h, levels, sigmas, key_extra))
    ctx.denoise_guided(levels, *sigmas, flags=flags)
    what = f"{w}x{h} levels {levels} sigmas {sigmas} {key_extra}"
    print(f"{what}: {stats}")
    got, got_var = _compare(ctx, want, want_var, what, w, h, same)
    return got, got_var, want, want_var, stats


def _levels(w):
    return 2 if w > 200 else 3           # (the var_0 kernel is what is new: two levels on top of it at the large size keep the case short)


# 1 x 1: N = 1, var_0 = 0; 3 x 2 and 8 x 8: the window is larger than the image; 33 x 9: one texel past the 32 x 8 tile in each axis;
# 38 x 14: tile + halo exactly; 35 x 11: tile + one side of the halo; 100 x 52: ragged; 264 x 260: several tiles in both axes
SIZES = [(1, 1), (3, 2), (8, 8), (33, 9), (38, 14), (35, 11), (100, 52), (264, 260)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes(ctx, orc, demo, env, w, h):
    """the seeded mix of counts, except at 1 x 1: one sample"""
    n = F(1) if (w, h) == (1, 1) else _mixed_counts(w, h)
    *_, want_var, stats = _run(ctx, orc, demo, env, w, h, _levels(w), SIGMAS, _moments(w, h, n), "mix")
    if (w, h) == (1, 1):
        assert stats["young"] == 1.0 and stats["young_lone"] == 1.0 and want_var[0, 0] == 0
    else:
        assert 0 < stats["young"] < 1 and stats["young_taps"] > 0            # (six of the eight counts are young: 0.75 at the large sizes)


PATTERN_SIZES = [(100, 52), (264, 260)]


def _tile_of_interest(w, h):
    """a tile with whole neighbours on every side: (x0, y0) of tile (1, 1)"""
    assert w >= 3 * TILE_W and h >= 3 * TILE_H
    return TILE_W, TILE_H


@pytest.mark.parametrize("w,h", PATTERN_SIZES, ids=[f"{w}x{h}" for w, h in PATTERN_SIZES])
def test_no_young_texel_gives_the_bits_of_the_variance_mode(ctx, orc, demo, env, w, h):
    """n = 4 everywhere: every block takes the light path, and the bits are those of the call without the flag on the same images"""
    moments = _moments(w, h, F(4))
    got, got_var, _, _, stats = _run(ctx, orc, demo, env, w, h, _levels(w), SIGMAS, moments, "n=4")
    assert stats["young"] == 0.0
    feat = _features[(w, h)]
    plain, plain_var, _ = _reference(orc, feat, _random_accum(w, h), moments, _levels(w), SIGMAS, key=(w, h, "n=4"), fn=mr.guided_variance)
    ctx.denoise_guided(_levels(w), *SIGMAS, flags=VARIANCE)
    _compare(ctx, plain, plain_var, "without the flag", w, h)
    assert pc.same_bits(got, plain) and pc.same_bits(got_var, plain_var)


@pytest.mark.parametrize("w,h", PATTERN_SIZES, ids=[f"{w}x{h}" for w, h in PATTERN_SIZES])
def test_one_sample_everywhere(ctx, orc, demo, env, w, h):
    """n = 1, M2 = 0: every block stages; var_0 is the spread of the neighbours' means.  Measured on the CPU with the oracle's features and
    the default sigmas, 7 x 7: rejected / below / above = 0.033 / 0.037 / 0.963 at 100 x 52 (0.015 / 0.009 / 0.991 at 264 x 260: most of
    that image is one plane, and no share is asserted there)"""
    *_, want_var, stats = _run(ctx, orc, demo, env, w, h, _levels(w), SIGMAS, _moments(w, h, F(1)), "n=1")
    assert stats["young"] == 1.0 and (want_var > 0).mean() > 0.9
    if (w, h) == (100, 52):
        assert stats["young_rejected"] >= 0.02 and stats["young_below"] >= 0.02 and stats["young_above"] >= 0.10


@pytest.mark.parametrize("w,h", PATTERN_SIZES, ids=[f"{w}x{h}" for w, h in PATTERN_SIZES])
def test_one_young_texel_at_each_corner_of_one_tile(ctx, orc, demo, env, w, h):
    """the tile stages, its eight neighbours take the light path -- and leave the young corners out of their 3 x 3 across the seams"""
    x0, y0 = _tile_of_interest(w, h)
    n = np.full((h, w), 4, F)
    corners = [(y0, x0), (y0, x0 + TILE_W - 1), (y0 + TILE_H - 1, x0), (y0 + TILE_H - 1, x0 + TILE_W - 1)]
    for k, (y, x) in enumerate(corners):
        n[y, x] = (1, 2, 3, BELOW_FOUR)[k]
    moments = _moments(w, h, n)
    *_, want_var, stats = _run(ctx, orc, demo, env, w, h, _levels(w), SIGMAS, moments, "corners")
    assert stats["young"] == 4 / (w * h) and stats["young_taps"] > 0
    # the case is not the flag-less one: the young corners change var_0 in their own tile and in the neighbours
    feat = _features[(w, h)]
    var0, _ = yr.initial_variance_young(orc, _random_accum(w, h), moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"], *SIGMAS[1:])
    differs = var0 != mr.initial_variance(moments, feat["ids"][..., 2])
    assert differs[y0:y0 + TILE_H, x0:x0 + TILE_W].any() and differs[y0 - 1, :].any() and differs[:, x0 - 1].any() and differs[:, x0 + TILE_W].any()


@pytest.mark.parametrize("w,h", PATTERN_SIZES, ids=[f"{w}x{h}" for w, h in PATTERN_SIZES])
def test_young_texels_in_the_first_row_and_column_of_the_next_tile(ctx, orc, demo, env, w, h):
    """young texels only in column 64 (rows 0 .. 15) and in row 16 (columns 0 .. 63): the tiles left of the column and below the row hold
    none and take the light path, whose last column / row must leave the young taps across the seam out"""
    n = np.full((h, w), 64, F)
    n[0:2 * TILE_H, 2 * TILE_W] = 1
    n[2 * TILE_H, 0:2 * TILE_W] = 2
    moments = _moments(w, h, n)
    _run(ctx, orc, demo, env, w, h, _levels(w), SIGMAS, moments, "seam")
    feat = _features[(w, h)]
    var0, _ = yr.initial_variance_young(orc, _random_accum(w, h), moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"], *SIGMAS[1:])
    differs = var0 != mr.initial_variance(moments, feat["ids"][..., 2])
    assert differs[0:2 * TILE_H, 2 * TILE_W - 1].any() and differs[2 * TILE_H - 1, 0:2 * TILE_W].any()      # light-path texels at the seam
    assert not (n[0:2 * TILE_H, 0:2 * TILE_W] < 4).any()


SIGMA_CASES = [("normal", (2.0, 0.35, 0.0, 0.0)), ("albedo", (2.0, 0.0, 0.1, 0.0)), ("plane", (2.0, 0.0, 0.0, 0.05)),
               ("color", (2.0, 0.0, 0.0, 0.0)), ("all-zero", (0.0, 0.0, 0.0, 0.0))]


@pytest.mark.parametrize("name,sigmas", SIGMA_CASES, ids=[c[0] for c in SIGMA_CASES])
def test_each_sigma_alone(ctx, orc, demo, env, name, sigmas):
    """no feature sigma ("color", "all-zero"): every w is 1 and var_0 is the plain pooled variance"""
    w, h = 100, 52
    *_, stats = _run(ctx, orc, demo, env, w, h, 3, sigmas, _moments(w, h, _mixed_counts(w, h)), "mix")
    if name in ("color", "all-zero"):
        assert stats["young_below"] == 0.0 and stats["young_above"] == 1.0
    else:
        assert stats["young_below"] > 0.0, f"sigma_{name} alone changes no weight of this case"


TIGHT = (2.0, 0.02, 0.1, 1e-7)


def test_tight_sigmas(ctx, orc, demo, env):
    """sigma_normal 0.02, sigma_plane 1e-7: the demo scene is mostly planes, whose normals agree to the bit and whose points leave the
    centre's plane by the rounding of the hit point alone -- only a sigma_plane of that size weighs them down (at 1e-6 the share below
    0.5 is still 0.039, at 3e-7 0.057).  Measured on the CPU with the oracle's features at 100 x 52, n = 1: below / above = 0.312 / 0.688,
    0.011 of the young texels pool fewer than two samples"""
    w, h = 100, 52
    *_, stats = _run(ctx, orc, demo, env, w, h, 3, TIGHT, _moments(w, h, F(1)), "n=1")
    assert stats["young_below"] >= 0.10 and stats["young_above"] >= 0.10


def _sample(ctx, demo, w, h, first, count, view=None):
    kw = {} if view is None else {"position": view[0], "direction": view[1]}
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=first, bounces=4, **kw).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, first).tobytes())
    ctx.submit_frames(MASK, count)


def _filter_what_the_device_holds(ctx, orc, w, h, what, queued=False):
    """the filter with the flag on the device's own images, against the reference on their read-back"""
    if queued:
        ctx.denoise_guided(3, *SIGMAS, flags=FLAGS)               # (the frames are still queued here: the call launches them)
    accum, moments = ctx.read_texture(TEX), ctx.read_moments()
    feat = {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}
    if not queued:
        ctx.denoise_guided(3, *SIGMAS, flags=FLAGS)
    want, want_var, stats = _reference(orc, feat, accum, moments, 3, SIGMAS)
    print(f"{what}: {stats}")
    _compare(ctx, want, want_var, what, w, h)
    assert ctx.read_texture(TEX).tobytes() == accum.tobytes() and ctx.read_moments().tobytes() == moments.tobytes()
    return moments, stats


def test_one_frame_after_a_reset(ctx, orc, demo, env):
    """64 x 64, the mean by count, one frame, called with the frame still queued.  Measured on the CPU with the oracle's features, 7 x 7:
    rejected / below / above = 0.062 / 0.033 / 0.967"""
    w = h = 64
    _prepare(ctx, demo, env, w, h)
    ctx.set_mean_by_count(True)
    try:
        ctx.reset()
        _sample(ctx, demo, w, h, 2, 1)
        moments, stats = _filter_what_the_device_holds(ctx, orc, w, h, "one frame after a reset", queued=True)
        assert np.all(moments[..., 3] == 1) and stats["young"] == 1.0
        assert stats["young_rejected"] >= 0.02 and stats["young_below"] >= 0.02 and stats["young_above"] >= 0.10
    finally:
        ctx.set_mean_by_count(False)


def test_one_frame_after_a_reprojection(ctx, orc, demo, env):
    """64 x 64: 8 frames in view A, an 8 degree orbit, reproject, 1 frame of view B, the filter with the flag: carried texels (n = 9) and
    disoccluded ones (n = 1) side by side"""
    w = h = 64
    _prepare(ctx, demo, env, w, h)
    ctx.set_mean_by_count(True)
    try:
        ctx.reset()
        _sample(ctx, demo, w, h, 2, 8)
        view = rr.orbit(demo.camera["position"], demo.camera["target"], 8.0)
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=10, bounces=4, position=view[0], direction=view[1]).tobytes())
        ctx.reproject()
        ctx.render_aovs(capi.AOV_ALL)
        _sample(ctx, demo, w, h, 10, 1, view)
        moments, stats = _filter_what_the_device_holds(ctx, orc, w, h, "one frame after a reprojection")
        assert stats["young"] >= 0.02 and (moments[..., 3] >= 4).mean() > 0.5
    finally:
        ctx.set_mean_by_count(False)


def test_f16_storage_and_a_bound_image(ctx, orc, demo, env):
    w, h = 100, 52
    moments = _moments(w, h, _mixed_counts(w, h))
    feat = _prepare(ctx, demo, env, w, h)
    try:
        ctx.set_storage(capi.STORAGE_F16)
        ctx.resize(w, h)
        ctx.render_aovs(capi.AOV_ALL)
        _sample(ctx, demo, w, h, 1, 3)                       # three frames: the mean as the accumulate step stores it, every texel young
        accum, sampled = ctx.read_texture(TEX), ctx.read_moments()
        assert pc.same_bits(accum[..., :3], accum[..., :3].astype(np.float16).astype(F)) and np.all(sampled[..., 3] == 3)
        want, want_var, _ = _reference(orc, feat, accum, sampled, 3, SIGMAS)
        ctx.denoise_guided(3, *SIGMAS, flags=FLAGS)
        _compare(ctx, want, want_var, "F16 storage", w, h)
    finally:
        ctx.set_storage(capi.STORAGE_F32)
    # a caller-owned accumulation image
    _prepare(ctx, demo, env, w, h)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    accum = _random_accum(w, h, seed=7)
    bound, nbytes = ctypes.c_void_p(), h * w * 16
    assert hip.hipMalloc(ctypes.byref(bound), nbytes) == 0
    try:
        assert hip.hipMemcpy(bound, accum.ctypes.data_as(ctypes.c_void_p), nbytes, 1) == 0          # hipMemcpyHostToDevice
        ctx.bind_accumulation(bound.value, nbytes)
        try:
            ctx.write_moments(moments)
            assert ctx.read_texture(TEX).tobytes() == accum.tobytes()
            want, want_var, _ = _reference(orc, feat, accum, moments, 3, SIGMAS)
            ctx.denoise_guided(3, *SIGMAS, flags=FLAGS)
            _compare(ctx, want, want_var, "a bound image", w, h)
        finally:
            ctx.bind_accumulation(None, 0)
    finally:
        hip.hipFree(bound)


def test_present_draws_the_canvas_from_the_filtered_image(ctx, orc, demo, env):
    """The flag together with MI3PT_GUIDED_PRESENT: the canvas equals the oracle's fullscreen pass on the REFERENCE image, `denoise` 0"""
    w, h = 100, 52
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments = _random_accum(w, h), _moments(w, h, _mixed_counts(w, h))
    ctx.write_texture(TEX, accum)
    ctx.write_moments(moments)
    want, want_var, _ = _reference(orc, feat, accum, moments, 3, SIGMAS, key=(w, h, 3, SIGMAS, "mix"))
    ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(w, h, 1.0, denoise=1, tonemapping=1).tobytes())
    ctx.denoise_guided(3, *SIGMAS, flags=FLAGS | capi.GUIDED_PRESENT)
    want_f, want_8 = orc.fullscreen(pc.fs_uniforms(w, h, 1.0, denoise=0, tonemapping=1).tobytes(), want)
    got_f, got_8 = ctx.read_texture(capi.TEX_CANVAS), ctx.read_canvas_rgba8()
    assert pc.same_bits(got_f, want_f), pc.describe_diff(got_f, want_f)
    assert np.array_equal(got_8.reshape(want_8.shape), want_8)
    _compare(ctx, want, want_var, "with present", w, h)


def test_count_and_m2_catalogue(ctx, orc, demo, env):
    """NaN, negative and infinite M2 and n (moments_edge_cases.overlay) among young and settled texels: the bits of the reference, a NaN
    where it has one, no fault.  One level: the pool spreads a NaN over 7 x 7 texels before the levels do, and three quarters of this image
    are young -- measured on the CPU with the oracle's features, a NaN in 0.145 of the variance's texels after one level, 0.84 after two"""
    w, h = 100, 52
    accum, moments = _random_accum(w, h), _moments(w, h, _mixed_counts(w, h))
    ec.overlay(accum, moments, 3, False, only=lambda name: "mean" not in name, pitch=6)
    _, _, want, want_var, stats = _run(ctx, orc, demo, env, w, h, 1, SIGMAS, moments, "catalogue", accum=accum, same=pc.same_bits_or_nan)
    share = float(np.isnan(want_var).mean())
    print(f"count and M2 catalogue: a NaN in {share:.3f} of the variance's texels")
    assert 0 < share <= 0.5


def _code(fn, *a, **kw):
    with pytest.raises(capi.Mi3ptError) as e:
        fn(*a, **kw)
    return e.value


def test_refusals_and_a_call_without_the_flag_afterwards(ctx, orc, demo, env):
    w, h = 100, 52
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments = _random_accum(w, h), _moments(w, h, _mixed_counts(w, h))
    ctx.write_texture(TEX, accum)
    ctx.write_moments(moments)
    # the flag alone, with and without present: an invalid argument
    assert _code(ctx.denoise_guided, 3, *SIGMAS, flags=capi.GUIDED_YOUNG).code == 1
    assert _code(ctx.denoise_guided, 3, *SIGMAS, flags=capi.GUIDED_YOUNG | capi.GUIDED_PRESENT).code == 1
    assert _code(ctx.denoise_guided, 3, *SIGMAS, flags=FLAGS | 8).code == 1
    # a call with the flag, then one without it: the old bits
    ctx.denoise_guided(3, *SIGMAS, flags=FLAGS)
    ctx.denoise_guided(3, *SIGMAS, flags=VARIANCE)
    plain, plain_var, _ = _reference(orc, feat, accum, moments, 3, SIGMAS, key=(w, h, "mix"), fn=mr.guided_variance)
    _compare(ctx, plain, plain_var, "without the flag, afterwards", w, h)
    young, young_var, _ = _reference(orc, feat, accum, moments, 3, SIGMAS, key=(w, h, 3, SIGMAS, "mix"))
    assert not pc.same_bits(young_var, plain_var)
    # moments switched off: the wrong state
    ctx.set_moments(False)
    e = _code(ctx.denoise_guided, 3, *SIGMAS, flags=FLAGS)
    assert e.code == 4 and "mi3pt_set_moments" in e.message
    ctx.set_moments(True)
    # a rank of a tile split and a device group stay refused
    ctx.set_tile(0, 2, 8)
    ctx.resize(w, h)
    ctx.render_aovs(capi.AOV_ALL)
    assert _code(ctx.denoise_guided, 3, *SIGMAS, flags=FLAGS).code == 4
    ctx.set_tile(0, 1, 8)
    ctx.resize(w, h)
    with capi.Context(devices=[0, 0]) as g:
        g.set_moments(True)
        pc.upload_scene(g, demo, env)
        g.resize(16, 16)
        g.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, 16, 16).tobytes())
        g.render_aovs(capi.AOV_ALL)
        assert _code(g.denoise_guided, 3, *SIGMAS, flags=FLAGS).code == 4
    # a context that never enabled the moments image: both bits are unknown to it
    with capi.Context(0) as c:
        pc.upload_scene(c, demo, env)
        c.resize(16, 16)
        c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, 16, 16).tobytes())
        c.render_aovs(capi.AOV_ALL)
        assert _code(c.denoise_guided, 3, *SIGMAS, flags=FLAGS).code == 1
        assert _code(c.denoise_guided, 3, *SIGMAS, flags=capi.GUIDED_YOUNG).code == 1


def test_pass_time_includes_the_kernel(ctx, orc, demo, env):
    ctx.enable_timing(True)
    try:
        w, h = 100, 52
        _run(ctx, orc, demo, env, w, h, 3, SIGMAS, _moments(w, h, _mixed_counts(w, h)), "mix")
        ctx.sync()
        assert ctx.pass_time_us(capi.PASS_GUIDED) > 0.0
    finally:
        ctx.enable_timing(False)
