"""MI3PT_GUIDED_VARIANCE on the GPU against tests/moments_reference.py::guided_variance: the colour image (read_guided) and the last
level's variance (read_guided_variance) are compared bit for bit (ptcommon.same_bits) -- no tolerance anywhere.  The features are the
device's own read_aov of the demo scene (tests/test_gpu_aov.py pins those to the oracle).  Unless said otherwise the accumulation is
written with write_texture (seeded, [0, 4), alpha included, as tests/test_gpu_guided.py) and the moments with write_moments (seeded: M2
per channel uniform in [0, 24), n = 4 -- sigma_color^2 x the variance of the mean is then near the mean squared colour distance of 8).
The conditions that keep a case from passing vacuously are asserted on the reference's statistics, never on the device's output."""
import numpy as np
import pytest

import guided_reference as gr
import moments_edge_cases as ec
import moments_reference as mr
import ptcommon as pc
from mi3pt_host import capi

pytestmark = pytest.mark.gpu

NAMES = capi.AOV_NAMES
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
SIGMAS = (2.0, 0.35, 0.1, 0.05)
FLAG = capi.GUIDED_VARIANCE
_features = {}
_references = {}


@pytest.fixture(scope="module")
def ctx(built):
    """A context of this module's own, with the moments image on: the session's shared one never opts into it"""
    c = capi.Context(0)
    c.set_moments(True)
    yield c
    c.close()


def _prepare(ctx, demo, env, w, h):
    ctx.set_kernel_variant(0)
    ctx.set_tile(0, 1, 8)
    ctx.set_moments(True)
    pc.upload_scene(ctx, demo, env)
    ctx.resize(w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h).tobytes())
    ctx.render_aovs(capi.AOV_ALL)
    if (w, h) not in _features:
        _features[(w, h)] = {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}
    return _features[(w, h)]


def _random_accum(w, h, seed=20261018):
    return (np.random.default_rng(seed).random((h, w, 4), dtype=np.float32) * np.float32(4)).astype(np.float32)


def _random_moments(w, h, seed=20261019, scale=24.0, n=4.0):
    m = (np.random.default_rng(seed).random((h, w, 4), dtype=np.float32) * np.float32(scale)).astype(np.float32)
    m[..., 3] = np.float32(n)
    return m


def _reference(orc, feat, accum, moments, levels, sigmas, key=None):
    if key is not None and key in _references:
        return _references[key]
    out = mr.guided_variance(orc, accum, moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"], levels, *sigmas)
    if key is not None:
        _references[key] = out
    return out


def _assert_not_vacuous(stats, what):
    print(f"{what}: {stats}")
    assert stats["rejected"] >= 0.02, f"{what}: the hit rule rejects {stats['rejected']:.3f} of the in-image taps"
    assert stats["below"] >= 0.10 and stats["above"] >= 0.10, f"{what}: counted off-centre taps below / above 0.5: {stats['below']:.3f} / {stats['above']:.3f}"


def _compare(ctx, want, want_var, what, w, h):
    got, got_var = ctx.read_guided(), ctx.read_guided_variance()
    assert got.shape == (h, w, 4) and got.dtype == np.float32 and got_var.shape == (h, w) and got_var.dtype == np.float32
    assert pc.same_bits(got, want), what + ": colour: " + pc.describe_diff(got, want)
    assert pc.same_bits(got_var, want_var), what + ": variance: " + pc.describe_diff(got_var, want_var)
    return got, got_var


def _run(ctx, orc, demo, env, w, h, levels, sigmas, moments=None, key_extra=None, accum=None):
    feat = _prepare(ctx, demo, env, w, h)
    accum = _random_accum(w, h) if accum is None else accum
    moments = _random_moments(w, h) if moments is None else moments
    ctx.write_texture(capi.TEX_ACCUMULATION, accum)
    ctx.write_moments(moments)
    want, want_var, stats = _reference(orc, feat, accum, moments, levels, sigmas, key=(w, h, levels, sigmas, key_extra))
    ctx.denoise_guided(levels, *sigmas, flags=FLAG)
    what = f"{w}x{h} levels {levels} sigmas {sigmas} {key_extra or ''}"
    got, got_var = _compare(ctx, want, want_var, what, w, h)
    return got, got_var, want, want_var, stats


def _sample_frames(ctx, demo, w, h, first, count):
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=first, bounces=4).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, first).tobytes())
    ctx.submit_frames(MASK, count)


@pytest.fixture(scope="module")
def calibrated(ctx, demo, env):
    """Mean and moments accumulated by the device from frames 1 .. 4 of the demo scene at 64 x 64, and the device's own feature images"""
    w = h = 64
    feat = _prepare(ctx, demo, env, w, h)
    ctx.set_pipelining(True)
    ctx.set_storage(capi.STORAGE_F32)
    _sample_frames(ctx, demo, w, h, 1, 4)
    return feat, ctx.read_texture(capi.TEX_ACCUMULATION), ctx.read_moments()


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_calibrated_case(ctx, orc, demo, env, calibrated, levels):
    """Measured with the oracle's features: rejected / below / above = 0.043 / 0.43 / 0.57 at one level, 0.093 / 0.55 / 0.45 at three,
    0.166 / 0.61 / 0.39 at five."""
    feat, accum, moments = calibrated
    w = h = 64
    assert np.all(moments[..., 3] == 4) and (moments[..., :3] > 0).mean() > 0.9
    _prepare(ctx, demo, env, w, h)
    ctx.write_texture(capi.TEX_ACCUMULATION, accum)
    ctx.write_moments(moments)
    want, want_var, stats = _reference(orc, feat, accum, moments, levels, SIGMAS, key=("calibrated", levels, SIGMAS))
    _assert_not_vacuous(stats, f"calibrated, {levels} level(s)")
    ctx.denoise_guided(levels, *SIGMAS, flags=FLAG)
    _compare(ctx, want, want_var, f"calibrated, {levels} level(s)", w, h)


def test_calibrated_case_from_the_queue_and_nothing_else_changes(ctx, orc, demo, env, calibrated):
    """The filter called with the four frames still queued sees them in the mean AND in the moments; accumulation, moments and the four
    feature images are byte-identical before and after; the colour term alone (2, 0, 0, 0) on the same images."""
    feat, accum, moments = calibrated
    w = h = 64
    _prepare(ctx, demo, env, w, h)
    _sample_frames(ctx, demo, w, h, 1, 4)
    ctx.denoise_guided(3, *SIGMAS, flags=FLAG)                  # (the frames are still queued here: the call launches them)
    want, want_var, _ = _reference(orc, feat, accum, moments, 3, SIGMAS, key=("calibrated", 3, SIGMAS))
    _compare(ctx, want, want_var, "calibrated, from the queue", w, h)
    assert ctx.read_texture(capi.TEX_ACCUMULATION).tobytes() == accum.tobytes()
    assert ctx.read_moments().tobytes() == moments.tobytes()
    for k, name in enumerate(NAMES):
        assert ctx.read_aov(k).tobytes() == feat[name].tobytes(), name
    alone = (2.0, 0.0, 0.0, 0.0)
    want, want_var, stats = _reference(orc, feat, accum, moments, 3, alone)
    print(f"colour term alone: {stats}")
    assert stats["below"] >= 0.10 and stats["above"] >= 0.10
    ctx.denoise_guided(3, *alone, flags=FLAG)
    _compare(ctx, want, want_var, "calibrated, colour term alone", w, h)


# 1 x 1 and 3 x 2: every off-centre tap of the levels is outside the image (the 3 x 3 of the variance kernel is not, at 3 x 2); 16 x 17 and
# 17 x 16: one texel past a block; 100 x 52: ragged; 33 x 33 and 64 x 64 at five levels: taps at +-32, stride classes of one or two texels;
# 264 x 260 at four and five levels: more than one 16 x 16 tile per stride class in both axes at strides 4, 8 and 16, and at stride 16
# classes of 17 and of 16 texels (as tests/test_gpu_guided.py; the tile counts are stated in tests/test_guided_reference.py)
SIZES = [(1, 1, 3), (3, 2, 3), (16, 17, 3), (17, 16, 3), (100, 52, 3), (33, 33, 5), (64, 64, 5), (264, 260, 4), (264, 260, 5)]


@pytest.mark.parametrize("w,h,levels", SIZES, ids=[f"{w}x{h}-{n}-levels" for w, h, n in SIZES])
def test_sizes(ctx, orc, demo, env, w, h, levels):
    """Thresholds checked on the CPU with the oracle's features for the sizes >= 64 wide, M2 scale 24: 100 x 52 at three levels
    rejected / below / above = 0.052 / 0.64 / 0.36, 64 x 64 at five 0.166 / 0.71 / 0.29 (no adjustment of the scale was needed);
    264 x 260 at four levels 0.039 / 0.72 / 0.28, at five 0.059 / 0.76 / 0.24."""
    *_, stats = _run(ctx, orc, demo, env, w, h, levels, SIGMAS)
    if w >= 64:
        _assert_not_vacuous(stats, f"{w}x{h} levels {levels}")
    if (w, h) == (1, 1):
        assert stats["taps"] == levels


SIGMA_CASES = [("color", (2.0, 0.0, 0.0, 0.0)), ("normal", (0.0, 0.35, 0.0, 0.0)), ("albedo", (0.0, 0.0, 0.1, 0.0)),
               ("plane", (0.0, 0.0, 0.0, 0.05)), ("all-zero", (0.0, 0.0, 0.0, 0.0))]


@pytest.mark.parametrize("name,sigmas", SIGMA_CASES, ids=[c[0] for c in SIGMA_CASES])
def test_each_sigma_alone(ctx, orc, demo, env, name, sigmas):
    """sigma_color 0 with the flag: the colour term is off and the variance is still propagated"""
    _, got_var, _, want_var, stats = _run(ctx, orc, demo, env, 100, 52, 3, sigmas)
    if name == "all-zero":
        assert stats["below"] == 0.0 and stats["above"] == 1.0       # every counted tap weighs h[dx] * h[dy]
    else:
        assert stats["below"] > 0.0, f"sigma_{name} alone changes no weight of this case"
    feat = _features[(100, 52)]
    var0 = mr.initial_variance(_random_moments(100, 52), feat["ids"][..., 2])
    assert (want_var > 0).all() and (want_var < var0).mean() > 0.9      # three levels of squared weights: the variance shrank


def test_one_sample_everywhere(ctx, orc, demo, env):
    """n = 1: v = 0 everywhere, denom = EPS -- any colour difference at all puts a tap's weight at exp(-huge) = 0"""
    w, h = 100, 52
    _, got_var, _, want_var, stats = _run(ctx, orc, demo, env, w, h, 3, SIGMAS, moments=_random_moments(w, h, n=1.0), key_extra="n=1")
    assert not want_var.any() and stats["above"] < 0.01


def test_negative_and_nan_moments(ctx, orc, demo, env):
    """M2 with negative and NaN entries (and n of 0, negative, NaN) at a handful of texels: the bits of the reference, no fault"""
    w, h = 100, 52
    m = _random_moments(w, h)
    m[3, 5, :3] = (-50.0, -60.0, -70.0)
    m[3, 6, 0] = np.nan
    m[10, 20] = (np.nan, np.nan, np.nan, 4.0)
    m[11, 21, 1] = -1e30
    m[30, 40, 3] = 0.0
    m[30, 41, 3] = -3.0
    m[30, 42, 3] = np.nan
    m[51, 99, :3] = np.inf
    _, got_var, _, want_var, _ = _run(ctx, orc, demo, env, w, h, 3, SIGMAS, moments=m, key_extra="bad")
    assert np.isfinite(want_var[0, 0]) and np.array_equal(np.isnan(got_var), np.isnan(want_var))


EDGE_SIZE = (100, 52)
# sigma_color 2 with the patches' variance of the mean of 0.0081: a squared colour distance of 3 weighs exp(-92.6), a subnormal.  One level:
# from the second on the plain texels around a patch reach into it (the colour term does not tighten per level under the flag)
SUBNORMAL_SIGMAS, SUBNORMAL_LEVELS = (ec.SUBNORMAL_SIGMA_VARIANCE, 0.35, 0.1, 0.05), 1
NON_FINITE_AT = [(5, 9), (5, 60), (26, 35), (45, 9), (45, 85), (26, 90)]


def subnormal_pair(w, h):
    accum, moments = _random_accum(w, h), _random_moments(w, h)
    ec.subnormal_patches(accum, moments)
    return accum, moments


def catalogue_pair(w, h):
    """the seeded pair with the count and M2 entries of the whole catalogue, NaN and infinite ones included, six texels apart: after three
    levels a NaN has spread over 29 x 29 texels of its hit class, and half of the image is to stay comparable"""
    accum, moments = _random_accum(w, h), _random_moments(w, h)
    where = ec.overlay(accum, moments, 3, False, only=lambda name: "mean" not in name, pitch=6)
    return accum, moments, where


def non_finite_accum(w, h):
    """the finite means of the catalogue six texels apart, and the six non-finite ones once each"""
    accum = _random_accum(w, h)
    ec.overlay(accum, np.zeros((h, w, 4), np.float32), 4, True, only=lambda name: name.startswith("mean="), pitch=6)
    ec.non_finite_means(accum, NON_FINITE_AT)
    return accum


def test_count_and_m2_catalogue(ctx, orc, demo, env):
    """k_guided_variance's `n >= 2 ? fmaxf(sum / (n (n - 1)), 0) : 0` at the counts on either side of 2 (1.5, the float below 2, 2), at NaN,
    negative and infinite counts, with sums that are negative, subnormal, overflow or are NaN, on both sides of the 16 x 16 tile seams of
    the level kernel -- then three levels on top.  The bits of the reference, a NaN where it has one"""
    w, h = EDGE_SIZE
    accum, moments, where = catalogue_pair(w, h)
    assert not ec.seam_sides(where, w, h)
    got, got_var, want, want_var, stats = _run(ctx, orc, demo, env, w, h, 3, SIGMAS, accum=accum, moments=moments, key_extra="catalogue")
    print(f"count and M2 catalogue: a NaN in {float(np.isnan(want_var).mean()):.3f} of the variance's texels; {stats}")
    assert np.isnan(want_var).any() and np.isnan(want_var).mean() <= 0.5
    assert pc.same_bits_or_nan(got, want) and pc.same_bits_or_nan(got_var, want_var)


def test_subnormal_weights(ctx, orc, demo, env):
    """weights in the fp32 subnormal range (tests/moments_edge_cases.py: subnormal_patches); a build that flushes them, or an exp that
    cuts off early, gives 0 where the reference has 6e-42 (tests/test_moments_edge_cases.py shows that on the reference alone)"""
    w, h = EDGE_SIZE
    accum, moments = subnormal_pair(w, h)
    *_, stats = _run(ctx, orc, demo, env, w, h, SUBNORMAL_LEVELS, SUBNORMAL_SIGMAS, accum=accum, moments=moments, key_extra="subnormal")
    print(f"subnormal weights: {stats['subnormal']} counted taps; {stats}")
    assert stats["subnormal"] > 0


SQUARED_SIGMAS = {"features off": (ec.SQUARED_SIGMA, 0.0, 0.0, 0.0), "default features": (ec.SQUARED_SIGMA, 0.35, 0.1, 0.05)}


def squared_pair(w, h, ids, delta=ec.SQUARED_DELTA[45]):
    """the seeded pair with moments_edge_cases.squared_weight_patches inside the hit classes: (accum, moments, the rings' mask)"""
    accum, moments = _random_accum(w, h), _random_moments(w, h)
    centres = ec.squared_weight_patches(accum, moments, np.ascontiguousarray(ids).view(np.int32)[..., 2], delta)
    return accum, moments, ec.rings(centres, (h, w))


@pytest.mark.parametrize("name", list(SQUARED_SIGMAS))
def test_subnormal_squared_weights(ctx, orc, demo, env, name):
    """`nv = nv + (w * w) * var(q)` with a normal w whose square is an fp32 subnormal (tests/moments_edge_cases.py:
    squared_weight_patches; test_subnormal_weights makes w itself subnormal, so its square is 0): the rings around the bright blocks
    carry variances of 2e-40 .. 7e-37 that a build which flushes the squares returns as 0 (tests/test_moments_edge_cases.py shows that
    on the reference alone).  One level, bit for bit"""
    w, h = EDGE_SIZE
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments, ring = squared_pair(w, h, feat["ids"])
    *_, want_var, stats = _run(ctx, orc, demo, env, w, h, 1, SQUARED_SIGMAS[name], accum=accum, moments=moments, key_extra="squared weights")
    tiny = (want_var[ring] > 0) & (want_var[ring] < gr.TINY)
    print(f"squared weights, {name}: {stats['squared_subnormal']} counted taps with a normal weight and a subnormal square; {int(tiny.sum())} of "
          f"{int(ring.sum())} ring texels hold a subnormal variance")
    assert stats["squared_subnormal"] >= 1000 and tiny.sum() >= 100 and (want_var[ring] > 0).mean() >= 0.9


def test_non_finite_colours(ctx, orc, demo, env):
    """means at the ends of fp32 and binary16, and six texels with infinities and NaNs, two levels"""
    w, h = EDGE_SIZE
    got, got_var, want, want_var, stats = _run(ctx, orc, demo, env, w, h, 2, SIGMAS, accum=non_finite_accum(w, h), key_extra="non-finite colours")
    share = float(np.isnan(want).any(axis=-1).mean())
    print(f"non-finite colours: a NaN in {share:.3f} of the texels; {stats['subnormal']} counted taps with a subnormal weight")
    assert 0 < share <= 0.5 and pc.same_bits_or_nan(got, want) and pc.same_bits_or_nan(got_var, want_var)


def test_present_draws_the_canvas_from_the_filtered_image(ctx, orc, demo, env):
    """The flag together with MI3PT_GUIDED_PRESENT: the canvas equals the oracle's fullscreen pass on the REFERENCE image, `denoise` 0"""
    w, h = 100, 52
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments = _random_accum(w, h), _random_moments(w, h)
    ctx.write_texture(capi.TEX_ACCUMULATION, accum)
    ctx.write_moments(moments)
    want, want_var, _ = _reference(orc, feat, accum, moments, 3, SIGMAS, key=(w, h, 3, SIGMAS, None))
    ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(w, h, 1.0, denoise=1, tonemapping=1).tobytes())
    ctx.denoise_guided(3, *SIGMAS, flags=FLAG | capi.GUIDED_PRESENT)
    want_f, want_8 = orc.fullscreen(pc.fs_uniforms(w, h, 1.0, denoise=0, tonemapping=1).tobytes(), want)
    got_f, got_8 = ctx.read_texture(capi.TEX_CANVAS), ctx.read_canvas_rgba8()
    assert pc.same_bits(got_f, want_f), pc.describe_diff(got_f, want_f)
    assert np.array_equal(got_8.reshape(want_8.shape), want_8)
    _compare(ctx, want, want_var, "with present", w, h)


def _code(fn, *a, **kw):
    with pytest.raises(capi.Mi3ptError) as e:
        fn(*a, **kw)
    return e.value


def test_without_the_flag_and_without_moments(ctx, orc, demo, env):
    w, h = 100, 52
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments = _random_accum(w, h), _random_moments(w, h)
    ctx.write_texture(capi.TEX_ACCUMULATION, accum)
    ctx.write_moments(moments)
    # a call without the flag, made with moments enabled: exactly the bits of the filter as it was
    plain = (4.0, 0.35, 0.1, 0.05)
    ctx.denoise_guided(3, *SIGMAS, flags=FLAG)
    ctx.denoise_guided(3, *plain)
    want, _ = gr.guided(orc, accum, feat["normal"], feat["position"], feat["albedo"], feat["ids"], 3, *plain)
    got = ctx.read_guided()
    assert pc.same_bits(got, want), pc.describe_diff(got, want)
    assert _code(ctx.read_guided_variance).code == 4                        # the last filter ran without the flag
    ctx.denoise_guided(1, *SIGMAS, flags=FLAG)
    out = np.empty((h, w), np.float32)
    assert ctx.lib.mi3pt_read_guided_variance(ctx.handle, out.ctypes.data, out.size - 1) == 1
    assert ctx.lib.mi3pt_read_guided_variance(ctx.handle, None, out.size) == 1
    assert ctx.read_guided_variance().shape == (h, w)
    ctx.resize(w, h)
    assert _code(ctx.read_guided_variance).code == 4                        # a resize frees the images
    # the flag without the moments image: refused, and the message says what is missing
    ctx.render_aovs(capi.AOV_ALL)
    ctx.set_moments(False)
    e = _code(ctx.denoise_guided, 3, *SIGMAS, flags=FLAG)
    assert e.code == 4 and "mi3pt_set_moments" in e.message
    ctx.denoise_guided(3, *plain)                                            # (the plain filter still runs)
    ctx.set_moments(True)
    # a rank of a tile split and a device group stay refused, with the flag too
    ctx.set_tile(0, 2, 8)
    ctx.resize(w, h)
    ctx.render_aovs(capi.AOV_ALL)
    assert _code(ctx.denoise_guided, 3, *SIGMAS, flags=FLAG).code == 4
    ctx.set_tile(0, 1, 8)
    ctx.resize(w, h)
    with capi.Context(devices=[0, 0]) as g:
        g.set_moments(True)
        pc.upload_scene(g, demo, env)
        g.resize(16, 16)
        g.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, 16, 16).tobytes())
        g.render_aovs(capi.AOV_ALL)
        assert _code(g.denoise_guided, 3, *SIGMAS, flags=FLAG).code == 4
        assert _code(g.read_guided_variance).code == 4
    # a context that never enabled the moments image answers as it did before the flag existed: bit 1 is unknown to it
    with capi.Context(0) as c:
        pc.upload_scene(c, demo, env)
        c.resize(16, 16)
        c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, 16, 16).tobytes())
        c.render_aovs(capi.AOV_ALL)
        assert _code(c.denoise_guided, 3, *SIGMAS, flags=FLAG).code == 1
        c.denoise_guided(1, *plain)
        assert _code(c.read_guided_variance).code == 4


def test_pass_time_includes_the_variance_kernel(ctx, orc, demo, env):
    ctx.enable_timing(True)
    try:
        _run(ctx, orc, demo, env, 100, 52, 3, SIGMAS)
        ctx.sync()
        assert ctx.pass_time_us(capi.PASS_GUIDED) > 0.0
    finally:
        ctx.enable_timing(False)
