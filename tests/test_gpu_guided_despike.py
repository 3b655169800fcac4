"""The firefly pre-pass of mi3pt_denoise_guided on the GPU (mi3pt_set_guided_despike; csrc/pt_guided.hip: k_guided_despike and the
_despiked twins of the two var_0 kernels) against tests/guided_despike_reference.py: the filtered image (read_guided), the last level's
variance where the mode has one (read_guided_variance) and the count of clamped texels (read_guided_despiked) are compared bit for bit
(ptcommon.same_bits) -- no tolerance anywhere.  Modelled on tests/test_gpu_guided_young.py: the features are the device's own read_aov of
the demo scene, the accumulation is written with write_texture and the moments with write_moments.  The kernel works on 32 x 8 tiles
with a halo of 1 and counts in 64 slots by wave number; tests/despike_edge_cases.py holds the images (they are built once more, with the
oracle's features, by tests/test_despike_edge_cases.py) and the worked examples of the value range.  The conditions that keep a case
from passing vacuously are asserted on the reference's statistics, never on the device's output."""
import ctypes

import numpy as np
import pytest

import despike_edge_cases as de
import guided_despike_reference as dr
import guided_reference as gr
import moments_reference as mr
import ptcommon as pc
from mi3pt_host import capi

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = capi.AOV_NAMES
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
TEX = capi.TEX_ACCUMULATION
SIGMAS = (2.0, 0.35, 0.1, 0.05)
MODES = {"fixed": 0, "variance": capi.GUIDED_VARIANCE, "young": capi.GUIDED_VARIANCE | capi.GUIDED_YOUNG}
class_of, spiked_accum, smooth_accum, mixed_moments = de.class_of, de.spiked_accum, de.smooth_accum, de.mixed_moments
_features = {}
_references = {}


@pytest.fixture(scope="module")
def ctx(built):
    c = capi.Context(0)
    c.set_moments(True)
    yield c
    c.set_guided_despike(False)
    c.set_storage(capi.STORAGE_F32)
    c.close()


def _prepare(ctx, demo, env, w, h):
    ctx.set_kernel_variant(0)
    ctx.set_tile(0, 1, 8)
    ctx.set_storage(capi.STORAGE_F32)
    ctx.set_mean_by_count(False)
    ctx.set_moments(True)
    ctx.set_guided_despike(True)
    pc.upload_scene(ctx, demo, env)
    ctx.resize(w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h).tobytes())
    ctx.render_aovs(capi.AOV_ALL)
    if (w, h) not in _features:
        _features[(w, h)] = {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}
    return _features[(w, h)]


def reference(orc, feat, accum, moments, mode, levels, sigmas=SIGMAS, key=None):
    """(filtered, variance or None, stats) of the mode behind the pre-pass"""
    if key is not None and (mode, levels, key) in _references:
        return _references[(mode, levels, key)]
    args = (feat["normal"], feat["position"], feat["albedo"], feat["ids"], levels, *sigmas)
    if mode == "fixed":
        out, _, _, stats = dr.guided(orc, accum, *args)
        got = (out, None, stats)
    else:
        out, var, _, _, stats = dr.guided_variance(orc, accum, moments, *args, young=mode == "young")
        got = (out, var, stats)
    if key is not None:
        _references[(mode, levels, key)] = got
    return got


def plain_reference(orc, feat, accum, moments, mode, levels, sigmas=SIGMAS):
    """the same call with the state off"""
    import guided_young_reference as yr
    args = (feat["normal"], feat["position"], feat["albedo"], feat["ids"], levels, *sigmas)
    if mode == "fixed":
        return gr.guided(orc, accum, *args)[0], None
    fn = yr.guided_variance_young if mode == "young" else mr.guided_variance
    out, var, _ = fn(orc, accum, moments, *args)
    return out, var


def _compare(ctx, want, want_var, want_count, what, same=pc.same_bits):
    got = ctx.read_guided()
    assert got.shape == want.shape and got.dtype == np.float32
    assert same(got, want), what + ": colour: " + pc.describe_diff(got, want)
    if want_var is not None:
        got_var = ctx.read_guided_variance()
        assert same(got_var, want_var), what + ": variance: " + pc.describe_diff(got_var, want_var)
    if want_count is not None:
        assert ctx.read_guided_despiked() == want_count, what + ": count"
    return got


def not_vacuous(stats, w, h):
    """1 % .. 40 % of the texels clamped and a texel with fewer than eight taps; 1 x 1 has no tap and nothing to clamp"""
    if (w, h) == (1, 1):
        assert stats["count"] == 0 and stats["lone"] == 1.0
    else:
        assert 0.01 <= stats["clamped"] <= 0.40, stats
        assert stats["m_min"] < 8


def _run(ctx, orc, demo, env, w, h, mode, levels, sigmas=SIGMAS, same=pc.same_bits):
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments = spiked_accum(feat["ids"]), mixed_moments(w, h)
    ctx.write_texture(TEX, accum)
    ctx.write_moments(moments)
    want, want_var, stats = reference(orc, feat, accum, moments, mode, levels, sigmas, key=(w, h, sigmas))
    what = f"{w}x{h} {mode} levels {levels}"
    print(f"{what}: {stats}")
    not_vacuous(stats, w, h)
    ctx.denoise_guided(levels, *sigmas, flags=MODES[mode])
    _compare(ctx, want, want_var, stats["count"], what, same)
    return feat, accum, moments, want, want_var, stats


# 48 x 32: two tiles by four; 33 x 17: one texel past the 32 x 8 tile in x, partial blocks on both edges; 70 x 9: three tiles in x, one row
# past the tile; 5 x 1: no row neighbours; 1 x 1: no neighbour at all
SIZES = [(48, 32), (33, 17), (70, 9), (5, 1), (1, 1)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes(ctx, orc, demo, env, w, h, mode):
    *_, want, want_var, stats = _run(ctx, orc, demo, env, w, h, mode, 3)
    if mode != "fixed" and (w, h) != (1, 1):
        # the scaled var_0 is not the plain one: the state changes the variance the levels carry
        feat = _features[(w, h)]
        plain = plain_reference(orc, feat, spiked_accum(feat["ids"]), mixed_moments(w, h), mode, 3)
        assert not pc.same_bits(want_var, plain[1]) and not pc.same_bits(want, plain[0])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("levels", [1, 5])
def test_levels(ctx, orc, demo, env, levels, mode):
    _run(ctx, orc, demo, env, 33, 17, mode, levels)


def _sample(ctx, demo, w, h, first, count):
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=first, bounces=4).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, first).tobytes())
    ctx.submit_frames(MASK, count)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("storage", ["f32", "f16"])
def test_a_mean_of_four_device_frames_with_the_sun(ctx, orc, demo, env, storage, mode):
    """48 x 32, the hosts' default environment: the fireflies the pre-pass is for, in the mean the accumulate step stores (under F16 storage
    rounded to binary16), filtered while the frames are still queued.  Accumulation, moments and counters are those of before the call."""
    w, h = 48, 32
    feat = _prepare(ctx, demo, env, w, h)
    try:
        if storage == "f16":
            ctx.set_storage(capi.STORAGE_F16)
            ctx.resize(w, h)
            ctx.render_aovs(capi.AOV_ALL)
        ctx.reset()
        _sample(ctx, demo, w, h, 1, 4)
        ctx.denoise_guided(3, *SIGMAS, flags=MODES[mode])            # (the frames are still queued here: the call launches them)
        accum, moments, counters = ctx.read_texture(TEX), ctx.read_moments(), ctx.counters()
        assert np.all(moments[..., 3] == 4)
        if storage == "f16":
            assert pc.same_bits(accum[..., :3], accum[..., :3].astype(np.float16).astype(F))
        want, want_var, stats = reference(orc, feat, accum, moments, mode, 3)
        print(f"four frames, {storage}, {mode}: {stats}")
        not_vacuous(stats, w, h)
        _compare(ctx, want, want_var, stats["count"], f"four frames, {storage}, {mode}")
        ctx.denoise_guided(3, *SIGMAS, flags=MODES[mode])            # and again on the settled image
        _compare(ctx, want, want_var, stats["count"], f"four frames, {storage}, {mode}, again")
        assert ctx.read_texture(TEX).tobytes() == accum.tobytes() and ctx.read_moments().tobytes() == moments.tobytes()
        assert ctx.counters() == counters
        for k, name in enumerate(NAMES):
            assert ctx.read_aov(k).tobytes() == feat[name].tobytes()
    finally:
        ctx.set_storage(capi.STORAGE_F32)


def test_two_adjacent_spikes_and_the_corners(ctx, orc, demo, env):
    """the planted texels of spiked_accum, on the reference: every corner is clamped unless it is alone in its class, the brighter of the
    adjacent pair comes down to the other one and that one stays -- and the device agrees (test_sizes compares this very image)"""
    w, h = 48, 32
    feat, accum, *_ = _run(ctx, orc, demo, env, w, h, "fixed", 3)
    cd, s, _ = dr.despike(accum, feat["ids"])
    lum = dr.luminance(accum)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        assert s[y, x] < 0.2, (y, x)
    big = lum > 100
    pair = big[:, :-1] & big[:, 1:] & (class_of(feat["ids"])[:, :-1] == class_of(feat["ids"])[:, 1:])
    assert pair.any()
    y, x = np.argwhere(pair)[0]
    lo, hi = sorted(((y, x), (y, x + 1)), key=lambda p: lum[p])
    assert s[lo] == 1 and s[hi] == lum[lo] / lum[hi]
    border = s < 0.2
    assert border.sum() > 8                      # the spikes on the class borders came down to their own side


def _nonfinite_accum(ids):
    a = spiked_accum(ids, seed=11)
    h, w = a.shape[:2]
    values = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    k = 0
    for y in range(1, h, 5):
        for x in range(2, w, 7):
            a[y, x, k % 3] = values[k % len(values)]
            if k % 4 == 0:
                a[y, x, :3] = values[k % len(values)]
            k += 1
    return a


@pytest.mark.parametrize("mode", list(MODES))
def test_non_finite_texels(ctx, orc, demo, env, mode):
    """NaN, +inf and -inf in single channels and in whole texels, as centres and as neighbours: the bits of the reference, a NaN where it
    has one, the same count; no fault.  One level: the levels spread a NaN over 5 x 5 texels each"""
    w, h = 48, 32
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments = _nonfinite_accum(feat["ids"]), mixed_moments(w, h)
    ctx.write_texture(TEX, accum)
    ctx.write_moments(moments)
    want, want_var, stats = reference(orc, feat, accum, moments, mode, 1)
    share = float(np.isnan(want).any(axis=-1).mean())
    print(f"non-finite, {mode}: {stats}; a NaN in {share:.3f} of the filtered texels")
    assert 0 < share <= 0.9 and stats["count"] > 0
    ctx.denoise_guided(1, *SIGMAS, flags=MODES[mode])
    _compare(ctx, want, want_var, stats["count"], "non-finite " + mode, same=pc.same_bits_or_nan)


@pytest.mark.parametrize("mode", list(MODES))
def test_state_off_after_on_and_an_image_without_a_spike(ctx, orc, demo, env, mode):
    w, h = 33, 17
    feat, accum, moments, want, want_var, stats = _run(ctx, orc, demo, env, w, h, mode, 3)
    plain, plain_var = plain_reference(orc, feat, accum, moments, mode, 3)
    assert not pc.same_bits(want, plain)
    # off after on: the bits of the call as it always was, and no count to read
    ctx.set_guided_despike(False)
    ctx.denoise_guided(3, *SIGMAS, flags=MODES[mode])
    _compare(ctx, plain, plain_var, None, "state off after on")
    with pytest.raises(capi.Mi3ptError) as e:
        ctx.read_guided_despiked()
    assert e.value.code == 4
    # on again: the pre-pass's bits again
    ctx.set_guided_despike(True)
    ctx.denoise_guided(3, *SIGMAS, flags=MODES[mode])
    _compare(ctx, want, want_var, stats["count"], "state on again")
    # a colour per class: nothing is clamped, the state on gives the bits of the state off
    flat = smooth_accum(feat["ids"])
    ctx.write_texture(TEX, flat)
    ctx.write_moments(moments)
    _, _, flat_stats = reference(orc, feat, flat, moments, mode, 3)
    assert flat_stats["count"] == 0
    plain, plain_var = plain_reference(orc, feat, flat, moments, mode, 3)
    ctx.denoise_guided(3, *SIGMAS, flags=MODES[mode])
    on = _compare(ctx, plain, plain_var, 0, "no spike, state on")
    ctx.set_guided_despike(False)
    ctx.denoise_guided(3, *SIGMAS, flags=MODES[mode])
    assert ctx.read_guided().tobytes() == on.tobytes()


def test_present_draws_the_canvas_from_the_filtered_image(ctx, orc, demo, env):
    """MI3PT_GUIDED_PRESENT with the state on: the canvas equals the oracle's fullscreen pass on the REFERENCE image, `denoise` 0"""
    w, h = 48, 32
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments = spiked_accum(feat["ids"]), mixed_moments(w, h)
    ctx.write_texture(TEX, accum)
    ctx.write_moments(moments)
    want, _, stats = reference(orc, feat, accum, moments, "fixed", 3, key=(w, h, SIGMAS))
    ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(w, h, 1.0, denoise=1, tonemapping=1).tobytes())
    ctx.denoise_guided(3, *SIGMAS, flags=capi.GUIDED_PRESENT)
    want_f, want_8 = orc.fullscreen(pc.fs_uniforms(w, h, 1.0, denoise=0, tonemapping=1).tobytes(), want)
    got_f, got_8 = ctx.read_texture(capi.TEX_CANVAS), ctx.read_canvas_rgba8()
    assert pc.same_bits(got_f, want_f), pc.describe_diff(got_f, want_f)
    assert np.array_equal(got_8.reshape(want_8.shape), want_8)
    _compare(ctx, want, None, stats["count"], "with present")


def _code(fn, *a, **kw):
    with pytest.raises(capi.Mi3ptError) as e:
        fn(*a, **kw)
    return e.value.code


def test_error_codes(ctx, orc, demo, env):
    lib = capi.load_library()
    n = ctypes.c_uint32()
    # a null context, a null pointer
    assert lib.mi3pt_set_guided_despike(None, 1) == 1
    assert lib.mi3pt_read_guided_despiked(None, ctypes.byref(n)) == 1
    w, h = 33, 17
    feat = _prepare(ctx, demo, env, w, h)
    assert lib.mi3pt_read_guided_despiked(ctx.handle, None) == 1
    # no filter since the resize; a filter with the state off; a filter with the state on; a resize
    assert _code(ctx.read_guided_despiked) == 4
    ctx.write_texture(TEX, spiked_accum(feat["ids"]))
    ctx.set_guided_despike(False)
    ctx.denoise_guided(3, *SIGMAS)
    assert _code(ctx.read_guided_despiked) == 4
    ctx.set_guided_despike(True)
    ctx.denoise_guided(3, *SIGMAS)
    assert ctx.read_guided_despiked() > 0
    ctx.resize(w, h)
    assert _code(ctx.read_guided_despiked) == 4
    ctx.render_aovs(capi.AOV_ALL)
    # bit 8 and the bits above it are no flags
    for bit in (8, 16, 1 << 31):
        assert _code(ctx.denoise_guided, 3, *SIGMAS, flags=bit) == 1
    # a rank of a tile split and a device group stay refused; the setter goes to every member of a group
    ctx.set_tile(0, 2, 8)
    ctx.resize(w, h)
    ctx.render_aovs(capi.AOV_ALL)
    assert _code(ctx.denoise_guided, 3, *SIGMAS) == 4
    ctx.set_tile(0, 1, 8)
    ctx.resize(w, h)
    with capi.Context(devices=[0, 0]) as g:
        g.set_guided_despike(True)
        pc.upload_scene(g, demo, env)
        g.resize(16, 16)
        g.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, 16, 16).tobytes())
        g.render_aovs(capi.AOV_ALL)
        assert _code(g.denoise_guided, 3, *SIGMAS) == 4
        assert _code(g.read_guided_despiked) == 4
    # a context that never opted into moments: the state is no flag bit, the fixed-sigma mode runs behind the pre-pass
    with capi.Context(0) as c:
        pc.upload_scene(c, demo, env)
        c.resize(w, h)
        c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h).tobytes())
        c.render_aovs(capi.AOV_ALL)
        accum = spiked_accum(feat["ids"])
        c.write_texture(TEX, accum)
        c.set_guided_despike(True)
        c.denoise_guided(3, *SIGMAS)
        want, _, stats = reference(orc, feat, accum, None, "fixed", 3, key=(w, h, SIGMAS))
        _compare(c, want, None, stats["count"], "a context without moments")


def test_pass_time_includes_the_kernel(ctx, orc, demo, env):
    ctx.enable_timing(True)
    try:
        _run(ctx, orc, demo, env, 48, 32, "variance", 3)
        ctx.sync()
        assert ctx.pass_time_us(capi.PASS_GUIDED) > 0.0
    finally:
        ctx.enable_timing(False)


# ---- the count past its DESPIKE_SLOTS slots (DESIGN.md "Pinned decomposition"; tests/despike_edge_cases.py: count_slots).  96 x 48: 18
# blocks, 72 waves, 8 slots shared by two waves; 160 x 32: 20 blocks in five columns, 80 waves, 16 shared slots; 264 x 260: 297 blocks in
# nine columns and 33 rows, 1188 waves, every slot shared -- there the _despiked twins of the two var_0 kernels also run over several
# tiles in both axes.  tests/test_despike_edge_cases.py asserts the same conditions with the oracle's features
SLOT_SIZES = [(96, 48, m, 3) for m in MODES] + [(160, 32, m, 3) for m in MODES] + [(264, 260, "fixed", 1), (264, 260, "young", 1)]


@pytest.mark.parametrize("w,h,mode,levels", SLOT_SIZES, ids=[f"{w}x{h}-{m}" for w, h, m, _ in SLOT_SIZES])
def test_the_count_is_folded_over_more_waves_than_slots(ctx, orc, demo, env, w, h, mode, levels):
    feat, accum, *_, stats = _run(ctx, orc, demo, env, w, h, mode, levels)
    texels, waves, adding = de.assert_crosses_the_slots(dr.despike(accum, feat["ids"])[1] != 1)
    print(f"{w}x{h}: {de.launch_shape(w, h)} blocks / waves, {len(adding)} waves add to {int((texels > 0).sum())} slots, {int((waves >= 2).sum())} "
          f"slots shared; slots 0 .. 31 hold {int(texels[:32].sum())} of {stats['count']}")


def test_the_count_slots_are_cleared_by_every_call(ctx, orc, demo, env):
    """three filters on one context without a resize between them: the spiked image, an image with nothing to clamp -- a slot the call
    does not clear shows here --, the spiked image again"""
    w, h = 96, 48
    feat, accum, moments, want, _, stats = _run(ctx, orc, demo, env, w, h, "fixed", 3)
    de.assert_crosses_the_slots(dr.despike(accum, feat["ids"])[1] != 1)
    flat = smooth_accum(feat["ids"])
    ctx.write_texture(TEX, flat)
    flat_want, _, flat_stats = reference(orc, feat, flat, moments, "fixed", 3)
    assert flat_stats["count"] == 0
    ctx.denoise_guided(3, *SIGMAS)
    _compare(ctx, flat_want, None, 0, "nothing to clamp after a spiked image")
    ctx.write_texture(TEX, accum)
    ctx.denoise_guided(3, *SIGMAS)
    _compare(ctx, want, None, stats["count"], "the spiked image again")


# ---- the value range of the pre-pass (DESIGN.md "Pinned value range"; tests/despike_edge_cases.py: catalogue, EXAMPLES)
EDGE_SIZES = [(96, 48), (100, 52)]
# sigma_color 1e-3: a squared colour distance above 1e-4 weighs exp(-100 ...) = 0, so the output follows c' texel by texel
TIGHT = (1e-3,) + SIGMAS[1:]
EDGE_CASES = [(w, h, m, SIGMAS) for w, h in EDGE_SIZES for m in MODES] + [(w, h, "fixed", TIGHT) for w, h in EDGE_SIZES]


def edge_reference(orc, feat, w, h, mode, sigmas, finite=False, examples=True, stored=None):
    """the catalogue's images, the reference of one level over them and the conditions that keep the case from being vacuous, asserted on
    the reference alone.  stored: the accumulation as the device holds it (F16 storage)"""
    moments = mixed_moments(w, h)
    accum, where, placed = de.catalogue(feat["ids"], finite, moments, examples)
    if stored is not None:
        accum = stored
    want, want_var, stats = reference(orc, feat, accum, moments, mode, 1, sigmas)
    cd, s, _ = dr.despike(accum, feat["ids"])
    share = float(np.isnan(want).any(axis=-1).mean())
    print(f"{w}x{h} {mode} sigma_color {sigmas[0]}: {stats['count']} clamped ({stats['clamped']:.3f}), s = 0 at {int((s == 0).sum())}, subnormal s at "
          f"{int(((s > 0) & (s < gr.TINY)).sum())}, a NaN in {float(np.isnan(cd).any(axis=-1).mean()):.3f} of c' and {share:.3f} of the filtered texels")
    assert stats["count"] > 0 and 0.01 <= stats["clamped"] <= 0.40
    if stored is None:
        assert not de.ec.seam_sides(where, w, h) and min(de.coverage(where, placed, feat["ids"]).values()) >= 1
    assert 0 < share <= 0.5
    if examples:
        de.check_examples(placed, cd, s, accum)
        assert (s == 0).any() and ((s > 0) & (s < gr.TINY)).any()
        if mode != "fixed":
            _, hit = dr._class_of(feat["ids"])
            if mode == "young":
                import guided_young_reference as yr
                var0 = yr.initial_variance_young(orc, cd, moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"], *sigmas[1:])[0]
            else:
                var0 = mr.initial_variance(moments, hit)
            de.check_example_variances(placed, var0, dr._scaled(var0, s))
    if sigmas is TIGHT:
        ok = np.isfinite(cd[..., :3]).all(axis=-1) & np.isfinite(want[..., :3]).all(axis=-1)
        close = np.abs(want[..., :3].astype(np.float64) - cd[..., :3]) <= 2.0 ** -22 * np.abs(cd[..., :3].astype(np.float64))
        assert ok.mean() >= 0.5 and close.all(axis=-1)[ok].mean() >= 0.95
    return accum, moments, want, want_var, stats


@pytest.mark.parametrize("w,h,mode,sigmas", EDGE_CASES, ids=[f"{w}x{h}-{m}-{'tight' if s is TIGHT else 'default'}" for w, h, m, s in EDGE_CASES])
def test_value_edges(ctx, orc, demo, env, w, h, mode, sigmas):
    """the means of the catalogue, NaN and +-inf included, six texels apart and on both sides of every tile seam of the spiked image, and
    the worked examples: ties, negative and -0 luminances under the 0 floor of the cap, luminances that overflow from finite channels,
    subnormals on both sides of the division, an s whose square underflows.  One level (it spreads a NaN over 5 x 5 texels); the bits of
    the reference, a NaN where it has one, the same count"""
    feat = _prepare(ctx, demo, env, w, h)
    accum, moments, want, want_var, stats = edge_reference(orc, feat, w, h, mode, sigmas)
    ctx.write_texture(TEX, accum)
    ctx.write_moments(moments)
    ctx.denoise_guided(1, *sigmas, flags=MODES[mode])
    _compare(ctx, want, want_var, stats["count"], f"value edges {w}x{h} {mode}", same=pc.same_bits_or_nan)


@pytest.mark.parametrize("mode", list(MODES))
def test_value_edges_of_a_mean_stored_as_binary16(ctx, orc, demo, env, mode):
    """the finite catalogue, six texels apart, as a context under F16 storage holds it -- every channel a binary16 value: 65520, 1e19 and
    3e38 are +inf, 1e-42 is 0 --: the pre-pass reads the mean as stored and does not round what it writes"""
    w, h = EDGE_SIZES[0]
    feat = _prepare(ctx, demo, env, w, h)
    try:
        ctx.set_storage(capi.STORAGE_F16)
        ctx.resize(w, h)
        ctx.render_aovs(capi.AOV_ALL)
        accum, _, _ = de.catalogue(feat["ids"], True, None, examples=False)
        with np.errstate(over="ignore"):
            accum[..., :3] = accum[..., :3].astype(np.float16).astype(F)          # what an accumulate step stores (write_texture keeps the bits it is given)
        ctx.write_texture(TEX, accum)
        stored = ctx.read_texture(TEX)
        assert stored.tobytes() == accum.tobytes() and np.isinf(stored).any()
        _, moments, want, want_var, stats = edge_reference(orc, feat, w, h, mode, SIGMAS, finite=True, examples=False, stored=stored)
        assert not pc.same_bits_or_nan(want[..., :3], want[..., :3].astype(np.float16).astype(F))
        ctx.write_moments(moments)
        ctx.denoise_guided(1, *SIGMAS, flags=MODES[mode])
        _compare(ctx, want, want_var, stats["count"], f"value edges under F16 storage, {mode}", same=pc.same_bits_or_nan)
    finally:
        ctx.set_storage(capi.STORAGE_F32)


@pytest.mark.parametrize("value", [F(3e38), F(np.inf)], ids=["3e38", "inf"])
def test_a_texel_alone_in_its_class_keeps_the_largest_mean(ctx, orc, demo, env, value):
    """48 x 12 has a texel without a 3 x 3 neighbour of its class (96 x 48 and 100 x 52 have none): m = 0, left alone whatever it holds"""
    w, h = 48, 12
    feat = _prepare(ctx, demo, env, w, h)
    lone = np.argwhere(de.taps_of_class(class_of(feat["ids"])) == 0)
    assert len(lone) >= 1
    accum, moments = spiked_accum(feat["ids"]), mixed_moments(w, h)
    for y, x in lone:
        accum[y, x, :3] = value
    cd, s, stats = dr.despike(accum, feat["ids"])
    assert all(s[y, x] == 1 and cd[y, x].tobytes() == accum[y, x].tobytes() for y, x in lone) and stats["count"] > 0
    want, want_var, stats = reference(orc, feat, accum, moments, "variance", 1)
    ctx.write_texture(TEX, accum)
    ctx.write_moments(moments)
    ctx.denoise_guided(1, *SIGMAS, flags=MODES["variance"])
    _compare(ctx, want, want_var, stats["count"], "alone in its class", same=pc.same_bits_or_nan)
