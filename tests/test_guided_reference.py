"""The reference of the feature-guided a-trous de-noise (tests/guided_reference.py) on the CPU: its special cases by hand, and what the
filter is for -- the error of a 1- and a 4-frame mean against a 3000-frame mean, beside the reference's own bilateral de-noiser."""
import numpy as np
import pytest

import aov_reference as ar
import guided_reference as gr
import ptcommon as pc
from mi3pt_host import scenes

F = np.float32


def _flat_features(h, w, hit=1):
    z = np.zeros((h, w, 4), np.float32)
    ids = np.zeros((h, w, 4), np.int32)
    ids[..., 2] = hit
    return z.copy(), z.copy(), z.copy(), ids


def _b3_blur(img, s):
    """the normalised 5 x 5 B3-spline blur with taps s apart, taps outside the image left out; fp32, in the filter's tap order"""
    hk = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
    h, w = img.shape[:2]
    out = img.copy()
    for y in range(h):
        for x in range(w):
            den = F(0)
            num = [F(0), F(0), F(0)]
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = y + s * dy, x + s * dx
                    if not (0 <= qy < h and 0 <= qx < w):
                        continue
                    wgt = F(1) * (hk[dx + 2] * hk[dy + 2])
                    den = den + wgt
                    for k in range(3):
                        num[k] = num[k] + wgt * img[qy, qx, k]
            for k in range(3):
                out[y, x, k] = num[k] / den
    return out


def test_all_sigmas_zero_is_a_b3_spline_blur(orc):
    h, w = 5, 7
    img = (np.random.default_rng(11).random((h, w, 4), dtype=np.float32) * 4).astype(np.float32)
    n, p, a, ids = _flat_features(h, w)
    got1, st = gr.guided(orc, img, n, p, a, ids, 1, 0.0, 0.0, 0.0, 0.0)
    want1 = _b3_blur(img, 1)
    assert pc.same_bits(got1, want1), pc.describe_diff(got1, want1)
    assert st["rejected"] == 0.0 and st["below"] == 0.0 and st["above"] == 1.0      # every counted tap has exp(-0) = 1
    got2, _ = gr.guided(orc, img, n, p, a, ids, 2, 0.0, 0.0, 0.0, 0.0)
    want2 = _b3_blur(want1, 2)
    assert pc.same_bits(got2, want2), pc.describe_diff(got2, want2)
    assert not pc.same_bits(got2, got1) and np.array_equal(got2[..., 3], img[..., 3])


def test_constant_image_stays_constant(orc, demo, env):
    """Channels that are powers of two: w * c is then exact, num = c * den to the bit whatever the weights are, and the correctly rounded
    quotient is c.  (For another constant the products round and the quotient may be an ulp off: not a property of the filter.)"""
    w, h = 40, 24
    feat = ar.reference(orc, pc.oracle_scene(orc, demo, env), pc.rt_uniforms(demo, w, h).tobytes(), w, h)
    assert 0.1 < feat["hit"].mean() < 0.9
    img = np.empty((h, w, 4), np.float32)
    img[...] = (0.5, 2.0, 0.25, 0.75)
    got, st = gr.guided(orc, img, feat["normal"], feat["position"], feat["albedo"], feat["ids"], 4, 1.0, 0.35, 0.1, 0.05)
    assert st["rejected"] > 0.02 and st["below"] > 0.02      # the weights do differ from tap to tap
    assert got.tobytes() == img.tobytes()


def test_texel_alone_in_its_hit_class_is_returned_unchanged(orc):
    """Only the centre tap counts: the result is fl(fl(9/64 * c) / (9/64)).  With c a multiple of 2^-10 below 4 the product has 16
    significant bits and is exact, so the texel comes back to the bit (a full-width fp32 value may come back an ulp off)."""
    h, w = 9, 11
    rng = np.random.default_rng(5)
    img = (rng.integers(0, 4096, (h, w, 4)).astype(np.float32) / F(1024)).astype(np.float32)
    n, p, a, ids = _flat_features(h, w, hit=0)
    lonely = [(0, 0), (4, 5), (8, 10)]
    for y, x in lonely:
        ids[y, x, 2] = 1
    got, st = gr.guided(orc, img, n, p, a, ids, 3, 1.0, 0.35, 0.1, 0.05)
    for y, x in lonely:
        assert got[y, x].tobytes() == img[y, x].tobytes()
    assert st["rejected"] > 0.0
    assert not pc.same_bits(got[1, 1], img[1, 1])            # (the others are filtered)


def test_the_size_with_several_tiles_per_stride_class(orc, demo, env):
    """264 x 260, the size at which tests/test_gpu_guided.py and tests/test_gpu_guided_variance.py run more than one block per stride
    class.  The launch arithmetic of csrc/pt_guided.hip restated: level i has s = 2^i classes per axis, class c holds the texels c, c + s,
    ... (ceil((size - c) / s) of them), and the grid has ceil(ceil(size / s) / 16) tiles of 16 per class.  And the reference's statistics
    with the ORACLE's features and the two modules' own seeded inputs, held to the bounds the GPU cases assert (measured, rejected /
    below / above: plain 0.039 / 0.114 / 0.886 at four levels and 0.059 / 0.112 / 0.888 at five, variance 0.039 / 0.719 / 0.281 and
    0.059 / 0.762 / 0.238)."""
    import moments_reference as mr
    import test_gpu_guided as gg
    import test_gpu_guided_variance as gv
    w, h = 264, 260
    assert (w, h, 4) in gg.SIZES and (w, h, 5) in gg.SIZES and (w, h, 4) in gv.SIZES and (w, h, 5) in gv.SIZES
    tile = 16
    for size in (w, h):
        for s, want in ((4, 5), (8, 3), (16, 2)):
            longest = (size + s - 1) // s
            assert (longest + tile - 1) // tile == want >= 2, (size, s)
        lengths = {len(range(c, size, 16)) for c in range(16)}
        assert lengths == {17, 16}, size                   # classes with a texel in their second tile, and classes without
    feat = ar.reference(orc, pc.oracle_scene(orc, demo, env), pc.rt_uniforms(demo, w, h).tobytes(), w, h)
    accum, moments = gg._random_accum(w, h), gv._random_moments(w, h)
    for levels in (4, 5):
        _, stats = gr.guided(orc, accum, feat["normal"], feat["position"], feat["albedo"], feat["ids"], levels, *gg.ALL_ON)
        gg._assert_not_vacuous(stats, f"plain, {levels} levels")
        _, _, stats = mr.guided_variance(orc, accum, moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"], levels, *gv.SIGMAS)
        gv._assert_not_vacuous(stats, f"variance, {levels} levels")


def _tone_rmse(x, truth):
    a = np.asarray(x, np.float64)[..., :3]
    b = np.asarray(truth, np.float64)[..., :3]
    return float(np.sqrt(np.mean((a / (1 + a) - b / (1 + b)) ** 2)))


def test_guided_filter_beats_the_bilateral_at_low_sample_counts(orc, demo):
    """The demo scene at 96 x 96 under the sun-less sky, four bounces.  Error: RMSE of x / (1 + x) over rgb against the mean of 3000
    other frames.  Ordering asserted at 1 and 4 frames: guided (default parameters, sigma_color = 2 / sqrt(frames)) < the reference's
    bilateral (oracle fullscreen, denoise 1, tone mapping 0) < un-filtered.  No number is fixed; the three errors are printed."""
    w = h = 96
    env = scenes.synthetic_env(sun_radiance=0.0)
    osc = pc.oracle_scene(orc, demo, env)
    feat = ar.reference(orc, osc, pc.rt_uniforms(demo, w, h).tobytes(), w, h)
    truth = np.zeros((h, w, 4), np.float64)
    for f in range(1000, 4000):
        truth += orc.raytrace(osc, pc.rt_uniforms(demo, w, h, frame=f, bounces=4).tobytes(), w, h)[0]
    truth /= 3000
    for frames in (1, 4):
        mean = np.zeros((h, w, 4), np.float32)
        for k in range(frames):               # (accumulate weights 1, 1/2, 1/3, 1/4: the plain mean)
            img, _ = orc.raytrace(osc, pc.rt_uniforms(demo, w, h, frame=2 + k, bounces=4).tobytes(), w, h)
            mean = orc.accumulate(pc.acc_uniforms(w, h, 1 + k).tobytes(), w, h, img, mean)
        bilateral = orc.fullscreen(pc.fs_uniforms(w, h, 1.0, denoise=1, tonemapping=0).tobytes(), mean)[0][::-1]      # (canvas row 0 = top)
        guided, _ = gr.guided(orc, mean, feat["normal"], feat["position"], feat["albedo"], feat["ids"],
                              levels=3, sigma_color=2.0 / np.sqrt(frames), sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.05)
        e_raw, e_bil, e_gui = _tone_rmse(mean, truth), _tone_rmse(bilateral, truth), _tone_rmse(guided, truth)
        print(f"{frames} frame(s): un-filtered {e_raw:.4f}  bilateral {e_bil:.4f}  guided {e_gui:.4f}")
        assert e_gui < e_bil < e_raw
