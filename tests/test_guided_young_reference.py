"""MI3PT_GUIDED_YOUNG on the CPU (include/mi3pt.h): tests/guided_young_reference.py, the numpy restatement the kernel is held to, checked
against an independent scalar walk through the header's lines, against float64 statistics of explicit sample sets, on its two limits
(no young texel; one sample everywhere), on the order of its sums, and on the use case -- texels of very different age side by side
after a reset and after a reprojection, with the oracle's renderer."""
import numpy as np
import pytest

import aov_reference as ar
import guided_young_reference as yr
import moments_reference as mr
import ptcommon as pc
import reproject_reference as rr
from mi3pt_host import scenes

F = np.float32
SIGMAS = (2.0, 0.35, 0.1, 0.05)
BELOW_ONE, BELOW_FOUR = np.nextafter(F(1), F(0)), np.nextafter(F(4), F(0))


def _exp(orc, x):
    return orc.math_fn(4, np.array([x], F))[0]


def _scalar_law(orc, C, M, Nn, P, Al, hit, sn, sa, sp):
    """the header's lines for one texel after the other, numpy fp32 scalars, no arrays: independent of guided_young_reference's canvas"""
    rows, w = hit.shape
    one, zero, two, four = F(1), F(0), F(2), F(4)
    inv = lambda s: zero if F(s) == 0 else one / (F(s) * F(s))
    inv_n, inv_a, inv_p = inv(sn), inv(sa), inv(sp)
    g = [F(0.25), F(0.5), F(0.25)]
    out = np.zeros((rows, w), F)

    def sq3(a, b):
        d = [a[k] - b[k] for k in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]

    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(w):
                n_p = M[y, x, 3]
                if not n_p < four:                                   # not young (a NaN count included): the 3 x 3, young taps left out
                    num = den = zero
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            qx, qy = x + dx, y + dy
                            if not (0 <= qx < w and 0 <= qy < rows) or hit[qy, qx] != hit[y, x]:
                                continue
                            m2, n = M[qy, qx, :3], M[qy, qx, 3]
                            if (dx or dy) and n < four:
                                continue
                            v = np.fmax(((m2[0] + m2[1]) + m2[2]) / (n * (n - one)), zero) if n >= two else zero
                            wgt = g[dx + 1] * g[dy + 1]
                            num = num + wgt * v
                            den = den + wgt
                    out[y, x] = num / den
                    continue
                if n_p < one:
                    out[y, x] = zero
                    continue
                taps = []
                N, A = zero, [zero] * 3
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        qx, qy = x + dx, y + dy
                        if not (0 <= qx < w and 0 <= qy < rows) or hit[qy, qx] != hit[y, x] or not M[qy, qx, 3] >= one:
                            continue
                        if dx or dy:
                            en = sq3(Nn[qy, qx], Nn[y, x]) * inv_n
                            ea = sq3(Al[qy, qx], Al[y, x]) * inv_a
                            dP = [P[qy, qx, k] - P[y, x, k] for k in range(3)]
                            pd = (Nn[y, x, 0] * dP[0] + Nn[y, x, 1] * dP[1]) + Nn[y, x, 2] * dP[2]
                            ep = (pd * pd) * inv_p
                            wq = _exp(orc, -((en + ea) + ep))
                        else:
                            wq = one
                        a = wq * M[qy, qx, 3]
                        N = N + a
                        A = [A[k] + a * C[qy, qx, k] for k in range(3)]
                        taps.append((qx, qy, wq))
                mu = [A[k] / N for k in range(3)]
                SS = zero
                for qx, qy, wq in taps:
                    d2 = sq3(C[qy, qx], mu)
                    s_q = (M[qy, qx, 0] + M[qy, qx, 1]) + M[qy, qx, 2]
                    SS = SS + wq * (s_q + M[qy, qx, 3] * d2)
                v = np.fmax(SS / (N - one), zero) if N >= two else zero
                out[y, x] = (v / n_p) * (four / n_p)
    return out


def _synthetic(rows, w, seed):
    """seeded images with taps on both sides of every rule: two hit classes in patches, a handful of normals / albedos / depths (weights
    of exactly 1, in between, and 0), counts on either side of 1 and of 4"""
    rng = np.random.default_rng(seed)
    C = (rng.random((rows, w, 4), dtype=F) * F(4)).astype(F)
    normals = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [0, 0.28, 0.96]], F)
    Nn = np.zeros((rows, w, 4), F)
    Nn[..., :3] = normals[rng.integers(0, 4, (rows, w)) * (rng.random((rows, w)) < 0.4)]
    P = np.zeros((rows, w, 4), F)
    ys, xs = np.mgrid[0:rows, 0:w]
    P[..., 0], P[..., 1] = xs * F(0.125), ys * F(0.125)
    P[..., 2] = (rng.integers(0, 3, (rows, w)) * (rng.random((rows, w)) < 0.3) * F(0.03125)).astype(F)
    Al = np.zeros((rows, w, 4), F)
    Al[..., :3] = (rng.integers(0, 3, (rows, w, 1)) * (rng.random((rows, w, 1)) < 0.3) * F(0.0625) + F(0.5)).astype(F)
    ids = np.zeros((rows, w, 4), np.int32)
    ids[..., 2] = (((xs // 4) + (ys // 3)) % 3 != 0) ^ (rng.random((rows, w)) < 0.05)
    counts = np.array([0, 0.5, BELOW_ONE, 1, 1, 1.5, 2, 3, BELOW_FOUR, 4, 4, 64, np.nan], F)
    M = (rng.random((rows, w, 4), dtype=F) * F(24)).astype(F)
    M[..., 3] = counts[rng.integers(0, len(counts), (rows, w))]
    M[..., :3] = np.where((M[..., 3:] >= 2) | (rng.random((rows, w, 1)) < 0.2), M[..., :3], 0)
    return C, M, Nn, P, Al, ids


@pytest.mark.parametrize("rows,w,seed,sigmas", [(11, 13, 1, SIGMAS[1:]), (5, 9, 2, SIGMAS[1:]), (2, 3, 3, SIGMAS[1:]), (1, 1, 4, SIGMAS[1:]),
                                                (9, 10, 5, (0.0, 0.0, 0.0)), (9, 10, 6, (0.0, 0.1, 0.0))])
def test_the_reference_is_the_header_line_by_line(orc, rows, w, seed, sigmas):
    C, M, Nn, P, Al, ids = _synthetic(rows, w, seed)
    if seed == 1:
        # N just below and at 2: a lone n = 1.5 and a pair of n = 1 at weight 1, each walled in by the other hit class
        ids[0:3, 0:4, 2] = 0
        ids[1, 1, 2] = ids[1, 2, 2] = 7
        M[1, 1], M[1, 2] = (0, 0, 0, 1), (0, 0, 0, 1)
        Al[1, 1:3], P[1, 1:3, 2] = Al[1, 1], 0
        Nn[1, 1:3, :3] = (0, 1, 0)                                    # (dP runs along x: the plane term is 0 too)
        ids[6:9, 6:9, 2] = 0
        ids[7, 7, 2] = 9
        M[7, 7] = (1, 2, 3, 1.5)
    if rows == w == 1:
        M[0, 0] = (5, 6, 7, 1)                                            # one texel with one sample: N = 1, nothing to pool
    want = _scalar_law(orc, C, M, Nn, P, Al, ids[..., 2], *sigmas)
    got, stats = yr.initial_variance_young(orc, C, M, Nn, P, Al, ids, *sigmas)
    assert pc.same_bits_or_nan(got, want), pc.describe_diff(got, want)
    v, N, _ = yr.pooled_variance(orc, C, M, Nn, P, Al, ids, *sigmas)
    n = M[..., 3]
    if seed == 1:
        # both sides of every rule were met
        hit = ids[..., 2]
        assert N[1, 1] == 2 and N[1, 2] == 2 and got[1, 1] > 0 and N[7, 7] == F(1.5) and got[7, 7] == 0
        assert (hit[:, 1:] != hit[:, :-1]).any() and (hit[:, 1:] == hit[:, :-1]).any()
        for value in (BELOW_ONE, F(1), BELOW_FOUR, F(4)):
            assert (n == value).any(), value
        assert (n[0] < 4).any() and (n[-1] < 4).any() and (n[:, 0] < 4).any() and (n[:, -1] < 4).any()        # young texels on every border
        assert 0.02 < stats["young_rejected"] < 0.98 and stats["young_below"] > 0.02 and stats["young_above"] > 0.02
        assert 0 < stats["young"] < 1 and 0 < stats["young_lone"] < 1
    if rows == w == 1:
        assert N[0, 0] == 1 and got[0, 0] == 0


def test_the_pool_is_the_sample_variance_of_the_union():
    """Identical features (every w = 1), integer counts 1 .. 6 per texel, explicit samples per texel folded into (mean, M2, n) by
    reproject_reference.by_count_step: SS / (N - 1) is the float64 sample variance, summed over rgb, of all the samples in the window.
    Tolerance 4e-5 relative, from the fp32 roundings, u = 2^-24, samples in [0, 4), per-sample variance 3 x 16 / 12 = 4:
    every texel's mean and M2 carry at most 6 steps x 4 operations = 24 u; N, A and SS are sums of at most 49 non-negative terms of at most
    8 operations each: 57 u, so the pooled mean is off by at most delta = 4 x (57 + 24) u = 1.9e-5, which moves the sum of n_q |c_q - mu|^2
    by at most N delta (2 max|d| + delta) = N x 1.5e-4 against SS of about 4 N: 3.9e-5 (a bound: to first order the shift cancels, sum of
    n_q d_q = 0); the sums themselves add (57 + 24 + 1) u = 4.9e-6.  Measured: 2.6e-7."""
    class NoExp:
        @staticmethod
        def math_fn(fn, x):
            assert fn == 4 and not np.any(x)          # every exponent is -0: the features are identical
            return np.ones_like(x)

    rng = np.random.default_rng(11)
    rows, w, most = 12, 15, 6
    count = rng.integers(1, most + 1, (rows, w))
    samples = rng.random((most, rows, w, 3)) * 4
    mean, moments = np.zeros((rows, w, 4), F), np.zeros((rows, w, 4), F)
    for k in range(most):
        c = np.concatenate([samples[k], np.ones((rows, w, 1))], axis=-1).astype(F)
        mean, moments = rr.by_count_step(mean, moments, c, inside=count > k)
    assert np.array_equal(moments[..., 3], count)
    samples = samples.astype(F).astype(np.float64)                    # (the samples as the steps saw them)
    flat = np.zeros((rows, w, 4), F)
    ids = np.ones((rows, w, 4), np.int32)
    v, N, _ = yr.pooled_variance(NoExp, mean, moments, flat, flat, flat, ids, 0.35, 0.1, 0.05)
    worst = 0.0
    for y in range(rows):
        for x in range(w):
            y0, y1, x0, x1 = max(0, y - 3), min(rows, y + 4), max(0, x - 3), min(w, x + 4)
            union = np.concatenate([samples[:count[qy, qx], qy, qx] for qy in range(y0, y1) for qx in range(x0, x1)])
            assert N[y, x] == len(union)
            worst = max(worst, abs(v[y, x] / union.var(axis=0, ddof=1).sum() - 1))
    print(f"pooled variance against the union's: worst relative difference {worst:.3g}")
    assert worst <= 4e-5


def _demo_features(orc, demo, w, h):
    osc = pc.oracle_scene(orc, demo, scenes.synthetic_env())
    return ar.reference(orc, osc, pc.rt_uniforms(demo, w, h).tobytes(), w, h)


def _seeded(w, h, n):
    accum = (np.random.default_rng(20261018).random((h, w, 4), dtype=F) * F(4)).astype(F)
    moments = (np.random.default_rng(20261019).random((h, w, 4), dtype=F) * F(24)).astype(F)
    moments[..., 3] = F(n)
    return accum, moments


def test_no_young_texel_is_the_variance_mode_and_one_sample_everywhere_is_not_zero(orc, demo):
    w, h = 40, 24
    feat = _demo_features(orc, demo, w, h)
    args = (feat["normal"], feat["position"], feat["albedo"], feat["ids"], 3) + SIGMAS
    accum, moments = _seeded(w, h, 4)
    plain = mr.guided_variance(orc, accum, moments, *args)
    young = yr.guided_variance_young(orc, accum, moments, *args)
    assert pc.same_bits(young[0], plain[0]) and pc.same_bits(young[1], plain[1])
    assert young[2]["young"] == 0 and young[2]["young_taps"] == 0 and {k: young[2][k] for k in plain[2]} == plain[2]
    assert mr.initial_variance is not None and mr.guided_variance(orc, accum, moments, *args)[1].tobytes() == plain[1].tobytes()
    # n = 1, M2 = 0 everywhere: today var_0 = 0; with the flag it is the spread of the neighbours' means wherever two of them pool
    moments[..., :3], moments[..., 3] = 0, 1
    assert not mr.initial_variance(moments, feat["ids"][..., 2]).any()
    var0, stats = yr.initial_variance_young(orc, accum, moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"], *SIGMAS[1:])
    _, N, _ = yr.pooled_variance(orc, accum, moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"], *SIGMAS[1:])
    assert stats["young"] == 1.0 and stats["young_lone"] < 0.05
    assert (var0[N >= 2] > 0).all() and not var0[N < 2].any() and (N >= 2).mean() > 0.95
    out, var, _ = yr.guided_variance_young(orc, accum, moments, *args)
    raw = mr.guided_variance(orc, accum, moments, *args)[0]
    assert pc.same_bits(raw[..., :3], accum[..., :3]) or np.abs(raw - accum).max() < 1e-6      # today: the filter leaves such an image raw
    assert np.abs(out[..., :3] - accum[..., :3]).mean() > 0.1                                   # with the flag it filters


def test_the_tap_order_is_the_sums_order():
    """A 7 x 7 image of one class at weight 1 and n = 1, every colour equal (d = 0: a tap adds its s alone).  The first four taps of the
    centre's window hold s = 2^24, 1, -2^24, 1: ((2^24 + 1) - 2^24) + 1 = 1 in fp32 in the header's order, dy outer and dx inner; any
    order that adds the two small terms first, or the columns first, gives 2 or 0.  Likewise a count of 2^24 at the first tap: N."""
    class NoExp:
        math_fn = staticmethod(lambda fn, x: np.ones_like(x))

    accum = np.full((7, 7, 4), 1.5, F)
    moments = np.zeros((7, 7, 4), F)
    moments[..., 3] = 1
    moments[0, 0:4, 0] = (2.0 ** 24, 1, -2.0 ** 24, 1)
    flat, ids = np.zeros((7, 7, 4), F), np.ones((7, 7, 4), np.int32)
    v, N, _ = yr.pooled_variance(NoExp, accum, moments, flat, flat, flat, ids)
    assert N[3, 3] == 49 and v[3, 3] == F(1) / F(48)
    var0, _ = yr.initial_variance_young(NoExp, accum, moments, flat, flat, flat, ids)
    assert var0[3, 3] == (F(1) / F(48)) * F(4)
    moments[..., :3] = 0
    moments[0, 0, 3] = 2.0 ** 24
    _, N, _ = yr.pooled_variance(NoExp, accum, moments, flat, flat, flat, ids)
    assert N[3, 3] == F(2.0 ** 24)                       # 2^24 first: every 1 after it is rounded away; the ones first would give 2^24 + 48


# ---- the use case ----
def _tone_rmse(x, truth, sel):
    a = np.asarray(x, np.float64)[..., :3][sel]
    b = np.asarray(truth, np.float64)[..., :3][sel]
    return float(np.sqrt((((a / (1 + a)) - (b / (1 + b))) ** 2).mean()))


ORBIT_DEGREES = 8.0


def test_young_texels_are_filtered_after_a_reset_and_after_a_camera_move(orc, demo):
    """48 x 32, four bounces, the sun-less sky of test_reproject_reference.py, a 1 024-frame yardstick of view B, tone-mapped RMSE over
    B's hit texels, three levels, sigma 2 / 0.35 / 0.1 / 0.05.
    1. One frame of view B after a reset: with the flag 0.0253, the variance flag alone 0.0957 (= the raw image).
    2. 64 frames in view A, an 8 degree orbit, reproject (maxHistory 64), + 1 frame: over the 98 young of the 1 171 hit texels (0.084)
       with the flag 0.0317, without 0.1056; over the carried ones 0.01120 against 0.01125 (ratio 0.996: printed, not asserted)."""
    w, h = 48, 32
    osc = pc.oracle_scene(orc, demo, scenes.synthetic_env(sun_radiance=0.0))
    cam = demo.camera
    pos_b, dir_b = rr.orbit(cam["position"], cam["target"], ORBIT_DEGREES)
    ua = lambda frame: pc.rt_uniforms(demo, w, h, frame=frame, bounces=4)
    ub = lambda frame: pc.rt_uniforms(demo, w, h, frame=frame, bounces=4, position=pos_b, direction=dir_b)
    truth = np.zeros((h, w, 4), np.float64)
    for f in range(1000, 2024):
        truth += orc.raytrace(osc, ub(f).tobytes(), w, h)[0]
    truth /= 1024
    feat_a = ar.reference(orc, osc, ua(0).tobytes(), w, h)
    feat_b = ar.reference(orc, osc, ub(0).tobytes(), w, h)
    hit_b = feat_b["ids"][..., 2] == 1
    filt = lambda fn, a, m: fn(orc, a, m, feat_b["normal"], feat_b["position"], feat_b["albedo"], feat_b["ids"], 3, *SIGMAS)[0]
    fresh = orc.raytrace(osc, ub(66).tobytes(), w, h)[0]
    # 1. one frame after a reset
    a1, m1 = rr.by_count_step(np.zeros((h, w, 4), F), np.zeros((h, w, 4), F), fresh)
    e_raw, e_plain, e_young = (_tone_rmse(x, truth, hit_b) for x in (a1, filt(mr.guided_variance, a1, m1), filt(yr.guided_variance_young, a1, m1)))
    print(f"one frame after a reset: raw {e_raw:.5f}, variance flag alone {e_plain:.5f}, with the young flag {e_young:.5f}")
    assert e_young < e_plain
    # 2. a carried history with disoccluded texels in it
    mean, moments = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    for k in range(64):
        mean, moments = rr.by_count_step(mean, moments, orc.raytrace(osc, ua(2 + k).tobytes(), w, h)[0])
    a, m, info = rr.reproject(mean, moments, rr.view_frame(ua(0).tobytes()), (F(w), F(h)), feat_b, feat_a, (w, h), max_history=64)
    a, m = rr.by_count_step(a, m, fresh)
    young = hit_b & (m[..., 3] < 4)
    carried = hit_b & ~young
    share = young.sum() / hit_b.sum()
    plain, with_flag = filt(mr.guided_variance, a, m), filt(yr.guided_variance_young, a, m)
    y_plain, y_flag = _tone_rmse(plain, truth, young), _tone_rmse(with_flag, truth, young)
    c_plain, c_flag = _tone_rmse(plain, truth, carried), _tone_rmse(with_flag, truth, carried)
    print(f"after the orbit + 1 frame: {int(young.sum())} of {int(hit_b.sum())} hit texels young ({share:.3f}); young: flag alone {y_plain:.5f}, "
          f"with the young flag {y_flag:.5f}; carried: {c_plain:.5f} / {c_flag:.5f}, ratio {c_flag / c_plain:.4f}")
    assert share >= 0.02
    assert y_flag < y_plain
