"""The firefly pre-pass of the guided de-noise on the CPU (include/mi3pt.h: mi3pt_set_guided_despike): tests/guided_despike_reference.py,
the numpy restatement the kernel is held to, checked against an independent scalar walk through the header's lines, on its limits (a
smooth image, a lone class, non-finite texels) and on the use case -- the sun of the hosts' default environment, whose fireflies the
fixed-sigma filter keeps."""
import math

import numpy as np

import aov_reference as ar
import guided_despike_reference as dr
import guided_reference as gr
import moments_reference as mr
import ptcommon as pc
from mi3pt_host import scenes

F = np.float32
SIGMAS = (2.0, 0.35, 0.1, 0.05)


def _ids(mat, hit=None):
    mat = np.asarray(mat, np.int32)
    ids = np.zeros(mat.shape + (4,), np.int32)
    ids[..., 1] = mat
    ids[..., 2] = 1 if hit is None else hit
    return ids


def _scalar_law(C, ids):
    """the header's lines for one texel after the other, numpy fp32 scalars: independent of guided_despike_reference's canvas"""
    rows, w = C.shape[:2]
    third = F(1) / F(3)
    lum = lambda t: ((t[0] + t[1]) + t[2]) * third
    out, S, M = C.copy(), np.ones((rows, w), F), np.zeros((rows, w), int)
    with np.errstate(all="ignore"):
        for y in range(rows):
            for x in range(w):
                cap, m = F(0), 0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        qx, qy = x + dx, y + dy
                        if (dx == 0 and dy == 0) or not (0 <= qx < w and 0 <= qy < rows):
                            continue
                        if ids[qy, qx, 1] != ids[y, x, 1] or ids[qy, qx, 2] != ids[y, x, 2]:
                            continue
                        m += 1
                        lq = lum(C[qy, qx])
                        cap = cap if np.isnan(lq) else (lq if lq > cap else cap)           # fmaxf from 0: drops a NaN
                M[y, x] = m
                lp = lum(C[y, x])
                if m >= 1 and lp > cap:
                    S[y, x] = cap / lp
                    for k in range(3):
                        out[y, x, k] = C[y, x, k] * S[y, x]
    return out, S, M


def test_the_reference_is_the_headers_law_texel_by_texel():
    rng = np.random.default_rng(20261020)
    rows, w = 9, 13
    C = (rng.random((rows, w, 4), dtype=F) * F(4)).astype(F)
    spikes = rng.random((rows, w)) < 0.15
    C[spikes, :3] *= F(40)
    ids = _ids(rng.integers(0, 3, (rows, w)), rng.integers(0, 2, (rows, w)))
    out, s, stats = dr.despike(C, ids)
    want, want_s, m = _scalar_law(C, ids)
    assert pc.same_bits(out, want) and pc.same_bits(s, want_s)
    assert stats["count"] == int((want_s != 1).sum()) and 0.01 < stats["clamped"] < 0.4
    assert stats["lone"] == float((m == 0).mean()) and stats["m_min"] == m.min()
    assert pc.same_bits(out[..., 3], C[..., 3])


def test_a_smooth_image_is_returned_bit_for_bit(orc):
    """c a function of the feature class alone: every counting tap equals the centre, no L(p) > cap; the three modes return the bits of
    their references without the pre-pass"""
    rng = np.random.default_rng(3)
    rows, w = 12, 20
    mat, hit = rng.integers(0, 4, (rows, w)), rng.integers(0, 2, (rows, w))
    palette = (rng.random((8, 4), dtype=F) * F(4)).astype(F)
    C = palette[mat * 2 + hit]
    ids = _ids(mat, hit)
    out, s, stats = dr.despike(C, ids)
    assert out.tobytes() == C.tobytes() and np.all(s == 1) and stats["count"] == 0 and stats["clamped"] == 0.0
    feat = [(rng.random((rows, w, 4), dtype=F)).astype(F) for _ in range(3)]
    moments = (rng.random((rows, w, 4), dtype=F) * F(8)).astype(F)
    moments[..., 3] = rng.integers(1, 9, (rows, w))
    plain = gr.guided(orc, C, *feat, ids, 2, *SIGMAS)[0]
    assert dr.guided(orc, C, *feat, ids, 2, *SIGMAS)[0].tobytes() == plain.tobytes()
    want = mr.guided_variance(orc, C, moments, *feat, ids, 2, *SIGMAS)
    got = dr.guided_variance(orc, C, moments, *feat, ids, 2, *SIGMAS)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_a_planted_spike_is_clamped_to_its_largest_neighbour_of_its_class():
    C = np.ones((5, 5, 4), F)
    C[..., 3] = F(0.25)
    C[2, 2, :3] = (F(90), F(30), F(60))          # L = 60
    C[1, 1, :3] = F(3)                            # the largest neighbour of the class
    C[1, 2, :3] = F(500)                          # brighter, but another material
    C[3, 3, :3] = F(400)                          # brighter, but a miss
    mat, hit = np.zeros((5, 5), int), np.ones((5, 5), int)
    mat[1, 2] = 7
    hit[3, 3] = 0
    out, s, stats = dr.despike(C, _ids(mat, hit))
    assert s[2, 2] == F(3) / F(60) and stats["count"] == 1
    assert pc.same_bits(out[2, 2], [F(90) * s[2, 2], F(30) * s[2, 2], F(60) * s[2, 2], F(0.25)])
    assert dr.luminance(out)[2, 2] == F(3)
    keep = np.ones((5, 5), bool)
    keep[2, 2] = False
    assert out[keep].tobytes() == C[keep].tobytes() and np.all(s[keep] == 1)
    # the variance of a scaled variable
    var0 = np.full((5, 5), 2, F)
    scaled = dr._scaled(var0, s)
    assert scaled[2, 2] == F(2) * (s[2, 2] * s[2, 2]) and np.all(scaled[keep] == 2)


def test_a_spike_without_a_neighbour_of_its_class_is_left_alone():
    C = np.ones((3, 3, 4), F)
    C[1, 1, :3] = F(1000)
    mat = np.zeros((3, 3), int)
    mat[1, 1] = 5                                 # a small emitter in front of a wall
    out, s, stats = dr.despike(C, _ids(mat))
    assert out.tobytes() == C.tobytes() and np.all(s == 1) and stats["lone"] == 1 / 9 and stats["m_min"] == 0
    # one texel: no tap at all
    one = np.full((1, 1, 4), 7, F)
    out, s, stats = dr.despike(one, _ids(np.zeros((1, 1), int)))
    assert out.tobytes() == one.tobytes() and stats["lone"] == 1.0 and stats["count"] == 0


def test_two_adjacent_spikes_cap_each_other():
    C = np.ones((4, 5, 4), F)
    C[1, 1, :3], C[1, 2, :3] = F(50), F(80)
    out, s, stats = dr.despike(C, _ids(np.zeros((4, 5), int)))
    assert stats["count"] == 1 and s[1, 1] == 1 and s[1, 2] == F(50) / F(80)          # the brighter one comes down to the other, no further
    assert dr.luminance(out)[1, 2] >= F(50) * (1 - 2 ** -22) and out[1, 1].tobytes() == C[1, 1].tobytes()


def test_non_finite_texels_follow_the_comparisons_as_written():
    base = np.ones((3, 3, 4), F)
    ids = _ids(np.zeros((3, 3), int))
    with np.errstate(all="ignore"):
        c = base.copy()
        c[1, 1, 0] = np.nan                        # a NaN centre: L(p) > cap is false
        out, s, _ = dr.despike(c, ids)
        assert s[1, 1] == 1 and np.isnan(out[1, 1, 0]) and out[1, 1, 1:].tobytes() == c[1, 1, 1:].tobytes()
        assert np.all(s == 1)                      # and as a neighbour it is dropped by fmaxf: nobody is clamped to it or by it
        c = base.copy()
        c[1, 1, :3] = np.inf                       # a +inf centre over a finite cap: s = 0, c' = inf * 0 = NaN
        out, s, stats = dr.despike(c, ids)
        assert s[1, 1] == 0 and np.isnan(out[1, 1, :3]).all() and out[1, 1, 3] == 1 and stats["count"] == 1
        c = base.copy()
        c[0, 0, 1] = np.nan                        # a NaN neighbour of a spike: the cap comes from the others
        c[1, 1, :3] = F(9)
        c[2, 2, :3] = F(3)
        out, s, stats = dr.despike(c, ids)
        assert s[1, 1] == F(3) / F(9) and stats["count"] == 1
        c = base.copy()
        c[0, 0, :3], c[1, 1, :3] = np.inf, np.inf  # two +inf texels: inf > inf is false for both
        out, s, stats = dr.despike(c, ids)
        assert stats["count"] == 0 and out.tobytes() == c.tobytes()


# ---- the use case ----
def _tone_rmse(x, truth):
    a = np.asarray(x, np.float64)[..., :3]
    b = np.asarray(truth, np.float64)[..., :3]
    return float(np.sqrt((((a / (1 + a)) - (b / (1 + b))) ** 2).mean()))


def test_with_the_sun_the_fixed_sigma_filter_is_better_behind_the_pre_pass(orc, demo):
    """Demo scene, 48 x 32, four bounces, scenes.synthetic_env() with its sun, the mean of 16 frames against a 1 024-frame mean,
    tone-mapped RMSE over every texel, three levels, sigma_color 2 / sqrt(16).  Measured: un-filtered 0.0515, guided 0.0507, behind the
    pre-pass 0.0308 -- ratio 0.607, 10.6 % of the texels clamped, none without a tap (at 96 x 64 against 3 000 frames the prototype,
    which compared hit flags alone, had 0.53)."""
    w, h, frames = 48, 32, 16
    osc = pc.oracle_scene(orc, demo, scenes.synthetic_env())
    un = lambda frame: pc.rt_uniforms(demo, w, h, frame=frame, bounces=4).tobytes()
    truth = np.zeros((h, w, 4), np.float64)
    for f in range(1000, 2024):
        truth += orc.raytrace(osc, un(f), w, h)[0]
    truth /= 1024
    mean = np.zeros((h, w, 4), np.float64)
    for f in range(2, 2 + frames):
        mean += orc.raytrace(osc, un(f), w, h)[0]
    mean = (mean / frames).astype(F)
    feat = ar.reference(orc, osc, un(0), w, h)
    args = (feat["normal"], feat["position"], feat["albedo"], feat["ids"], 3, SIGMAS[0] / math.sqrt(frames), *SIGMAS[1:])
    plain = gr.guided(orc, mean, *args)[0]
    out, _, _, stats = dr.guided(orc, mean, *args)
    e_raw, e_plain, e_despiked = _tone_rmse(mean, truth), _tone_rmse(plain, truth), _tone_rmse(out, truth)
    print(f"16 frames with the sun: un-filtered {e_raw:.4f}, guided {e_plain:.4f}, behind the pre-pass {e_despiked:.4f}: ratio "
          f"{e_despiked / e_plain:.3f}; {100 * stats['clamped']:.1f} % of the texels clamped, {100 * stats['lone']:.1f} % without a tap")
    assert e_despiked < e_plain
