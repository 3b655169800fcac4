"""Reference for MI3PT_GUIDED_YOUNG (mi3pt_denoise_guided with MI3PT_GUIDED_VARIANCE | MI3PT_GUIDED_YOUNG), written from the header
comment of include/mi3pt.h: the initial variance of an image whose texels differ in age.  The levels are moments_reference.py's.

numpy fp32, one operation per line of the definition (numpy neither contracts nor reassociates; fp32 `/` is correctly rounded), with
pt_oracle.math_fn(4, .) for exp.  Nothing here looks at the device.  No test lives in this file.
"""
import numpy as np

import moments_reference as mr
from guided_reference import _shift, _sq3, inv_sigma

YOUNG_COUNT = np.float32(4)       # MI3PT_GUIDED_YOUNG_COUNT
R = 3                             # the young texels' window: 7 x 7


def _hit_of(ids):
    words = np.ascontiguousarray(ids)
    return (words if words.dtype == np.int32 else words.view(np.int32))[..., 2]


def settled_variance(moments, hit):
    """var_0 of the texels that are not young: moments_reference.initial_variance with the young taps left out (the centre always counts)"""
    m = np.asarray(moments, np.float32)
    v = mr.variance_of_mean(m)
    with np.errstate(invalid="ignore"):
        young = m[..., 3] < YOUNG_COUNT
    rows, w = v.shape
    inside_all = np.ones((rows, w), bool)
    num = np.zeros((rows, w), np.float32)
    den = np.zeros((rows, w), np.float32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            counts = _shift(inside_all, dy, dx, False) & (_shift(hit, dy, dx) == hit)
            if dy or dx:
                counts &= ~_shift(young, dy, dx, False)
            wgt = mr.G3[dx + 1] * mr.G3[dy + 1]
            with np.errstate(all="ignore"):
                t = wgt * _shift(v, dy, dx)
                num = np.where(counts, num + t, num)
            den = np.where(counts, den + wgt, den)
    with np.errstate(all="ignore"):
        return num / den


def pooled_variance(orc, accum, moments, normal, position, albedo, ids, sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.05):
    """The 7 x 7 pool of EVERY texel, young or not: (v, N, tap counts) -- v = N >= 2 ? fmax(SS / (N - 1), 0) : 0, the per-sample variance
    summed over rgb of the samples the counted taps hold, and N their weighted count.  The tap counts are those of the windows around
    the young texels with n >= 1 (initial_variance_young turns them into shares)."""
    c = np.ascontiguousarray(accum, np.float32)[..., :3]
    m = np.ascontiguousarray(moments, np.float32)
    n = np.ascontiguousarray(normal, np.float32)[..., :3]
    pos = np.ascontiguousarray(position, np.float32)[..., :3]
    a = np.ascontiguousarray(albedo, np.float32)[..., :3]
    hit = _hit_of(ids)
    rows, w = c.shape[:2]
    inv_normal, inv_albedo, inv_plane = inv_sigma(sigma_normal), inv_sigma(sigma_albedo), inv_sigma(sigma_plane)
    cnt = m[..., 3]
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(all="ignore"):
        s = (m[..., 0] + m[..., 1]) + m[..., 2]
        young = cnt < YOUNG_COUNT
        sampled = cnt >= one
    pools = young & sampled                      # the centres that run the 7 x 7
    inside_all = np.ones((rows, w), bool)
    N = np.zeros((rows, w), np.float32)
    A = np.zeros((rows, w, 3), np.float32)
    weights, counted = [], []
    taps = rejected = counted_off = below = above = 0
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                inside = _shift(inside_all, dy, dx, False)
                nq = _shift(cnt, dy, dx)
                counts = inside & (_shift(hit, dy, dx) == hit) & (nq >= one)
                if dy or dx:
                    en = _sq3(_shift(n, dy, dx) - n) * inv_normal
                    ea = _sq3(_shift(a, dy, dx) - a) * inv_albedo
                    dp = _shift(pos, dy, dx) - pos
                    pd = (n[..., 0] * dp[..., 0] + n[..., 1] * dp[..., 1]) + n[..., 2] * dp[..., 2]
                    ep = (pd * pd) * inv_plane
                    wgt = orc.math_fn(4, -((en + ea) + ep))
                else:
                    wgt = np.ones((rows, w), np.float32)
                cq = _shift(c, dy, dx)
                aw = wgt * nq
                N = np.where(counts, N + aw, N)
                for k in range(3):
                    A[..., k] = np.where(counts, A[..., k] + aw * cq[..., k], A[..., k])
                weights.append(wgt)
                counted.append(counts)
                taps += int((inside & pools).sum())
                rejected += int((inside & ~counts & pools).sum())
                if dy or dx:
                    counted_off += int((counts & pools).sum())
                    below += int((counts & pools & (wgt < 0.5)).sum())
                    above += int((counts & pools & (wgt > 0.5)).sum())
        mu = np.empty_like(A)
        for k in range(3):
            mu[..., k] = A[..., k] / N
        SS = np.zeros((rows, w), np.float32)
        i = 0
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                d = _shift(c, dy, dx) - mu
                d2 = _sq3(d)
                t = _shift(s, dy, dx) + _shift(cnt, dy, dx) * d2
                SS = np.where(counted[i], SS + weights[i] * t, SS)
                i += 1
        q = SS / (N - one)
        v = np.where(N >= np.float32(2), np.fmax(q, zero), zero).astype(np.float32)
    return v, N, {"taps": taps, "rejected": rejected, "counted_off": counted_off, "below": below, "above": above}


def initial_variance_young(orc, accum, moments, normal, position, albedo, ids, sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.05):
    """var_0 under MI3PT_GUIDED_YOUNG.  Returns ((rows, w) float32, stats).  stats, over the 7 x 7 windows of the young texels with
    n >= 1 (the windows the law evaluates): "young_taps" in-image taps, "young_rejected" the share of them the hit / count rule rejects,
    "young_below" / "young_above" the shares of the counted off-centre taps whose w lies below / above 0.5; over the image: "young" the
    share of young texels, "young_lone" the share of the young texels whose pooled count N is below 2 (never sampled ones included)."""
    v, N, t = pooled_variance(orc, accum, moments, normal, position, albedo, ids, sigma_normal, sigma_albedo, sigma_plane)
    taps, rejected, counted_off, below, above = t["taps"], t["rejected"], t["counted_off"], t["below"], t["above"]
    m = np.ascontiguousarray(moments, np.float32)
    hit = _hit_of(ids)
    cnt = m[..., 3]
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(all="ignore"):
        young = cnt < YOUNG_COUNT
        sampled = cnt >= one
        pooled = (v / cnt) * (YOUNG_COUNT / cnt)
    var0 = np.where(young, np.where(sampled, pooled, zero), settled_variance(m, hit)).astype(np.float32)
    n_young = int(young.sum())
    with np.errstate(invalid="ignore"):
        lone = int((young & ~(sampled & (N >= np.float32(2)))).sum())
    stats = {"young_taps": taps, "young_rejected": rejected / taps if taps else 0.0,
             "young_below": below / counted_off if counted_off else 0.0, "young_above": above / counted_off if counted_off else 0.0,
             "young": n_young / young.size, "young_lone": lone / n_young if n_young else 0.0}
    return var0, stats


def guided_variance_young(orc, accum, moments, normal, position, albedo, ids, levels=3, sigma_color=2.0, sigma_normal=0.35, sigma_albedo=0.1,
                          sigma_plane=0.05):
    """moments_reference.guided_variance with MI3PT_GUIDED_YOUNG: its level loop on initial_variance_young's var_0.  Returns (filtered,
    variance after the last level, stats): guided_variance's stats and initial_variance_young's."""
    var0, young_stats = initial_variance_young(orc, accum, moments, normal, position, albedo, ids, sigma_normal, sigma_albedo, sigma_plane)
    # the level loop is guided_variance's own: it asks its module for var_0, and for this one call the module answers with ours
    plain = mr.initial_variance
    mr.initial_variance = lambda _moments, _hit: var0
    try:
        out, var, stats = mr.guided_variance(orc, accum, moments, normal, position, albedo, ids, levels, sigma_color, sigma_normal,
                                             sigma_albedo, sigma_plane)
    finally:
        mr.initial_variance = plain
    stats = dict(stats)
    stats.update(young_stats)
    return out, var, stats
