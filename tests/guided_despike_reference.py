"""Reference for the firefly pre-pass of the guided de-noise (mi3pt_set_guided_despike), written from the header comment of
include/mi3pt.h: the image c' the filter reads in the accumulation image's place, the scale s per texel, and the three modes on top of
guided_reference.py, moments_reference.py and guided_young_reference.py.

numpy fp32, one operation per line of the definition (numpy neither contracts nor reassociates; fp32 `/` is correctly rounded).  The cap's
fmaxf is written as a comparison: it starts at +0 and is never a NaN, so `L(q) > cap ? L(q) : cap` drops a NaN as fmaxf does and keeps +0
against a -0, as the header pins it -- np.fmax(+0, -0) is -0 in numpy's vector loops and +0 in its scalar one.  Nothing here looks at
the device.  No test lives in this file.
"""
import numpy as np

import guided_reference as gr
import guided_young_reference as yr
import moments_reference as mr
from guided_reference import _shift

THIRD = np.float32(1.0) / np.float32(3.0)


def _class_of(ids):
    """words 1 and 2 of the ids image: material and hit flag"""
    words = np.ascontiguousarray(ids)
    words = words if words.dtype == np.int32 else words.view(np.int32)
    return words[..., 1], words[..., 2]


def luminance(c):
    with np.errstate(all="ignore"):
        t = c[..., 0] + c[..., 1]
        t = t + c[..., 2]
        return t * THIRD


def despike(accum, ids):
    """Returns (c' (rows, w, 4) float32, s (rows, w) float32, stats).  stats: "clamped" the share of clamped texels, "count" their number,
    "lone" the share of texels without a counting tap (m == 0), "m_min" the smallest m in the image."""
    c = np.ascontiguousarray(accum, np.float32)
    mat, hit = _class_of(ids)
    rows, w = c.shape[:2]
    L = luminance(c)
    inside_all = np.ones((rows, w), bool)
    m = np.zeros((rows, w), np.int32)
    cap = np.zeros((rows, w), np.float32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            if dy == 0 and dx == 0:
                continue
            counts = _shift(inside_all, dy, dx, False) & (_shift(mat, dy, dx) == mat) & (_shift(hit, dy, dx) == hit)
            m = m + counts
            with np.errstate(invalid="ignore"):
                cap = np.where(counts & (_shift(L, dy, dx) > cap), _shift(L, dy, dx), cap)          # fmaxf from +0 (see above)
    with np.errstate(all="ignore"):
        clamped = (m >= 1) & (L > cap)
        s = np.where(clamped, cap / L, np.float32(1)).astype(np.float32)
        out = c.copy()
        for k in range(3):
            out[..., k] = np.where(clamped, c[..., k] * s, c[..., k])
    stats = {"clamped": float(clamped.mean()), "count": int(clamped.sum()), "lone": float((m == 0).mean()), "m_min": int(m.min())}
    return out, s, stats


def _scaled(var0, s):
    """var_0(p) * (s * s) for the clamped texels (s != 1: a clamped texel's cap / L lies below 1), var_0's own bits elsewhere"""
    with np.errstate(all="ignore"):
        ss = s * s
        return np.where(s != np.float32(1), var0 * ss, var0).astype(np.float32)


def _levels_on(var0, orc, accum, moments, normal, position, albedo, ids, levels, sigmas):
    """moments_reference.guided_variance's level loop on a given var_0 (guided_young_reference.guided_variance_young's way)"""
    plain = mr.initial_variance
    mr.initial_variance = lambda _moments, _hit: var0
    try:
        return mr.guided_variance(orc, accum, moments, normal, position, albedo, ids, levels, *sigmas)
    finally:
        mr.initial_variance = plain


def guided(orc, accum, normal, position, albedo, ids, levels=3, sigma_color=1.0, sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.05):
    """guided_reference.guided behind the pre-pass.  Returns (filtered, c', s, stats): guided's stats and despike's."""
    cd, s, dstats = despike(accum, ids)
    out, stats = gr.guided(orc, cd, normal, position, albedo, ids, levels, sigma_color, sigma_normal, sigma_albedo, sigma_plane)
    stats = dict(stats)
    stats.update(dstats)
    return out, cd, s, stats


def guided_variance(orc, accum, moments, normal, position, albedo, ids, levels=3, sigma_color=2.0, sigma_normal=0.35, sigma_albedo=0.1,
                    sigma_plane=0.05, young=False):
    """moments_reference.guided_variance (young: guided_young_reference.guided_variance_young) behind the pre-pass: var_0 exactly as
    there -- the young texels' pool reads c' --, times s * s for the clamped texels.  Returns (filtered, variance after the last level,
    c', s, stats)."""
    cd, s, dstats = despike(accum, ids)
    _, hit = _class_of(ids)
    if young:
        var0, ystats = yr.initial_variance_young(orc, cd, moments, normal, position, albedo, ids, sigma_normal, sigma_albedo, sigma_plane)
    else:
        var0, ystats = mr.initial_variance(moments, hit), {}
    sigmas = (sigma_color, sigma_normal, sigma_albedo, sigma_plane)
    out, var, stats = _levels_on(_scaled(var0, s), orc, cd, moments, normal, position, albedo, ids, levels, sigmas)
    stats = dict(stats)
    stats.update(ystats)
    stats.update(dstats)
    return out, var, cd, s, stats
