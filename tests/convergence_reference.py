"""Reference for the per-tile error estimate of the running mean (mi3pt_estimate_convergence), written from the header comment of
include/mi3pt.h.

numpy fp32, one operation per line of the definition (numpy neither contracts nor reassociates; fp32 `/` is correctly rounded).  Nothing
here looks at the device.  No test lives in this file.
"""
import math

import numpy as np

from moments_reference import variance_of_mean

FIELDS = ("tiles", "tiles_above", "tiles_young", "tiles_nonfinite", "texels", "worst_tile", "worst_texel", "n_min", "threshold")
INF = np.float32(np.inf)
THIRD = np.float32(1.0) / np.float32(3.0)


def texel_error(accum, moments):
    """(counts (rows, w) bool, r (rows, w) float32): which texels count and r(q) of every texel"""
    c = np.asarray(accum, np.float32)
    mo = np.asarray(moments, np.float32)
    with np.errstate(all="ignore"):
        counts = mo[..., 3] >= np.float32(1)
        v = variance_of_mean(mo)
        s3 = (c[..., 0] + c[..., 1]) + c[..., 2]
        s = s3 * THIRD
        m = np.where(s < np.float32(0), np.float32(0), s)         # (a NaN stays a NaN)
        d = np.float32(1) + m
        d2 = d * d
        d4 = d2 * d2
        r = v / d4
    return counts, r.astype(np.float32)


def _lanes(image, fill):
    """(rows, w) -> (tiles_y, tiles_x, 64): lane j = 8 * (row in tile) + (column in tile); outside the image: fill"""
    rows, w = image.shape
    ty, tx = (rows + 7) // 8, (w + 7) // 8
    full = np.full((ty * 8, tx * 8), fill, image.dtype)
    full[:rows, :w] = image
    return full.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty, tx, 64)


def tree_sum(lanes):
    """six halving rounds over the last axis (length 64): a[j] = a[j] + a[j + s] for j < s, s = 32, 16, 8, 4, 2, 1"""
    a = np.array(lanes, np.float32)
    with np.errstate(all="ignore"):
        for s in (32, 16, 8, 4, 2, 1):
            a = a[..., :s] + a[..., s:2 * s]
    return a[..., 0]


def tile_map(accum, moments):
    """(tiles_y, tiles_x, 4) float32: (sum_r, max_r, count, n_min) per 8 x 8 tile"""
    counts, r = texel_error(accum, moments)
    n = np.asarray(moments, np.float32)[..., 3]
    lc = _lanes(counts, False)
    lr = np.where(lc, _lanes(r, np.float32(0)), np.float32(0))
    ln = np.where(lc, _lanes(n, INF), INF)
    sum_r = tree_sum(lr)
    max_r = np.float32(0)
    n_min = INF
    for j in range(64):
        max_r = np.fmax(max_r, lr[..., j])                         # (fmax drops a NaN)
        n_min = np.fmin(n_min, ln[..., j])
    count = lc.sum(axis=-1)
    out = np.zeros(count.shape + (4,), np.float32)
    out[..., 0] = sum_r
    out[..., 1] = max_r
    out[..., 2] = count.astype(np.float32)
    out[..., 3] = n_min
    out[count == 0] = np.float32(0)
    return out


def verdict(tiles, threshold, min_frames):
    """(counted, young, above, nonfinite): bool per tile"""
    t = np.asarray(tiles, np.float32)
    th = np.float32(threshold)
    t2 = (th * th) * np.float32(3.0)
    counted = t[..., 2] > 0
    with np.errstate(all="ignore"):
        young = counted & (t[..., 3] < np.float32(min_frames))
        bound = t2 * t[..., 2]
        above = counted & (young | ~(t[..., 0] <= bound))
        nonfinite = counted & ~np.isfinite(t[..., 0])
    return counted, young, above, nonfinite


def summary(tiles, threshold, min_frames):
    """The nine fields of mi3pt_convergence as a dict (floats as np.float32)"""
    t = np.asarray(tiles, np.float32).reshape(-1, 4)
    counted, young, above, nonfinite = verdict(t, threshold, min_frames)
    worst_tile = np.float32(0)
    worst_texel = np.float32(0)
    n_min = INF
    with np.errstate(all="ignore"):
        per_texel = t[counted, 0] / t[counted, 2]
    for q in per_texel:
        worst_tile = np.fmax(worst_tile, q)
    for q in t[:, 1]:
        worst_texel = np.fmax(worst_texel, q)
    for q in t[counted, 3]:
        n_min = np.fmin(n_min, q)
    return {"tiles": int(counted.sum()), "tiles_above": int(above.sum()), "tiles_young": int(young.sum()),
            "tiles_nonfinite": int(nonfinite.sum()), "texels": int(t[counted, 2].astype(np.int64).sum()),
            "worst_tile": np.float32(worst_tile), "worst_texel": np.float32(worst_texel),
            "n_min": np.float32(n_min if counted.any() else 0), "threshold": np.float32(threshold)}


def estimate(accum, moments, threshold, min_frames):
    """(tile map, summary)"""
    tiles = tile_map(accum, moments)
    return tiles, summary(tiles, threshold, min_frames)


def converged(s):
    return s["tiles"] > 0 and s["tiles_above"] == 0


def combine(summaries):
    """A device group's summary from its members': counts add, max of max, min of min"""
    out = {k: 0 for k in FIELDS[:5]}
    out.update(worst_tile=np.float32(0), worst_texel=np.float32(0), n_min=np.float32(0), threshold=np.float32(0))
    first = True
    for s in summaries:
        for k in FIELDS[:5]:
            out[k] += s[k]
        out["worst_tile"] = np.fmax(out["worst_tile"], s["worst_tile"])
        out["worst_texel"] = np.fmax(out["worst_texel"], s["worst_texel"])
        if s["tiles"]:
            out["n_min"] = s["n_min"] if first else np.fmin(out["n_min"], s["n_min"])
            first = False
        out["threshold"] = s["threshold"]
    return out


def same_summary(got, want):
    """Field for field: integers equal, floats bit for bit (a NaN matches a NaN)"""
    for k in FIELDS:
        a, b = got[k], want[k]
        if k in FIELDS[:5]:
            if int(a) != int(b):
                return False
        elif not (np.float32(a) == np.float32(b) or (np.isnan(a) and np.isnan(b))):
            return False
    return True


def rmse_estimate(tiles):
    """The image-wide estimate a host forms from the tile map, in double: sqrt(sum of sum_r / (3 * texels))"""
    t = np.asarray(tiles, np.float64).reshape(-1, 4)
    texels = t[:, 2].sum()
    return math.sqrt(t[:, 0].sum() / (3.0 * texels)) if texels else 0.0


def render_until(chunk_estimate, max_frames, check_every, lookahead=True):
    """Renderer.renderUntil's loop over a replay: chunk_estimate(frames) -> the summary of the mean of `frames` frames.  Returns
    (converged, frames, summary)."""
    frames = 0
    pending = s = s_frames = None
    while frames < max_frames:
        frames += min(check_every, max_frames - frames)
        if lookahead:
            if pending is not None:
                s, s_frames = chunk_estimate(pending), pending
                if converged(s):
                    return True, frames, s
            pending = frames
        else:
            s, s_frames = chunk_estimate(frames), frames
            if converged(s):
                return True, frames, s
    if s_frames != frames:
        s = chunk_estimate(frames)
    return converged(s), frames, s
