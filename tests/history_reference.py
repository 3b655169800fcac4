"""Reference for the validated merge of a held history (mi3pt_hold_history, mi3pt_merge_history), written from the header comment of
include/mi3pt.h.

numpy fp32, one operation per line of the definition, the window in the header's order: dy outer, dx inner (numpy neither contracts nor
reassociates; fp32 `/` is correctly rounded; np.fmax / np.fmin return the other operand for a NaN, as fmaxf / fminf do).  Nothing here
looks at the device.  No test lives in this file.
"""
import numpy as np

from reproject_reference import store_round

F32 = np.float32
EPS = F32(1e-8)          # MI3PT_HISTORY_EPS


def per_sample_variance(moments):
    """var(m2, n).k = n >= 2 ? fmaxf(m2.k / (n - 1), 0) : 0, as (rows, w, 3)"""
    m = np.asarray(moments, F32)
    n = m[..., 3]
    with np.errstate(all="ignore"):
        nm1 = n - F32(1)
        q = np.fmax(m[..., :3] / nm1[..., None], F32(0))
        return np.where((n >= F32(2))[..., None], q, F32(0)).astype(F32)


def merge_history(accum, moments, accum_held, moments_held, rect=None, radius=1, z_keep=2.0, z_drop=4.0, store_f16=False):
    """mi3pt_merge_history's kernel.  accum / moments: the live pair, accum_held / moments_held: the held pair, each (rows, w, 4) float32;
    rect: (res_w, res_h) of the accumulate block (None: the image).  Returns (accum', moments', info): info["merged"], ["dropped"],
    ["only_held"], ["neither"]: (rows, w) bool over the texels inside the rectangle; info["nk"]: the held samples a merged texel kept (0
    elsewhere), info["z2"], info["lam"]: the test's score and the share, where both sides have samples."""
    A = np.ascontiguousarray(accum, F32)
    M = np.ascontiguousarray(moments, F32)
    Ah = np.ascontiguousarray(accum_held, F32)
    Mh = np.ascontiguousarray(moments_held, F32)
    rows, w = A.shape[:2]
    r = int(radius)
    res_w, res_h = (w, rows) if rect is None else (int(rect[0]), int(rect[1]))
    ys, xs = np.mgrid[0:rows, 0:w]
    in_rect = (xs < res_w) & (ys < res_h)
    zk, zd = F32(z_keep), F32(z_drop)
    with np.errstate(all="ignore"):
        n, nh = M[..., 3], Mh[..., 3]
        pair = in_rect & (n >= F32(1)) & (nh >= F32(1))
        sf, sh = per_sample_variance(M), per_sample_variance(Mh)
        wgt = F32(1) / n + F32(1) / nh
        d_tap = A[..., :3] - Ah[..., :3]
        v_tap = np.fmax(sf, sh) * wgt[..., None]
        # the taps' values on a canvas with a margin of r: outside the image nothing pairs
        P = np.zeros((rows + 2 * r, w + 2 * r), bool)
        Dt = np.zeros((rows + 2 * r, w + 2 * r, 3), F32)
        Vt = np.zeros((rows + 2 * r, w + 2 * r, 3), F32)
        P[r:r + rows, r:r + w] = pair
        Dt[r:r + rows, r:r + w] = d_tap
        Vt[r:r + rows, r:r + w] = v_tap
        D = np.zeros((rows, w, 3), F32)
        V = np.zeros((rows, w, 3), F32)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                sl = (slice(r + dy, r + dy + rows), slice(r + dx, r + dx + w))
                counts = P[sl][..., None]
                D = np.where(counts, D + Dt[sl], D)
                V = np.where(counts, V + Vt[sl], V)
        DD = D * D
        z = DD / (V + EPS)
        z2 = np.fmax(np.fmax(z[..., 0], z[..., 1]), z[..., 2])
        drop2 = zd * zd
        keep2 = zk * zk
        lam = np.fmin(np.fmax((drop2 - z2) / (drop2 - keep2), F32(0)), F32(1))
        nk = np.floor(nh * lam)
        live, held = n >= F32(1), nh >= F32(1)
        merged = in_rect & live & held & (nk >= F32(1))
        only_held = in_rect & ~live & held
        N = n + nk
        f = nk / N
        nf = n * f
        nk1 = nk - F32(1)
        d = Ah[..., :3] - A[..., :3]
        new_a = np.empty((rows, w, 4), F32)
        new_m = np.empty((rows, w, 4), F32)
        for k in range(3):
            new_a[..., k] = store_round(A[..., k] + d[..., k] * f, store_f16)
            kept = M[..., k] + sh[..., k] * nk1
            between = (d[..., k] * d[..., k]) * nf
            new_m[..., k] = kept + between
        new_a[..., 3] = F32(1)
        new_m[..., 3] = N
    out_a = np.where(merged[..., None], new_a, np.where(only_held[..., None], Ah, A))
    out_m = np.where(merged[..., None], new_m, np.where(only_held[..., None], Mh, M))
    info = {"merged": merged, "only_held": only_held, "dropped": in_rect & live & ~merged, "neither": in_rect & ~live & ~held,
            "nk": np.where(merged, nk, F32(0)).astype(F32), "z2": z2, "lam": lam}
    return out_a.astype(F32), out_m.astype(F32), info


def kept_share(moments_before, moments_after, moments_held, where=None):
    """the share of carried samples kept: the sum of n' - n over the sum of nh, in float64 (where: a (rows, w) bool selection)"""
    n0 = np.asarray(moments_before, np.float64)[..., 3]
    n1 = np.asarray(moments_after, np.float64)[..., 3]
    nh = np.asarray(moments_held, np.float64)[..., 3]
    if where is not None:
        n0, n1, nh = n0[where], n1[where], nh[where]
    total = float(nh.sum())
    return float((n1 - n0).sum()) / total if total > 0 else 0.0
