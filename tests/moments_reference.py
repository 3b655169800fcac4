"""Reference for the moments image (mi3pt_set_moments) and the variance-guided filter (MI3PT_GUIDED_VARIANCE), written from the header
comments of include/mi3pt.h.

numpy fp32, one operation per line of the definitions (numpy neither contracts nor reassociates; fp32 `/` is correctly rounded), with
pt_oracle.math_fn(4, .) for exp.  Nothing here looks at the device.  No test lives in this file.
"""
import numpy as np

from guided_reference import H5, TINY, _shift, _sq3, inv_sigma

G3 = np.array([1 / 4, 1 / 2, 1 / 4], np.float32)
VARIANCE_EPS = np.float32(1e-8)       # MI3PT_GUIDED_VARIANCE_EPS


def welford(frames, means_before, means_after, acc_frames, enabled=1, moments=None, inside=None):
    """The moments image after one accumulate step per entry of `frames`.  frames[k]: the radiance (rows, w, >= 3) the step reads;
    means_before[k] / means_after[k]: the mean before the step and after it AS STORED; acc_frames[k]: the accumulate block's u32
    `frame` of the step; enabled: its `enabled`, one value or one per step; moments: the image before the first step (zero);
    inside: (rows, w) bool, the texels inside the accumulate block's rectangle (all).  Returns (rows, w, 4) float32: M2.rgb, n."""
    rows, w = np.asarray(frames[0]).shape[:2]
    m = np.zeros((rows, w, 4), np.float32) if moments is None else np.array(moments, np.float32)
    inside = np.ones((rows, w), bool) if inside is None else np.asarray(inside, bool)
    enabled = list(enabled) if np.ndim(enabled) else [enabled] * len(frames)
    for k in range(len(frames)):
        c = np.asarray(frames[k], np.float32)
        p = np.asarray(means_before[k], np.float32)
        pn = np.asarray(means_after[k], np.float32)
        frame = int(acc_frames[k]) & 0xFFFFFFFF
        restart = frame <= 1 or int(enabled[k]) != 1
        new = np.empty_like(m)
        if restart:
            new[..., :3] = np.float32(0)
            new[..., 3] = np.float32(1)
        else:
            with np.errstate(all="ignore"):
                for ch in range(3):
                    a = c[..., ch] - p[..., ch]
                    b = c[..., ch] - pn[..., ch]
                    ab = a * b
                    new[..., ch] = m[..., ch] + ab
                new[..., 3] = m[..., 3] + np.float32(1)
        m = np.where(inside[..., None], new, m)
    return m


def variance_of_mean(moments):
    """v per texel: fmax(((M2.r + M2.g) + M2.b) / (n * (n - 1)), 0) for n >= 2, else 0"""
    m = np.asarray(moments, np.float32)
    n = m[..., 3]
    with np.errstate(all="ignore"):
        s = (m[..., 0] + m[..., 1]) + m[..., 2]
        nm1 = n - np.float32(1)
        d = n * nm1
        q = s / d
        v = np.fmax(q, np.float32(0))
    return np.where(n >= np.float32(2), v, np.float32(0)).astype(np.float32)


def initial_variance(moments, hit):
    """var_0: v averaged over the 3 x 3 neighbours inside the image whose hit flag is the centre's, g = [1/4, 1/2, 1/4]"""
    v = variance_of_mean(moments)
    rows, w = v.shape
    inside_all = np.ones((rows, w), bool)
    num = np.zeros((rows, w), np.float32)
    den = np.zeros((rows, w), np.float32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            counts = _shift(inside_all, dy, dx, False) & (_shift(hit, dy, dx) == hit)
            wgt = G3[dx + 1] * G3[dy + 1]
            with np.errstate(all="ignore"):
                t = wgt * _shift(v, dy, dx)
                num = np.where(counts, num + t, num)
            den = np.where(counts, den + wgt, den)
    with np.errstate(all="ignore"):
        return num / den


def guided_variance(orc, accum, moments, normal, position, albedo, ids, levels=3, sigma_color=2.0, sigma_normal=0.35, sigma_albedo=0.1,
                    sigma_plane=0.05, flush_squares=False):
    """guided_reference.guided with MI3PT_GUIDED_VARIANCE.  moments: (rows, w, 4) float32.  Returns (filtered (rows, w, 4) float32,
    variance (rows, w) float32 after the last level, stats as guided_reference.guided and "squared_subnormal": the counted taps with a
    normal weight w whose square w * w is an fp32 subnormal).  flush_squares: what a build computes that returns such a square as 0 --
    never the reference, only the proof that a test case can tell the two apart."""
    c = np.ascontiguousarray(accum, np.float32)
    n = np.ascontiguousarray(normal, np.float32)[..., :3]
    pos = np.ascontiguousarray(position, np.float32)[..., :3]
    a = np.ascontiguousarray(albedo, np.float32)[..., :3]
    words = np.ascontiguousarray(ids)
    hit = (words if words.dtype == np.int32 else words.view(np.int32))[..., 2]
    rows, w = c.shape[:2]
    sc = np.float32(sigma_color)
    with np.errstate(over="ignore"):
        k_c = sc * sc
    inv_normal, inv_albedo, inv_plane = inv_sigma(sigma_normal), inv_sigma(sigma_albedo), inv_sigma(sigma_plane)
    inside_all = np.ones((rows, w), bool)
    taps = rejected = counted_off = below = above = subnormal = squared_subnormal = 0
    cur = c
    var = initial_variance(moments, hit)
    for i in range(levels):
        s = 1 << i
        den = np.zeros((rows, w), np.float32)
        num = np.zeros((rows, w, 3), np.float32)
        nv = np.zeros((rows, w), np.float32)
        cp = cur[..., :3]
        with np.errstate(all="ignore"):
            kv = k_c * var
            denom = kv + VARIANCE_EPS
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                inside = _shift(inside_all, oy, ox, False)
                counts = inside & (_shift(hit, oy, ox) == hit)
                cq = _shift(cur, oy, ox)[..., :3]
                vq = _shift(var, oy, ox)
                with np.errstate(all="ignore"):
                    ec = _sq3(cq - cp) / denom if sc != 0 else np.zeros((rows, w), np.float32)
                    en = _sq3(_shift(n, oy, ox) - n) * inv_normal
                    ea = _sq3(_shift(a, oy, ox) - a) * inv_albedo
                    dp = _shift(pos, oy, ox) - pos
                    pd = (n[..., 0] * dp[..., 0] + n[..., 1] * dp[..., 1]) + n[..., 2] * dp[..., 2]
                    ep = (pd * pd) * inv_plane
                    e = orc.math_fn(4, -(((ec + en) + ea) + ep))
                    wgt = e * (H5[dx + 2] * H5[dy + 2])
                    den = np.where(counts, den + wgt, den)
                    for k in range(3):
                        num[..., k] = np.where(counts, num[..., k] + wgt * cq[..., k], num[..., k])
                    ww = wgt * wgt
                    tiny_square = (wgt >= TINY) & (ww > 0) & (ww < TINY)
                    if flush_squares:
                        ww = np.where(tiny_square, np.float32(0), ww)
                    nv = np.where(counts, nv + ww * vq, nv)
                squared_subnormal += int((counts & tiny_square).sum())
                taps += int(inside.sum())
                rejected += int((inside & ~counts).sum())
                if dy or dx:
                    counted_off += int(counts.sum())
                    below += int((counts & (e < 0.5)).sum())
                    above += int((counts & (e > 0.5)).sum())
                    subnormal += int((counts & (e > 0) & (e < TINY)).sum())
        out = np.empty_like(c)
        with np.errstate(all="ignore"):
            for k in range(3):
                out[..., k] = num[..., k] / den
            dd = den * den
            var = nv / dd
        out[..., 3] = cur[..., 3]
        cur = out
    stats = {"taps": taps, "rejected": rejected / taps if taps else 0.0,
             "below": below / counted_off if counted_off else 0.0, "above": above / counted_off if counted_off else 0.0, "subnormal": subnormal,
             "squared_subnormal": squared_subnormal}
    return cur, var, stats


def oracle_steps(orc, osc, steps, w, h, rt_uniforms, acc_uniforms, rank=0, nranks=1, block_rows=8, store_f16=False, mean=None,
                 moments=None, inside=None):
    """The oracle's accumulate steps with the moments image beside them.  steps: (raytrace frame, accumulate frame, enabled) per step;
    rt_uniforms(frame) / acc_uniforms(frame, enabled): the two uniform blocks as bytes.  Returns (mean, moments, frames, means): the
    final images, the radiance of every step and the mean after every step."""
    rows = orc.tile_local_rows(h, rank, nranks, block_rows)
    mean = np.zeros((rows, w, 4), np.float32) if mean is None else mean
    frames, before, after = [], [], []
    for rt_frame, acc_frame, enabled in steps:
        img, _ = orc.raytrace(osc, rt_uniforms(rt_frame), w, h, rank, nranks, block_rows, store_f16=store_f16)
        new = orc.accumulate(acc_uniforms(acc_frame, enabled), w, h, img, mean, rank, nranks, block_rows, store_f16=store_f16)
        frames.append(img)
        before.append(mean)
        after.append(new)
        mean = new
    m = welford(frames, before, after, [s[1] for s in steps], [s[2] for s in steps], moments=moments, inside=inside)
    return mean, m, frames, after
