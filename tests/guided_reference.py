"""Reference for the feature-guided a-trous de-noise (mi3pt_denoise_guided), written from the header comment of include/mi3pt.h.

numpy fp32, one operation per line of the definition (numpy neither contracts nor reassociates; fp32 `/` is correctly rounded), with
pt_oracle.math_fn(4, .) for exp.  Nothing here looks at the device.  No test lives in this file.
"""
import numpy as np

H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
TINY = np.float32(2.0 ** -126)      # the smallest normal fp32: exp(x) lies below it for x in about (-103.97, -87.34)


def inv_sigma(sigma):
    """1 / (sigma * sigma) in fp32; 0 switches the term off"""
    s = np.float32(sigma)
    if s == 0:
        return np.float32(0)
    with np.errstate(over="ignore", divide="ignore"):
        return np.float32(1) / (s * s)


def _shift(img, dy, dx, fill=0):
    """img[y + dy, x + dx] where that lies inside, `fill` elsewhere"""
    h, w = img.shape[:2]
    out = np.full_like(img, fill)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = img[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def guided(orc, accum, normal, position, albedo, ids, levels=3, sigma_color=1.0, sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.05):
    """accum, normal, position, albedo: (rows, w, 4) float32; ids: (rows, w, 4) int32.  Returns (filtered (rows, w, 4) float32, stats):
    stats["rejected"]: share of the in-image taps the hit rule rejects; stats["below"] / stats["above"]: shares of the counted
    off-centre taps whose exp(...) lies below / above 0.5; stats["subnormal"]: the counted taps whose exp(...) is a subnormal (0 < e < 2^-126); stats["taps"]: in-image taps
    -- all over every level."""
    c = np.ascontiguousarray(accum, np.float32)
    n = np.ascontiguousarray(normal, np.float32)[..., :3]
    pos = np.ascontiguousarray(position, np.float32)[..., :3]
    a = np.ascontiguousarray(albedo, np.float32)[..., :3]
    words = np.ascontiguousarray(ids)
    hit = (words if words.dtype == np.int32 else words.view(np.int32))[..., 2]
    rows, w = c.shape[:2]
    inv_color, inv_normal = inv_sigma(sigma_color), inv_sigma(sigma_normal)
    inv_albedo, inv_plane = inv_sigma(sigma_albedo), inv_sigma(sigma_plane)
    inside_all = np.ones((rows, w), bool)
    taps = rejected = counted_off = below = above = subnormal = 0
    cur = c
    for i in range(levels):
        s = 1 << i
        inv_c = inv_color * np.float32(4 ** i)
        den = np.zeros((rows, w), np.float32)
        num = np.zeros((rows, w, 3), np.float32)
        cp = cur[..., :3]
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * s, dx * s
                inside = _shift(inside_all, oy, ox, False)
                counts = inside & (_shift(hit, oy, ox) == hit)
                cq = _shift(cur, oy, ox)[..., :3]
                with np.errstate(all="ignore"):
                    ec = _sq3(cq - cp) * inv_c
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
        out[..., 3] = cur[..., 3]
        cur = out
    stats = {"taps": taps, "rejected": rejected / taps if taps else 0.0,
             "below": below / counted_off if counted_off else 0.0, "above": above / counted_off if counted_off else 0.0, "subnormal": subnormal}
    return cur, stats
