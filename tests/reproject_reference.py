"""Reference for the mean by count (mi3pt_set_mean_by_count) and the reprojection (mi3pt_reproject), written from the header comments of
include/mi3pt.h.

numpy fp32, one operation per line of the definitions (numpy neither contracts nor reassociates; fp32 `/` is correctly rounded).  The
camera frame F0 is an INPUT, as it is for the kernel (mi3pt_host_view_frame computes it; view_frame below is an independent double
computation of the same definition).  Nothing here looks at the device.  No test lives in this file.
"""
import math

import numpy as np

F32 = np.float32
INF = F32(np.inf)


def store_round(v, store_f16):
    """what a stored mean keeps: the value itself, or its binary16 rounding under MI3PT_STORAGE_F16"""
    v = np.asarray(v, F32)
    if not store_f16:
        return v
    with np.errstate(all="ignore"):
        return v.astype(np.float16).astype(F32)


def mix(p, c, weight):
    """pt_accum.h's mix: p * (1 - weight) + c * weight"""
    with np.errstate(all="ignore"):
        one_minus = F32(1) - weight
        a = p * one_minus
        b = c * weight
        return a + b


def by_count_step(mean, moments, radiance, enabled=1, store_f16=False, inside=None):
    """One accumulate step under mi3pt_set_mean_by_count.  mean / radiance: (rows, w, >= 3), moments: (rows, w, 4) = M2.rgb, n; inside:
    (rows, w) bool, the texels inside the accumulate block's rectangle (None: all).  Returns (mean', moments') as (rows, w, 4) float32."""
    p = np.array(mean, F32)
    m = np.array(moments, F32)
    c = np.asarray(radiance, F32)
    rows, w = p.shape[:2]
    inside = np.ones((rows, w), bool) if inside is None else np.asarray(inside, bool)
    n = m[..., 3]
    with np.errstate(all="ignore"):
        restart = np.full((rows, w), int(enabled) != 1) | ~(n >= F32(1))
        np1 = n + F32(1)
        weight = np.where(restart, F32(1), F32(1) / np1).astype(F32)
    new_p = np.empty((rows, w, 4), F32)
    new_m = np.empty((rows, w, 4), F32)
    for k in range(3):
        pn = store_round(mix(p[..., k], c[..., k], weight), store_f16)
        new_p[..., k] = pn
        with np.errstate(all="ignore"):
            a = c[..., k] - p[..., k]
            b = c[..., k] - pn
            ab = a * b
            new_m[..., k] = np.where(restart, F32(0), m[..., k] + ab)
    new_p[..., 3] = F32(1)
    with np.errstate(all="ignore"):
        new_m[..., 3] = np.where(restart, F32(1), n + F32(1))
    out_p = np.array(mean, F32)
    if out_p.shape[2] < 4:
        out_p = np.concatenate([out_p, np.ones((rows, w, 4 - out_p.shape[2]), F32)], axis=2)
    out_p = np.where(inside[..., None], new_p, out_p)
    out_m = np.where(inside[..., None], new_m, m)
    return out_p.astype(F32), out_m.astype(F32)


def default_step(mean, moments, radiance, frame, enabled=1, store_f16=False, inside=None):
    """One accumulate step of the DEFAULT law with the moments image beside it (accumulate.wgsl:18-28; mi3pt_set_moments): the weight
    from the accumulate block's u32 `frame`."""
    p = np.array(mean, F32)
    m = np.array(moments, F32)
    c = np.asarray(radiance, F32)
    rows, w = p.shape[:2]
    inside = np.ones((rows, w), bool) if inside is None else np.asarray(inside, bool)
    frame = int(frame) & 0xFFFFFFFF
    weight = F32(1)
    if frame > 0:
        weight = F32(1) / F32(frame)
    if int(enabled) != 1:
        weight = F32(1)
    restart = frame <= 1 or int(enabled) != 1
    new_p = np.empty((rows, w, 4), F32)
    new_m = np.empty((rows, w, 4), F32)
    for k in range(3):
        pn = store_round(mix(p[..., k], c[..., k], weight), store_f16)
        new_p[..., k] = pn
        with np.errstate(all="ignore"):
            a = c[..., k] - p[..., k]
            b = c[..., k] - pn
            ab = a * b
            new_m[..., k] = F32(0) if restart else m[..., k] + ab
    new_p[..., 3] = F32(1)
    with np.errstate(all="ignore"):
        new_m[..., 3] = F32(1) if restart else m[..., 3] + F32(1)
    out_p = np.where(inside[..., None], new_p, p[..., :4] if p.shape[2] >= 4 else new_p)
    out_m = np.where(inside[..., None], new_m, m)
    return out_p.astype(F32), out_m.astype(F32)


def view_frame(uniforms96):
    """mi3pt_host_view_frame's definition, independently: python doubles from the block's fp32 fields, each output rounded to fp32 once.
    position, aspect | fwd, t | u, r | v, 0"""
    raw = bytes(uniforms96)
    aspect = float(np.frombuffer(raw, F32, 1, 8)[0])
    pos = [float(v) for v in np.frombuffer(raw, F32, 3, 32)]
    d = [float(v) for v in np.frombuffer(raw, F32, 3, 48)]
    fov = float(np.frombuffer(raw, F32, 1, 60)[0])
    length = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    w = [-d[0] / length, -d[1] / length, -d[2] / length]
    up = [0.0, 0.0, 1.0] if abs(w[1]) > 0.99999 else [0.0, 1.0, 0.0]
    u = [up[1] * w[2] - up[2] * w[1], up[2] * w[0] - up[0] * w[2], up[0] * w[1] - up[1] * w[0]]
    ul = math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    u = [x / ul for x in u]
    v = [w[1] * u[2] - w[2] * u[1], w[2] * u[0] - w[0] * u[2], w[0] * u[1] - w[1] * u[0]]
    t = math.tan(fov * math.pi / 360.0)
    r = aspect * t
    return np.array(pos + [aspect] + [-w[0], -w[1], -w[2], t] + u + [r] + v + [0.0], np.float64).astype(F32)


def orbit(position, target, degrees):
    """the camera turned by `degrees` about the vertical axis through its target: (position, unit direction towards the target)"""
    p, t = np.array(position, np.float64), np.array(target, np.float64)
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    d = p - t
    q = t + np.array([c * d[0] + s * d[2], d[1], -s * d[0] + c * d[2]])
    v = t - q
    return tuple(q), tuple(v / math.sqrt(float(v @ v)))


def _dot(ax, ay, az, bx, by, bz):
    with np.errstate(all="ignore"):
        return (ax * bx + ay * by) + az * bz


def _ids_words(ids):
    words = np.ascontiguousarray(ids)
    return words if words.dtype == np.int32 else words.view(np.int32)


def reproject(accum, moments, f0, res0, new, old, rect, plane_tolerance=0.02, normal_cos_min=0.9, max_history=64, store_f16=False):
    """mi3pt_reproject's kernel.  accum / moments: (rows, w, 4) float32 of the old view; f0: the 16 floats of the old view's frame; res0:
    the old block's two resolution floats; new / old: dicts with "position", "normal" (float32 (rows, w, 4)) and "ids" (int32 (rows, w,
    4)) of the new view and the previous set; rect: (res_w, res_h) of the accumulate block.  Returns (accum', moments', info) with
    info["carried"] / info["restarted"]: (rows, w) bool over the texels inside the rectangle, info["taps"]: (rows, w) taps that counted, info["weighted"]: the taps with bw > 0 of a texel
    whose projection passed every "needs" (all of them counting: the carried mean is the bilinear one)."""
    A = np.ascontiguousarray(accum, F32)
    M = np.ascontiguousarray(moments, F32)
    rows, w = A.shape[:2]
    f0 = np.asarray(f0, F32)
    pos1, nrm1, ids1 = np.asarray(new["position"], F32), np.asarray(new["normal"], F32), _ids_words(new["ids"])
    pos0, nrm0, ids0 = np.asarray(old["position"], F32), np.asarray(old["normal"], F32), _ids_words(old["ids"])
    ys, xs = np.mgrid[0:rows, 0:w]
    res_w, res_h = int(rect[0]), int(rect[1])
    in_rect = (xs < res_w) & (ys < res_h)
    tol, cos_min, hist = F32(plane_tolerance), F32(normal_cos_min), F32(float(int(max_history)))
    with np.errstate(all="ignore"):
        ok = in_rect & (ids1[..., 2] == 1)
        Px, Py, Pz, t1 = pos1[..., 0], pos1[..., 1], pos1[..., 2], pos1[..., 3]
        Nx, Ny, Nz = nrm1[..., 0], nrm1[..., 1], nrm1[..., 2]
        dx, dy, dz = Px - f0[0], Py - f0[1], Pz - f0[2]
        a = _dot(dx, dy, dz, f0[8], f0[9], f0[10])
        b = _dot(dx, dy, dz, f0[12], f0[13], f0[14])
        cz = _dot(dx, dy, dz, f0[4], f0[5], f0[6])
        ok &= cz > F32(0)
        k = f0[3] / cz
        uvx = (a * k + f0[11]) / (f0[11] + f0[11])
        uvy = (b * k + f0[7]) / (f0[7] + f0[7])
        fx = uvx * F32(res0[0])
        fy = uvy * F32(res0[1])
        ok &= (fx > F32(-1)) & (fx < F32(w)) & (fy > F32(-1)) & (fy < F32(rows))
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0f, fy - y0f
        wx = [F32(1) - tx, tx]
        wy = [F32(1) - ty, ty]
        x0 = np.where(ok, x0f, 0).astype(np.int64)
        y0 = np.where(ok, y0f, 0).astype(np.int64)
        plane_max = tol * t1
        ws = np.zeros((rows, w), F32)
        nmin = np.full((rows, w), INF, F32)
        col = np.zeros((rows, w, 3), F32)
        var = np.zeros((rows, w, 3), F32)
        taps = np.zeros((rows, w), np.int32)
        weighted = np.zeros((rows, w), np.int32)
        for j in range(2):
            for i in range(2):
                qx, qy = x0 + i, y0 + j
                bw = wx[i] * wy[j]
                inside = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < rows) & (qx < res_w) & (qy < res_h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, rows - 1)
                counts = inside & (bw > F32(0)) & (ids0[cy, cx, 2] == 1) & (ids0[cy, cx, 1] == ids1[..., 1])
                n0 = M[cy, cx, 3]
                counts &= n0 >= F32(1)
                counts &= _dot(Nx, Ny, Nz, nrm0[cy, cx, 0], nrm0[cy, cx, 1], nrm0[cy, cx, 2]) >= cos_min
                ex, ey, ez = pos0[cy, cx, 0] - Px, pos0[cy, cx, 1] - Py, pos0[cy, cx, 2] - Pz
                counts &= np.abs(_dot(Nx, Ny, Nz, ex, ey, ez)) <= plane_max
                ws = np.where(counts, ws + bw, ws)
                nmin = np.where(counts, np.fmin(nmin, n0), nmin)
                nm1 = n0 - F32(1)
                for ch in range(3):
                    col[..., ch] = np.where(counts, col[..., ch] + bw * A[cy, cx, ch], col[..., ch])
                    v = np.where(n0 >= F32(2), np.fmax(M[cy, cx, ch] / nm1, F32(0)), F32(0)).astype(F32)
                    var[..., ch] = np.where(counts, var[..., ch] + bw * v, var[..., ch])
                taps += counts
                weighted += ok & (bw > F32(0))
        carried = in_rect & (ws > F32(0))
        n_new = np.fmin(nmin, hist)
        nm1 = n_new - F32(1)
        out_a = np.zeros((rows, w, 4), F32)
        out_m = np.zeros((rows, w, 4), F32)
        for ch in range(3):
            out_a[..., ch] = np.where(carried, store_round(col[..., ch] / ws, store_f16), F32(0))
            out_m[..., ch] = np.where(carried, (var[..., ch] / ws) * nm1, F32(0))
        out_a[..., 3] = F32(1)
        out_m[..., 3] = np.where(carried, n_new, F32(0))
    out_a = np.where(in_rect[..., None], out_a, A)
    out_m = np.where(in_rect[..., None], out_m, M)
    return out_a.astype(F32), out_m.astype(F32), {"carried": carried, "restarted": in_rect & ~carried, "taps": taps, "weighted": weighted}
