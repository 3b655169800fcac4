"""Reference for the reprojection across a scene change (mi3pt_reproject_scene), written from the header comment of include/mi3pt.h.

numpy fp32, one operation per line of the definition (numpy neither contracts nor reassociates; fp32 `/` and sqrt are correctly rounded),
on reproject_reference's helpers.  The camera frame F0 and the two sets of triangle records are INPUTS, as they are for the kernel.
Nothing here looks at the device.  No test lives in this file.
"""
import numpy as np

import reproject_reference as rr

F32 = np.float32
INF = rr.INF
_dot = rr._dot


def records(tris):
    """112-byte triangle records (a layout.TRIANGLE array or raw bytes) as (n, 28) float32 words: positions at 0 / 4 / 8, normals at
    12 / 16 / 20"""
    raw = np.ascontiguousarray(tris)
    return np.frombuffer(raw.tobytes(), F32).reshape(-1, 28)


def reproject_scene(accum, moments, f0, res0, new, old, rect, tris1, tris0, plane_tolerance=0.02, normal_cos_min=0.9, max_history=64,
                    max_history_moved=8, store_f16=False):
    """mi3pt_reproject_scene's kernel.  The arguments of reproject_reference.reproject, and tris1 / tris0: the current and the kept
    records (what `records` takes).  Returns (accum', moments', info); info as reproject's, and info["static"] / info["moved"]: (rows, w)
    bool over the texels inside the rectangle with hit1 == 1 and a triangle index in range."""
    A = np.ascontiguousarray(accum, F32)
    M = np.ascontiguousarray(moments, F32)
    rows, w = A.shape[:2]
    f0 = np.asarray(f0, F32)
    r1, r0 = records(tris1), records(tris0)
    ntris = r1.shape[0]
    assert r0.shape[0] == ntris
    pos1, nrm1, ids1 = np.asarray(new["position"], F32), np.asarray(new["normal"], F32), rr._ids_words(new["ids"])
    pos0, nrm0, ids0 = np.asarray(old["position"], F32), np.asarray(old["normal"], F32), rr._ids_words(old["ids"])
    ys, xs = np.mgrid[0:rows, 0:w]
    res_w, res_h = int(rect[0]), int(rect[1])
    in_rect = (xs < res_w) & (ys < res_h)
    tol, cos_min = F32(plane_tolerance), F32(normal_cos_min)
    hist, hist_moved = F32(float(int(max_history))), F32(float(int(max_history_moved)))
    with np.errstate(all="ignore"):
        T = ids1[..., 0].astype(np.int64)
        ok = in_rect & (ids1[..., 2] == 1) & (T >= 0) & (T < ntris)
        Tc = np.clip(T, 0, ntris - 1)
        R1, R0 = r1[Tc], r0[Tc]                                                    # (rows, w, 28)
        static = np.all(R1[..., [0, 1, 2, 4, 5, 6, 8, 9, 10]].view(np.int32) == R0[..., [0, 1, 2, 4, 5, 6, 8, 9, 10]].view(np.int32), axis=-1)
        moved = ok & ~static
        static = ok & static
        P = [pos1[..., k] for k in range(3)]
        t1 = pos1[..., 3]
        N = [nrm1[..., k] for k in range(3)]
        a1, b1, c1 = ([R1[..., o + k] for k in range(3)] for o in (0, 4, 8))
        a0, b0, c0, na0, nb0, nc0 = ([R0[..., o + k] for k in range(3)] for o in (0, 4, 8, 12, 16, 20))
        e1 = [b1[k] - a1[k] for k in range(3)]
        e2 = [c1[k] - a1[k] for k in range(3)]
        ww = [P[k] - a1[k] for k in range(3)]
        d11, d12, d22 = _dot(*e1, *e1), _dot(*e1, *e2), _dot(*e2, *e2)
        w1, w2 = _dot(*ww, *e1), _dot(*ww, *e2)
        den = d11 * d22 - d12 * d12
        u = (d22 * w1 - d12 * w2) / den
        v = (d11 * w2 - d12 * w1) / den
        g = (F32(1) - u) - v
        f1 = [b0[k] - a0[k] for k in range(3)]
        f2 = [c0[k] - a0[k] for k in range(3)]
        Qm = [a0[k] + (u * f1[k] + v * f2[k]) for k in range(3)]
        NQm = [(g * na0[k] + u * nb0[k]) + v * nc0[k] for k in range(3)]
        lenm = np.sqrt(_dot(*NQm, *NQm))
        dq = [Qm[k] - f0[k] for k in range(3)]
        tqm = np.sqrt(_dot(*dq, *dq))
        ok &= static | ((den > F32(0)) & (lenm > F32(0)))
        Q = [np.where(moved, Qm[k], P[k]).astype(F32) for k in range(3)]
        NQ = [np.where(moved, NQm[k], N[k]).astype(F32) for k in range(3)]
        ln = np.where(moved, lenm, F32(1)).astype(F32)
        tq = np.where(moved, tqm, t1).astype(F32)
        cap = np.where(moved, hist_moved, hist).astype(F32)
        # from here: mi3pt_reproject's law with Q in P's place
        dx, dy, dz = Q[0] - f0[0], Q[1] - f0[1], Q[2] - f0[2]
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
        cos_need = cos_min * ln
        plane_max = (tol * tq) * ln
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
                counts &= _dot(*NQ, nrm0[cy, cx, 0], nrm0[cy, cx, 1], nrm0[cy, cx, 2]) >= cos_need
                ex, ey, ez = pos0[cy, cx, 0] - Q[0], pos0[cy, cx, 1] - Q[1], pos0[cy, cx, 2] - Q[2]
                counts &= np.abs(_dot(*NQ, ex, ey, ez)) <= plane_max
                ws = np.where(counts, ws + bw, ws)
                nmin = np.where(counts, np.fmin(nmin, n0), nmin)
                nm1 = n0 - F32(1)
                for ch in range(3):
                    col[..., ch] = np.where(counts, col[..., ch] + bw * A[cy, cx, ch], col[..., ch])
                    vv = np.where(n0 >= F32(2), np.fmax(M[cy, cx, ch] / nm1, F32(0)), F32(0)).astype(F32)
                    var[..., ch] = np.where(counts, var[..., ch] + bw * vv, var[..., ch])
                taps += counts
                weighted += ok & (bw > F32(0))
        carried = in_rect & (ws > F32(0))
        n_new = np.fmin(nmin, cap)
        nm1 = n_new - F32(1)
        out_a = np.zeros((rows, w, 4), F32)
        out_m = np.zeros((rows, w, 4), F32)
        for ch in range(3):
            out_a[..., ch] = np.where(carried, rr.store_round(col[..., ch] / ws, store_f16), F32(0))
            out_m[..., ch] = np.where(carried, (var[..., ch] / ws) * nm1, F32(0))
        out_a[..., 3] = F32(1)
        out_m[..., 3] = np.where(carried, n_new, F32(0))
    out_a = np.where(in_rect[..., None], out_a, A)
    out_m = np.where(in_rect[..., None], out_m, M)
    info = {"carried": carried, "restarted": in_rect & ~carried, "taps": taps, "weighted": weighted, "static": static, "moved": moved}
    return out_a.astype(F32), out_m.astype(F32), info
