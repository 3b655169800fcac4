// pt_reproject_scene.hip -- the running mean and its moments carried across a scene change (include/mi3pt.h: mi3pt_reproject_scene).
//
// pt_reproject.hip's gather with one step in front of it: a texel of the NEW view whose triangle MOVED between the kept geometry
// (mi3pt_keep_geometry) and the current one takes the barycentric coordinates of its first hit in the current triangle and looks up the
// point Q -- and the interpolated normal NQ -- that these name in the kept triangle of the same index.  Q is then projected into the old
// view and validated against the old view's features in P's place: the motion-vector half of SVGF.  A texel whose triangle did not move
// (nine position floats equal as words) is k_reproject's texel bit for bit: Q = P, NQ = N, len = 1, tq = t1 make both test products exact.
// The arithmetic is the header's, operation for operation (fp32, nothing contracted, correctly rounded division and square root);
// tests/reproject_scene_reference.py restates it in numpy and tests/test_gpu_reproject_scene.py holds this file to it bit for bit.
//
// k_reproject's shape: one wave per 8 x 8 tile, lane j = 8 * (row in tile) + (column in tile), 256-thread blocks, no LDS, no atomics, every
// texel of both outputs written.  The records are read as aligned 16-byte loads (positions at byte 0 / 16 / 32, normals at 48 / 64 / 80 of
// the 112-byte record): the three position vectors of both records first, the kept record's normals by the moved lanes only.  Neighbouring
// texels share triangles, so these gathers mostly hit cache.  While no upload has followed mi3pt_keep_geometry both record pointers name
// one buffer: every texel is static and the kept record is not read at all.  The triangle index and every tap index are range-checked
// before they are used: images of NaNs or infinities neither hang nor fault.
#include "../../include/mi3pt.h"
#include "pt_kernels.h"
#include "pt_devmath.h"
#include "pt_accum.h"

namespace pt {

constexpr int RS_WAVES = 4;
constexpr size_t RS_RECORD = MI3PT_TRIANGLE_STRIDE / 16;        // a record in float4

PT_DEV float rs_dot(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
PT_DEV f3 rs_sub(f3 a, f3 b) { return F3(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_DEV bool rs_same_words(const float4 &a, const float4 &b)
{
    return __float_as_int(a.x) == __float_as_int(b.x) && __float_as_int(a.y) == __float_as_int(b.y) && __float_as_int(a.z) == __float_as_int(b.z);
}

__global__ void __launch_bounds__(256) k_reproject_scene(const ReprojectSceneLaunch S)
{
    const ReprojectLaunch &R = S.view;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const uint32_t tiles_x = (uint32_t)(R.width + 7) >> 3, tiles_y = (uint32_t)(R.rows + 7) >> 3;
    const uint32_t t = (uint32_t)blockIdx.x * RS_WAVES + (uint32_t)wave;
    if (t >= tiles_x * tiles_y) return;        // (the whole wave)
    const uint32_t trow = t / tiles_x;
    const int x = (int)(t - trow * tiles_x) * 8 + (lane & 7), y = (int)trow * 8 + (lane >> 3);
    if (x >= R.width || y >= R.rows) return;
    const size_t i = (size_t)y * (size_t)R.width + (size_t)x;
    if ((uint32_t)x >= R.res_w || (uint32_t)y >= R.res_h) {        // outside the rectangle: the texel keeps its bits
        R.accum_out[i] = R.accum[i];
        R.moments_out[i] = R.moments[i];
        return;
    }
    const float4 ids1 = R.ids1[i], pos1 = R.pos1[i], nrm1 = R.nrm1[i];
    const float inf = __uint_as_float(0x7f800000u);
    float ws = 0.0f, nmin = inf, history = R.max_history;
    f3 col = F3(0.0f, 0.0f, 0.0f), var = F3(0.0f, 0.0f, 0.0f);
    const int T = __float_as_int(ids1.x);
    if (__float_as_int(ids1.z) == 1 && T >= 0 && T < S.ntris) {
        const f3 P = xyz(pos1);
        f3 Q = P, NQ = xyz(nrm1);
        float len = 1.0f, tq = pos1.w;
        bool ok = true, moved = false;
        float4 a0, b0, c0, a1, b1, c1;
        if (S.tris0 != S.tris1) {        // (wave-uniform; else the kept geometry IS the current one)
            const float4 *r1 = S.tris1 + (size_t)T * RS_RECORD, *r0 = S.tris0 + (size_t)T * RS_RECORD;
            a1 = r1[0]; b1 = r1[1]; c1 = r1[2];
            a0 = r0[0]; b0 = r0[1]; c0 = r0[2];
            moved = !(rs_same_words(a0, a1) && rs_same_words(b0, b1) && rs_same_words(c0, c1));
            if (moved) {
                const float4 na0 = r0[3], nb0 = r0[4], nc0 = r0[5];
                const f3 e1 = rs_sub(xyz(b1), xyz(a1)), e2 = rs_sub(xyz(c1), xyz(a1)), w = rs_sub(P, xyz(a1));
                const float d11 = rs_dot(e1, e1), d12 = rs_dot(e1, e2), d22 = rs_dot(e2, e2), w1 = rs_dot(w, e1), w2 = rs_dot(w, e2);
                const float den = d11 * d22 - d12 * d12;
                const float u = (d22 * w1 - d12 * w2) / den;
                const float v = (d11 * w2 - d12 * w1) / den;
                const float g = (1.0f - u) - v;
                const f3 f1 = rs_sub(xyz(b0), xyz(a0)), f2 = rs_sub(xyz(c0), xyz(a0));
                Q = F3(a0.x + (u * f1.x + v * f2.x), a0.y + (u * f1.y + v * f2.y), a0.z + (u * f1.z + v * f2.z));
                NQ = F3((g * na0.x + u * nb0.x) + v * nc0.x, (g * na0.y + u * nb0.y) + v * nc0.y, (g * na0.z + u * nb0.z) + v * nc0.z);
                len = sqrtf(rs_dot(NQ, NQ));
                const f3 dq = rs_sub(Q, F3(R.f0[0], R.f0[1], R.f0[2]));
                tq = sqrtf(rs_dot(dq, dq));
                ok = den > 0.0f && len > 0.0f;        // (a NaN fails)
                history = S.max_history_moved;
            }
        }
        const f3 d = F3(Q.x - R.f0[0], Q.y - R.f0[1], Q.z - R.f0[2]);
        const float a = rs_dot(d, F3(R.f0[8], R.f0[9], R.f0[10]));
        const float b = rs_dot(d, F3(R.f0[12], R.f0[13], R.f0[14]));
        const float cz = rs_dot(d, F3(R.f0[4], R.f0[5], R.f0[6]));
        if (ok && cz > 0.0f) {
            const float aspect = R.f0[3], ft = R.f0[7], fr = R.f0[11];
            const float k = aspect / cz;
            const float uvx = (a * k + fr) / (fr + fr);
            const float uvy = (b * k + ft) / (ft + ft);
            const float fx = uvx * R.res0_x, fy = uvy * R.res0_y;
            if (fx > -1.0f && fx < (float)R.width && fy > -1.0f && fy < (float)R.rows) {        // (a NaN fails)
                const float x0f = floorf(fx), y0f = floorf(fy);
                const float tx = fx - x0f, ty = fy - y0f;
                const float wx[2] = { 1.0f - tx, tx }, wy[2] = { 1.0f - ty, ty };
                const int x0 = (int)x0f, y0 = (int)y0f;        // (-1 .. width - 1, -1 .. rows - 1)
                const int mat1 = __float_as_int(ids1.y);
                const float cos_min = R.normal_cos_min * len;
                const float plane_max = (R.plane_tolerance * tq) * len;
#pragma unroll
                for (int j = 0; j < 2; j++)
#pragma unroll
                    for (int ii = 0; ii < 2; ii++) {
                        const int qx = x0 + ii, qy = y0 + j;
                        const float bw = wx[ii] * wy[j];
                        if (qx < 0 || qy < 0 || qx >= R.width || qy >= R.rows || (uint32_t)qx >= R.res_w || (uint32_t)qy >= R.res_h) continue;
                        if (!(bw > 0.0f)) continue;
                        const size_t q = (size_t)qy * (size_t)R.width + (size_t)qx;
                        const float4 ids0 = R.ids0[q];
                        if (__float_as_int(ids0.z) != 1 || __float_as_int(ids0.y) != mat1) continue;
                        const float4 m = R.moments[q];
                        const float n0 = m.w;
                        if (!(n0 >= 1.0f)) continue;        // (a NaN does not count)
                        const float4 nrm0 = R.nrm0[q], pos0 = R.pos0[q];
                        if (!(rs_dot(NQ, xyz(nrm0)) >= cos_min)) continue;
                        const f3 dp = F3(pos0.x - Q.x, pos0.y - Q.y, pos0.z - Q.z);
                        if (!(fabsf(rs_dot(NQ, dp)) <= plane_max)) continue;
                        const float4 c = R.accum[q];
                        ws = ws + bw;
                        col = F3(col.x + bw * c.x, col.y + bw * c.y, col.z + bw * c.z);
                        nmin = fminf(nmin, n0);
                        const bool two = n0 >= 2.0f;
                        const float nm1 = n0 - 1.0f;
                        const f3 v = two ? F3(fmaxf(m.x / nm1, 0.0f), fmaxf(m.y / nm1, 0.0f), fmaxf(m.z / nm1, 0.0f)) : F3(0.0f, 0.0f, 0.0f);
                        var = F3(var.x + bw * v.x, var.y + bw * v.y, var.z + bw * v.z);
                    }
            }
        }
    }
    if (ws > 0.0f) {
        const float n = fminf(nmin, history);
        const float nm1 = n - 1.0f;
        R.accum_out[i] = make_float4(store_round(col.x / ws, R.store_f16), store_round(col.y / ws, R.store_f16), store_round(col.z / ws, R.store_f16), 1.0f);
        R.moments_out[i] = make_float4((var.x / ws) * nm1, (var.y / ws) * nm1, (var.z / ws) * nm1, n);
    } else {
        R.accum_out[i] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        R.moments_out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

void launch_reproject_scene(const ReprojectSceneLaunch &S, hipStream_t s)
{
    if (S.view.width <= 0 || S.view.rows <= 0) return;
    const uint32_t ntiles = (uint32_t)((S.view.width + 7) / 8) * (uint32_t)((S.view.rows + 7) / 8);      // (at most 4096 x 4096: the grid is never capped)
    hipLaunchKernelGGL(k_reproject_scene, dim3((ntiles + RS_WAVES - 1) / RS_WAVES), dim3(256), 0, s, S);
}

}  // namespace pt
