// pt_reproject.hip -- the running mean and its moments carried from one view to another (include/mi3pt.h: mi3pt_reproject).
//
// A gather: every texel of the NEW view takes its first hit's world position (the new POSITION image), projects it with the OLD view's
// camera frame (mi3pt_host_view_frame) and reads the up to four texels around that point from the old view's (mean, moments), each
// validated against the old view's first-hit features.  The arithmetic is the header's, operation for operation (DESIGN.md "Pinned
// arithmetic": fp32, nothing contracted, correctly rounded division); tests/reproject_reference.py restates it in numpy and
// tests/test_gpu_reproject.py holds this file to it bit for bit.
//
// pt_converge.hip's shape: one wave per 8 x 8 tile, lane j = 8 * (row in tile) + (column in tile), so a lane's loads and stores are 16 B
// and a tile row is 128 contiguous bytes; a block's four waves take four neighbouring tiles.  The taps of a tile fall into a patch of the
// old image about the tile's size unless the view turned far.  No LDS, no atomics.  Every tap index is range-checked before it is used: an
// image of NaNs or infinities neither hangs nor faults.  It writes EVERY texel of the two output images: a texel outside the accumulate
// block's rectangle is copied, so that the outputs can take the inputs' place.
#include "../../include/mi3pt.h"
#include "pt_kernels.h"
#include "pt_devmath.h"
#include "pt_accum.h"

namespace pt {

constexpr int RP_WAVES = 4;

PT_DEV float dot3(f3 a, f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__global__ void __launch_bounds__(256) k_reproject(const ReprojectLaunch R)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const uint32_t tiles_x = (uint32_t)(R.width + 7) >> 3, tiles_y = (uint32_t)(R.rows + 7) >> 3;
    const uint32_t t = (uint32_t)blockIdx.x * RP_WAVES + (uint32_t)wave;
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
    float ws = 0.0f, nmin = inf;
    f3 col = F3(0.0f, 0.0f, 0.0f), var = F3(0.0f, 0.0f, 0.0f);
    if (__float_as_int(ids1.z) == 1) {
        const f3 P = xyz(pos1), N = xyz(nrm1);
        const float t1 = pos1.w;
        const f3 d = F3(P.x - R.f0[0], P.y - R.f0[1], P.z - R.f0[2]);
        const float a = dot3(d, F3(R.f0[8], R.f0[9], R.f0[10]));
        const float b = dot3(d, F3(R.f0[12], R.f0[13], R.f0[14]));
        const float cz = dot3(d, F3(R.f0[4], R.f0[5], R.f0[6]));
        if (cz > 0.0f) {
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
                const float plane_max = R.plane_tolerance * t1;
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
                        if (!(dot3(N, xyz(nrm0)) >= R.normal_cos_min)) continue;
                        const f3 dp = F3(pos0.x - P.x, pos0.y - P.y, pos0.z - P.z);
                        if (!(fabsf(dot3(N, dp)) <= plane_max)) continue;
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
        const float n = fminf(nmin, R.max_history);
        const float nm1 = n - 1.0f;
        R.accum_out[i] = make_float4(store_round(col.x / ws, R.store_f16), store_round(col.y / ws, R.store_f16), store_round(col.z / ws, R.store_f16), 1.0f);
        R.moments_out[i] = make_float4((var.x / ws) * nm1, (var.y / ws) * nm1, (var.z / ws) * nm1, n);
    } else {
        R.accum_out[i] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        R.moments_out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

void launch_reproject(const ReprojectLaunch &R, hipStream_t s)
{
    if (R.width <= 0 || R.rows <= 0) return;
    const uint32_t ntiles = (uint32_t)((R.width + 7) / 8) * (uint32_t)((R.rows + 7) / 8);      // (at most 4096 x 4096: the grid is never capped)
    hipLaunchKernelGGL(k_reproject, dim3((ntiles + RP_WAVES - 1) / RP_WAVES), dim3(256), 0, s, R);
}

}  // namespace pt
