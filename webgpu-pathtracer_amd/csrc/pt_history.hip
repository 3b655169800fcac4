// pt_history.hip -- a held history validated against fresh samples before it is merged (include/mi3pt.h: mi3pt_hold_history,
// mi3pt_merge_history).
//
// Two (mean, moments) pairs over the same texels: the live one (A, M), sampled since the hold, and the held one (Ah, Mh), carried from
// before it.  Every texel pools the difference of the two means and the variance of that difference over a (2r + 1)^2 window, turns the
// pooled z-score into the share of the held samples it keeps, and combines the two pairs by Chan's pairwise rule.  The arithmetic is the
// header's, operation for operation (DESIGN.md "Pinned arithmetic": fp32, nothing contracted, correctly rounded division);
// tests/history_reference.py restates it in numpy and tests/test_gpu_history.py holds this file to it bit for bit.
//
// One 32 x 8 tile per block of four waves; a wave is two tile rows of 32 texels, so a lane's loads and stores are 16 B and a tile row
// is 512 contiguous bytes.  What a texel contributes to every window it lies in -- d.xyz, v.xyz and the pair flag -- is computed ONCE and
// staged in LDS with a halo of r texels (the eight divisions of a tap are the expensive part: a window read straight from the images
// would repeat them up to 49 times).  Seven planes of (32 + 2r) x (8 + 2r) words: 9.3 KiB at r = 1, 14.5 KiB at r = 3.  A window row read is
// 32 consecutive words per half wave whatever the row stride: no bank conflict (ds_read_b32 banks per 32-lane half).  The radius is
// a template parameter: the halo's index arithmetic and the window loops are constants.  Every index is range-checked before it is used:
// images of NaNs or infinities neither hang nor fault.  It writes EVERY texel of the two output images: a texel outside the accumulate
// block's rectangle is copied, so that the outputs can take the inputs' place.
#include "../../include/mi3pt.h"
#include "pt_kernels.h"
#include "pt_devmath.h"
#include "pt_accum.h"

namespace pt {

constexpr int HT_W = 32, HT_H = 8;        // the tile: 256 threads, thread t at (t & 31, t >> 5)

// what one texel contributes to the windows it lies in (pair: both sides hold at least one sample)
struct HistoryTap { f3 d, v; uint32_t pair; };

PT_DEV f3 per_sample_variance(const float4 &m)
{
    if (!(m.w >= 2.0f)) return F3(0.0f, 0.0f, 0.0f);
    const float nm1 = m.w - 1.0f;
    return F3(fmaxf(m.x / nm1, 0.0f), fmaxf(m.y / nm1, 0.0f), fmaxf(m.z / nm1, 0.0f));
}

PT_DEV HistoryTap history_tap(const float4 &a, const float4 &m, const float4 &ah, const float4 &mh)
{
    HistoryTap t;
    t.d = t.v = F3(0.0f, 0.0f, 0.0f);
    t.pair = (m.w >= 1.0f && mh.w >= 1.0f) ? 1u : 0u;        // (a NaN fails)
    if (!t.pair) return t;
    const f3 sf = per_sample_variance(m), sh = per_sample_variance(mh);
    const float w = 1.0f / m.w + 1.0f / mh.w;
    t.d = F3(a.x - ah.x, a.y - ah.y, a.z - ah.z);
    t.v = F3(fmaxf(sf.x, sh.x) * w, fmaxf(sf.y, sh.y) * w, fmaxf(sf.z, sh.z) * w);
    return t;
}

template <int R>
__global__ void __launch_bounds__(256) k_history(const HistoryLaunch H)
{
    constexpr int SW = HT_W + 2 * R, SH = HT_H + 2 * R, NE = SW * SH, HALO = NE - HT_W * HT_H;
    __shared__ float s_val[6][NE];        // d.x, d.y, d.z, v.x, v.y, v.z
    __shared__ uint32_t s_pair[NE];
    const int tid = (int)threadIdx.x, tx = tid & (HT_W - 1), ty = tid >> 5;
    const int x0 = (int)blockIdx.x * HT_W, y0 = (int)blockIdx.y * HT_H;
    const auto in_rect = [&](int gx, int gy) {
        return gx >= 0 && gy >= 0 && gx < H.width && gy < H.rows && (uint32_t)gx < H.res_w && (uint32_t)gy < H.res_h;
    };
    const auto stage = [&](int e, const HistoryTap &t) {
        s_val[0][e] = t.d.x; s_val[1][e] = t.d.y; s_val[2][e] = t.d.z;
        s_val[3][e] = t.v.x; s_val[4][e] = t.v.y; s_val[5][e] = t.v.z;
        s_pair[e] = t.pair;
    };
    // this thread's own texel: kept in registers for the merge
    const int x = x0 + tx, y = y0 + ty;
    const bool in_image = x < H.width && y < H.rows, inside = in_rect(x, y);
    const size_t i = (size_t)y * (size_t)H.width + (size_t)x;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 a = zero, m = zero, ah = zero, mh = zero;
    if (in_image) { a = H.accum[i]; m = H.moments[i]; }
    if (inside) { ah = H.accum_held[i]; mh = H.moments_held[i]; }
    const HistoryTap own = history_tap(a, m, ah, mh);        // (outside the rectangle: n = nh = 0, no pair)
    stage((ty + R) * SW + (tx + R), own);
    // the halo: R rows above, R rows below, R columns on either side
    for (int h = tid; h < HALO; h += 256) {
        int ix, iy;
        if (h < 2 * R * SW) {
            const int band = h / SW;        // 0 .. 2R - 1
            ix = h - band * SW;
            iy = band < R ? band : band + HT_H;
        } else {
            const int s = h - 2 * R * SW, row = s / (2 * (R > 0 ? R : 1)), c = s - row * 2 * R;
            ix = c < R ? c : c + HT_W;
            iy = row + R;
        }
        const int gx = x0 + ix - R, gy = y0 + iy - R;
        HistoryTap t;
        t.d = t.v = F3(0.0f, 0.0f, 0.0f);
        t.pair = 0u;
        if (in_rect(gx, gy)) {
            const size_t q = (size_t)gy * (size_t)H.width + (size_t)gx;
            t = history_tap(H.accum[q], H.moments[q], H.accum_held[q], H.moments_held[q]);
        }
        stage(iy * SW + ix, t);
    }
    __syncthreads();
    if (!in_image) return;
    float4 oa = a, om = m;        // outside the rectangle, dropped, neither: the texel keeps the live bits
    const float n = m.w, nh = mh.w;
    if (inside && n >= 1.0f) {
        if (nh >= 1.0f) {
            f3 D = F3(0.0f, 0.0f, 0.0f), V = F3(0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int dy = 0; dy <= 2 * R; dy++)
#pragma unroll
                for (int dx = 0; dx <= 2 * R; dx++) {
                    const int e = (ty + dy) * SW + (tx + dx);
                    if (!s_pair[e]) continue;
                    D = F3(D.x + s_val[0][e], D.y + s_val[1][e], D.z + s_val[2][e]);
                    V = F3(V.x + s_val[3][e], V.y + s_val[4][e], V.z + s_val[5][e]);
                }
            const float zx = (D.x * D.x) / (V.x + MI3PT_HISTORY_EPS), zy = (D.y * D.y) / (V.y + MI3PT_HISTORY_EPS),
                        zz = (D.z * D.z) / (V.z + MI3PT_HISTORY_EPS);
            const float z2 = fmaxf(fmaxf(zx, zy), zz);
            const float drop2 = H.z_drop * H.z_drop, keep2 = H.z_keep * H.z_keep;
            const float lam = fminf(fmaxf((drop2 - z2) / (drop2 - keep2), 0.0f), 1.0f);
            const float nk = floorf(nh * lam);
            if (nk >= 1.0f) {        // merged (a NaN drops)
                const f3 sh = per_sample_variance(mh);
                const float N = n + nk, f = nk / N, nf = n * f, nk1 = nk - 1.0f;
                const f3 d = F3(ah.x - a.x, ah.y - a.y, ah.z - a.z);
                oa = make_float4(store_round(a.x + d.x * f, H.store_f16), store_round(a.y + d.y * f, H.store_f16),
                                 store_round(a.z + d.z * f, H.store_f16), 1.0f);
                om = make_float4((m.x + sh.x * nk1) + (d.x * d.x) * nf, (m.y + sh.y * nk1) + (d.y * d.y) * nf,
                                 (m.z + sh.z * nk1) + (d.z * d.z) * nf, N);
            }
        }
    } else if (inside && nh >= 1.0f) {        // only held: the texel takes the held bits
        oa = ah;
        om = mh;
    }
    H.accum_out[i] = oa;
    H.moments_out[i] = om;
}

void launch_history(const HistoryLaunch &H, hipStream_t s)
{
    if (H.width <= 0 || H.rows <= 0) return;
    // (at most 32768 x 32768: 1024 x 4096 blocks, inside the grid's limits)
    const dim3 grid((uint32_t)((H.width + HT_W - 1) / HT_W), (uint32_t)((H.rows + HT_H - 1) / HT_H));
    switch (H.radius) {
    case 0: hipLaunchKernelGGL(k_history<0>, grid, dim3(256), 0, s, H); break;
    case 1: hipLaunchKernelGGL(k_history<1>, grid, dim3(256), 0, s, H); break;
    case 2: hipLaunchKernelGGL(k_history<2>, grid, dim3(256), 0, s, H); break;
    case 3: hipLaunchKernelGGL(k_history<3>, grid, dim3(256), 0, s, H); break;
    default: break;        // (mi3pt_merge_history refuses other radii)
    }
}

}  // namespace pt
