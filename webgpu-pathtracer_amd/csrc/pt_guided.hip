// pt_guided.hip -- the feature-guided a-trous de-noise of the running mean (include/mi3pt.h: mi3pt_denoise_guided).
//
// An edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global
// Illumination Filtering", HPG 2010) over the accumulation image, guided by the first-hit feature images.  The arithmetic is the header's,
// operation for operation (DESIGN.md "Pinned arithmetic": fp32, nothing contracted, correctly rounded division, ptm::exp1_nonpos);
// tests/guided_reference.py restates it in numpy and tests/test_gpu_guided.py holds this file to it bit for bit.
//
// One launch per level.  Level i looks at the texels 2^i apart, so the image falls into 4^i independent STRIDE CLASSES (x mod s, y mod s) and
// inside a class the 5 x 5 taps are neighbours: a 256-thread block filters 16 x 16 texels of one class, copies the 20 x 20 texels of that
// class around them (colour and features, 64 B per texel = 25 KB) into LDS once and runs the 25 taps from there -- every level is the same
// kernel with the stride as an argument.  A texel outside the image is marked in its LDS record and never loaded.
#include "../../include/mi3pt.h"
#include "pt_kernels.h"
#include "pt_devmath.h"
#include "pt_moments.h"

namespace pt {

constexpr int G_TILE = 16, G_HALO = 2, G_SPAN = G_TILE + 2 * G_HALO;      // 20 x 20 records per block

// normal.xyz and the hit flag (word 2 of the ids image) in one record: the filter reads one image less per level
__global__ void __launch_bounds__(256) k_guided_pack(const float4 *__restrict__ normal, const float4 *__restrict__ ids, float4 *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 nn = normal[i];
    out[i] = make_float4(nn.x, nn.y, nn.z, __uint_as_float(reinterpret_cast<const uint4 *>(ids)[i].z));       // (the flag's 32 bits: only ever compared as bits)
}

// One level for one texel block.  VARIANCE (MI3PT_GUIDED_VARIANCE): the colour term is |dc|^2 / (k_c * var(p) + EPS) -- `color` = k_c, no 4^level
// factor -- instead of |dc|^2 * `color` (= inv_c), and the variance is filtered with the squared weights beside the colour: it rides in the w
// slot of the LDS colour record, so the centre's alpha comes from memory.  One body, so that the two kernels cannot drift apart; the plain
// instantiation compiles to what it was (profiles/moments.log).
template <bool VARIANCE>
PT_DEV void guided_level(const GuidedLaunch &G, const float4 *__restrict__ src, float4 *__restrict__ dst, const float *__restrict__ var_src,
                         float *__restrict__ var_dst, const int s, const float color, const int color_on)
{
    __shared__ float4 l_col[G_SPAN * G_SPAN];       // c.rgb, c.w (VARIANCE: the variance)
    __shared__ float4 l_nh[G_SPAN * G_SPAN];        // n.xyz, hit
    __shared__ float4 l_pos[G_SPAN * G_SPAN];       // P.xyz, w: bits 1 = inside the image
    __shared__ float4 l_alb[G_SPAN * G_SPAN];       // a.rgb
    // the block's stride class and its 16 x 16 tile of class coordinates (texel = coordinate * s + class)
    const int cx = (int)blockIdx.x % s, cy = (int)blockIdx.y % s;
    const int u0 = ((int)blockIdx.x / s) * G_TILE, v0 = ((int)blockIdx.y / s) * G_TILE;
    for (int e = (int)threadIdx.x; e < G_SPAN * G_SPAN; e += 256) {
        const int x = (u0 - G_HALO + e % G_SPAN) * s + cx, y = (v0 - G_HALO + e / G_SPAN) * s + cy;
        const bool inside = x >= 0 && x < G.width && y >= 0 && y < G.rows;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nh = c, p = c, a = c;
        if (inside) {
            const size_t i = (size_t)y * (size_t)G.width + (size_t)x;
            c = src[i]; nh = G.normal_hit[i]; p = G.position[i]; a = G.albedo[i];
            if (VARIANCE) c.w = var_src[i];
            p.w = __uint_as_float(1u);
        }
        l_col[e] = c; l_nh[e] = nh; l_pos[e] = p; l_alb[e] = a;
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % G_TILE, ly = (int)threadIdx.x / G_TILE;
    const int x = (u0 + lx) * s + cx, y = (v0 + ly) * s + cy;
    if (x >= G.width || y >= G.rows) return;
    const int ec0 = (ly + G_HALO) * G_SPAN + lx + G_HALO;
    const float4 cp = l_col[ec0], np = l_nh[ec0], pp = l_pos[ec0], ap = l_alb[ec0];
    const uint32_t hit_p = __float_as_uint(np.w);
    const float denom = VARIANCE ? color * cp.w + MI3PT_GUIDED_VARIANCE_EPS : 0.0f;
    const float h[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float den = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f, nv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int e = ec0 + dy * G_SPAN + dx;
            const float4 pq = l_pos[e], nq = l_nh[e];
            if (__float_as_uint(pq.w) != 1u || __float_as_uint(nq.w) != hit_p) continue;
            const float4 cq = l_col[e], aq = l_alb[e];
            const float dcx = cq.x - cp.x, dcy = cq.y - cp.y, dcz = cq.z - cp.z;
            const float dc2 = (dcx * dcx + dcy * dcy) + dcz * dcz;
            const float ec = VARIANCE ? (color_on ? dc2 / denom : 0.0f) : dc2 * color;
            const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
            const float en = ((dnx * dnx + dny * dny) + dnz * dnz) * G.inv_normal;
            const float dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
            const float ea = ((dax * dax + day * day) + daz * daz) * G.inv_albedo;
            const float dpx = pq.x - pp.x, dpy = pq.y - pp.y, dpz = pq.z - pp.z;
            const float pd = (np.x * dpx + np.y * dpy) + np.z * dpz;
            const float ep = (pd * pd) * G.inv_plane;
            const float w = ptm::exp1_nonpos(-(((ec + en) + ea) + ep)) * (h[dx + 2] * h[dy + 2]);
            den = den + w;
            nr = nr + w * cq.x; ng = ng + w * cq.y; nb = nb + w * cq.z;
            if (VARIANCE) nv = nv + (w * w) * cq.w;
        }
    }
    const size_t i = (size_t)y * (size_t)G.width + (size_t)x;
    dst[i] = make_float4(nr / den, ng / den, nb / den, VARIANCE ? src[i].w : cp.w);
    if (VARIANCE) var_dst[i] = nv / (den * den);
}

__global__ void __launch_bounds__(256) k_guided_level(const GuidedLaunch G, const float4 *__restrict__ src, float4 *__restrict__ dst, const int s,
                                                      const float inv_c)
{
    guided_level<false>(G, src, dst, nullptr, nullptr, s, inv_c, 1);
}

// ---- MI3PT_GUIDED_VARIANCE: the colour term steered by the per-pixel variance of the mean (SVGF's spatial filter: Schied et al.,
// HPG 2017), from the moments image, carried from level to level: the variance kernel and guided_level's second instantiation. ----

// The firefly pre-pass's part in var_0 (mi3pt_set_guided_despike): the variance of a scaled variable, var_0(p) * (s * s), for the texels
// the pre-pass clamped -- `scale` holds 1 for every other texel, whose var_0 keeps its bits.  DESPIKED false: `v` itself, nothing read;
// the kernels of a context that never enables the state are those instantiations, compiled to what they were.
template <bool DESPIKED>
PT_DEV float despiked_variance(const float v, const float *__restrict__ scale, const size_t i)
{
    if (!DESPIKED) return v;
    const float s = scale[i];
    return s != 1.0f ? v * (s * s) : v;
}

// var_0: v (moments_variance, pt_moments.h) averaged over the 3 x 3 neighbours of the centre's hit class, g = [1/4, 1/2, 1/4]
template <bool DESPIKED>
PT_DEV void guided_variance(const float4 *__restrict__ moments, const float4 *__restrict__ normal_hit, float *__restrict__ var,
                            const float *__restrict__ scale, const int width, const int rows)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)width * (size_t)rows) return;
    const int y = (int)(i / (size_t)width), x = (int)(i - (size_t)y * (size_t)width);
    const uint32_t hit_p = __float_as_uint(normal_hit[i].w);
    const float g[3] = { 0.25f, 0.5f, 0.25f };
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
            if (__float_as_uint(normal_hit[q].w) != hit_p) continue;
            const float w = g[dx + 1] * g[dy + 1];
            num = num + w * moments_variance(moments[q]);
            den = den + w;
        }
    }
    var[i] = despiked_variance<DESPIKED>(num / den, scale, i);
}

__global__ void __launch_bounds__(256) k_guided_variance(const float4 *__restrict__ moments, const float4 *__restrict__ normal_hit,
                                                         float *__restrict__ var, const int width, const int rows)
{
    guided_variance<false>(moments, normal_hit, var, nullptr, width, rows);
}

__global__ void __launch_bounds__(256) k_guided_variance_despiked(const float4 *__restrict__ moments, const float4 *__restrict__ normal_hit,
                                                                  float *__restrict__ var, const float *__restrict__ scale, const int width,
                                                                  const int rows)
{
    guided_variance<true>(moments, normal_hit, var, scale, width, rows);
}

__global__ void __launch_bounds__(256) k_guided_level_variance(const GuidedLaunch G, const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                               const float *__restrict__ var_src, float *__restrict__ var_dst, const int s,
                                                               const float k_c, const int color_on)
{
    guided_level<true>(G, src, dst, var_src, var_dst, s, k_c, color_on);
}

// ---- MI3PT_GUIDED_YOUNG: var_0 for an image whose texels differ in age (after a reprojection most carry a long history and the
// disoccluded ones restart at n = 1).  A texel with fewer than MI3PT_GUIDED_YOUNG_COUNT samples takes the variance of the samples its
// 7 x 7 neighbours hold, pooled by Chan's pairwise rule from their own (mean, M2, n); the others keep k_guided_variance's 3 x 3, a
// young neighbour left out.
//
// Shaped as pt_history.hip: one 32 x 8 tile per block of four waves, a wave is two tile rows of 32 texels, so a tile row is 512
// contiguous bytes of every image.  What the 49 taps read is staged once per block with a halo of 3, as guided_level stages it: four
// float4 records per texel, 38 x 14 x 64 B = 33.25 KiB.  A lane reads whole records (ds_read_b128), the 32 lanes of a half wave at
// consecutive 16-byte slots whatever the row stride: each of the instruction's 16-lane groups covers the 16 slots of a bank row once,
// no conflict.  Four blocks = four waves per SIMD fit in a CU's 160 KiB; a 16 x 16 tile would stage 484 records instead of 532 but put
// two rows into a half wave, and a 64 x 4 tile 700.  The weights of pass 1 stay in registers for pass 2 (both loops are unrolled: 49
// registers, inside the 128 that four waves per SIMD leave each lane), so the features are read and the exp is taken once per tap.
// Left to itself the compiler hoists the 196 record reads of the unrolled pass in front of the arithmetic: 233 registers, two waves
// per SIMD, or 116 spilled under the bound.  A scheduling barrier after every tap keeps a tap's reads with its arithmetic: 85
// registers, no scratch (-Rpass-analysis=kernel-resource-usage).
// The usual block after a camera move holds no young texel: it decides that with one __syncthreads_or BEFORE any staging, runs the
// 3 x 3 from global memory and stages nothing.  Every index is range-checked before it is used. ----
constexpr int Y_W = 32, Y_H = 8, Y_R = 3, Y_SW = Y_W + 2 * Y_R, Y_SH = Y_H + 2 * Y_R, Y_NE = Y_SW * Y_SH;      // 38 x 14 records
constexpr int Y_TAPS = (2 * Y_R + 1) * (2 * Y_R + 1);

// var_0 of a centre that is not young: k_guided_variance's sum, operation for operation, over the taps that are not young either.  All nine
// taps are loaded first, from coordinates clamped into the image, and looked at afterwards: nine independent pairs of loads in flight per
// lane instead of a chain of load, test, load (the light path has half of k_guided_variance's waves per SIMD to hide them with).  Valid
// for a lane outside the image too, whose result nobody reads.  n_p: the centre's own count.
PT_DEV float guided_variance_settled(const float4 *__restrict__ moments, const float4 *__restrict__ normal_hit, const int x, const int y,
                                     const int width, const int rows, float &n_p)
{
    float4 m[9];
    uint32_t hit[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int qx = min(max(x + k % 3 - 1, 0), width - 1), qy = min(max(y + k / 3 - 1, 0), rows - 1);
        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
        hit[k] = __float_as_uint(normal_hit[q].w);
        m[k] = moments[q];
    }
    n_p = m[4].w;
    const float g[3] = { 0.25f, 0.5f, 0.25f };
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {        // dy outer, dx inner
        const int dx = k % 3 - 1, dy = k / 3 - 1, qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= width || qy < 0 || qy >= rows || hit[k] != hit[4]) continue;
        if (k != 4 && m[k].w < MI3PT_GUIDED_YOUNG_COUNT) continue;
        const float w = g[dx + 1] * g[dy + 1];
        num = num + w * moments_variance(m[k]);
        den = den + w;
    }
    return num / den;
}

template <bool DESPIKED>
PT_DEV void guided_variance_young(const GuidedLaunch &G, const float4 *__restrict__ accum, const float4 *__restrict__ moments,
                                  float *__restrict__ var, const float *__restrict__ scale)
{
    __shared__ float4 l_cn[Y_NE];        // c.rgb, n (0 outside the image: such a tap never counts)
    __shared__ float4 l_nh[Y_NE];        // n.xyz, hit
    __shared__ float4 l_ps[Y_NE];        // P.xyz, s = (M2.r + M2.g) + M2.b
    __shared__ float4 l_alb[Y_NE];       // a.rgb
    const int tid = (int)threadIdx.x, tx = tid & (Y_W - 1), ty = tid >> 5;
    const int x0 = (int)blockIdx.x * Y_W, y0 = (int)blockIdx.y * Y_H;
    const int x = x0 + tx, y = y0 + ty;
    const bool in_image = x < G.width && y < G.rows;
    const size_t i = (size_t)y * (size_t)G.width + (size_t)x;
    float n_p;
    const float settled = guided_variance_settled(moments, G.normal_hit, x, y, G.width, G.rows, n_p);        // (its loads are in flight before the vote)
    const bool young = in_image && n_p < MI3PT_GUIDED_YOUNG_COUNT;        // (a NaN count is not young)
    if (!__syncthreads_or(young ? 1 : 0)) {
        if (in_image) var[i] = despiked_variance<DESPIKED>(settled, scale, i);
        return;
    }
    for (int e = tid; e < Y_NE; e += 256) {
        const int iy = e / Y_SW, ix = e - iy * Y_SW;
        const int gx = x0 - Y_R + ix, gy = y0 - Y_R + iy;
        float4 cn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nh = cn, ps = cn, al = cn;
        if (gx >= 0 && gx < G.width && gy >= 0 && gy < G.rows) {
            const size_t q = (size_t)gy * (size_t)G.width + (size_t)gx;
            const float4 c = accum[q], mq = moments[q], p = G.position[q];
            cn = make_float4(c.x, c.y, c.z, mq.w);
            ps = make_float4(p.x, p.y, p.z, (mq.x + mq.y) + mq.z);
            nh = G.normal_hit[q]; al = G.albedo[q];
        }
        l_cn[e] = cn; l_nh[e] = nh; l_ps[e] = ps; l_alb[e] = al;
    }
    __syncthreads();
    if (!in_image) return;
    const int ec0 = (ty + Y_R) * Y_SW + tx + Y_R;
    const float4 np = l_nh[ec0], pp = l_ps[ec0], ap = l_alb[ec0];
    const uint32_t hit_p = __float_as_uint(np.w);
    if (!young) {
        var[i] = despiked_variance<DESPIKED>(settled, scale, i);
        return;
    }
    if (!(n_p >= 1.0f)) {        // never sampled
        var[i] = 0.0f;
        return;
    }
    // pass 1: the weights, the pooled count and the pooled mean
    float wgt[Y_TAPS];
    uint64_t counted = 0;
    float N = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
#pragma unroll
    for (int dy = -Y_R; dy <= Y_R; dy++) {
#pragma unroll
        for (int dx = -Y_R; dx <= Y_R; dx++) {
            const int k = (dy + Y_R) * (2 * Y_R + 1) + dx + Y_R, e = ec0 + dy * Y_SW + dx;
            const float4 cq = l_cn[e], nq = l_nh[e];
            wgt[k] = 0.0f;
            if (__float_as_uint(nq.w) != hit_p || !(cq.w >= 1.0f)) continue;
            float w = 1.0f;
            if ((dx | dy) != 0) {
                const float4 pq = l_ps[e], aq = l_alb[e];
                const float dnx = nq.x - np.x, dny = nq.y - np.y, dnz = nq.z - np.z;
                const float en = ((dnx * dnx + dny * dny) + dnz * dnz) * G.inv_normal;
                const float dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
                const float ea = ((dax * dax + day * day) + daz * daz) * G.inv_albedo;
                const float dpx = pq.x - pp.x, dpy = pq.y - pp.y, dpz = pq.z - pp.z;
                const float pd = (np.x * dpx + np.y * dpy) + np.z * dpz;
                const float ep = (pd * pd) * G.inv_plane;
                w = ptm::exp1_nonpos(-((en + ea) + ep));
            }
            wgt[k] = w;
            counted |= 1ull << k;
            const float a = w * cq.w;
            N = N + a;
            ar = ar + a * cq.x; ag = ag + a * cq.y; ab = ab + a * cq.z;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const float mr = ar / N, mg = ag / N, mb = ab / N;
    // pass 2: Chan's rule -- every counted texel's own M2 plus its count times the squared distance of its mean from the pooled one
    float ss = 0.0f;
#pragma unroll
    for (int dy = -Y_R; dy <= Y_R; dy++) {
#pragma unroll
        for (int dx = -Y_R; dx <= Y_R; dx++) {
            const int k = (dy + Y_R) * (2 * Y_R + 1) + dx + Y_R, e = ec0 + dy * Y_SW + dx;
            if (!((counted >> k) & 1ull)) continue;
            const float4 cq = l_cn[e];
            const float s_q = l_ps[e].w;
            const float ddx = cq.x - mr, ddy = cq.y - mg, ddz = cq.z - mb;
            const float d2 = (ddx * ddx + ddy * ddy) + ddz * ddz;
            ss = ss + wgt[k] * (s_q + cq.w * d2);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const float v = N >= 2.0f ? fmaxf(ss / (N - 1.0f), 0.0f) : 0.0f;
    var[i] = despiked_variance<DESPIKED>((v / n_p) * (MI3PT_GUIDED_YOUNG_COUNT / n_p), scale, i);
}

__global__ void __launch_bounds__(256, 4) k_guided_variance_young(const GuidedLaunch G, const float4 *__restrict__ accum,
                                                                  const float4 *__restrict__ moments, float *__restrict__ var)
{
    guided_variance_young<false>(G, accum, moments, var, nullptr);
}

__global__ void __launch_bounds__(256, 4) k_guided_variance_young_despiked(const GuidedLaunch G, const float4 *__restrict__ accum,
                                                                           const float4 *__restrict__ moments, float *__restrict__ var,
                                                                           const float *__restrict__ scale)
{
    guided_variance_young<true>(G, accum, moments, var, scale);
}

// ---- The firefly pre-pass (include/mi3pt.h: mi3pt_set_guided_despike): a texel brighter than every 3 x 3 neighbour of its own class
// (material and hit flag, words 1 and 2 of the ids image) is scaled down to the brightest of them, into `out`, the image level 0 and the
// young kernel then read in the accumulation image's place; `scale` (null outside the variance modes) takes s for the var_0 kernels.
//
// One launch over two images, shaped as the young kernel: a 32 x 8 tile per block of four waves, a tile row 512 contiguous bytes.  A
// lane loads its own texel once -- colour and ids, both kept in registers for the output -- and leaves what the eight taps need in LDS:
// the luminance and the two class words, three 4-byte arrays of 34 x 10 (4 080 B per block: no bound on occupancy), the 84 halo records
// by the block's first 84 lanes.  A half wave reads 32 consecutive words of an array per tap: no bank conflict.  A tap outside the image
// is decided from its coordinates; its record holds zeros and is never looked at.  Every index is range-checked before it is used.
// The count: one ballot per wave and one vector atomic add by its first lane, none from a wave that clamped nothing.  With a firefly in
// most waves that is one add per 64 texels, and onto ONE word they queue behind each other in the L2: 32 400 adds at 1080p cost 284 us
// against the 25 us of the pass itself (profiles/guided_despike.log).  So the count is kept in DESPIKE_SLOTS words 128 B apart
// (pt_kernels.h), a wave adds to the slot of its number in the grid, and the host sums the slots after the read-back. ----
constexpr int D_W = 32, D_H = 8, D_SW = D_W + 2, D_SH = D_H + 2, D_NE = D_SW * D_SH, D_RING = 2 * D_SW + 2 * D_H;      // 34 x 10 records, 84 of them halo

__global__ void __launch_bounds__(256) k_guided_despike(const float4 *__restrict__ accum, const float4 *__restrict__ ids, float4 *__restrict__ out,
                                                        float *__restrict__ scale, uint32_t *__restrict__ count, const int width, const int rows)
{
    __shared__ float l_lum[D_NE];
    __shared__ uint32_t l_mat[D_NE], l_hit[D_NE];
    const int tid = (int)threadIdx.x, tx = tid & (D_W - 1), ty = tid >> 5;
    const int x0 = (int)blockIdx.x * D_W, y0 = (int)blockIdx.y * D_H;
    const int x = x0 + tx, y = y0 + ty;
    const bool in_image = x < width && y < rows;
    const size_t i = (size_t)y * (size_t)width + (size_t)x;
    const int ec0 = (ty + 1) * D_SW + tx + 1;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float lum_p = 0.0f;
    uint32_t mat_p = 0u, hit_p = 0u;
    if (in_image) {
        c = accum[i];
        const uint4 id = reinterpret_cast<const uint4 *>(ids)[i];
        lum_p = ((c.x + c.y) + c.z) * (1.0f / 3.0f);
        mat_p = id.y; hit_p = id.z;
    }
    l_lum[ec0] = lum_p; l_mat[ec0] = mat_p; l_hit[ec0] = hit_p;
    if (tid < D_RING) {
        // the halo: the row before the tile, the row after it, the column left of it, the column right of it
        const int ix = tid < 2 * D_SW ? tid % D_SW : (tid < 2 * D_SW + D_H ? 0 : D_SW - 1);
        const int iy = tid < D_SW ? 0 : (tid < 2 * D_SW ? D_SH - 1 : 1 + (tid - 2 * D_SW) % D_H);
        const int gx = x0 - 1 + ix, gy = y0 - 1 + iy;
        float lum = 0.0f;
        uint32_t mat = 0u, hit = 0u;
        if (gx >= 0 && gx < width && gy >= 0 && gy < rows) {
            const size_t q = (size_t)gy * (size_t)width + (size_t)gx;
            const float4 cq = accum[q];
            const uint4 id = reinterpret_cast<const uint4 *>(ids)[q];
            lum = ((cq.x + cq.y) + cq.z) * (1.0f / 3.0f);
            mat = id.y; hit = id.z;
        }
        const int e = iy * D_SW + ix;
        l_lum[e] = lum; l_mat[e] = mat; l_hit[e] = hit;
    }
    __syncthreads();
    bool clamped = false;
    if (in_image) {
        float cap = 0.0f;
        int m = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                if ((dx | dy) == 0) continue;
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
                const int e = ec0 + dy * D_SW + dx;
                if (l_mat[e] != mat_p || l_hit[e] != hit_p) continue;
                m++;
                cap = fmaxf(cap, l_lum[e]);        // (drops a NaN)
            }
        }
        clamped = m >= 1 && lum_p > cap;
        float s = 1.0f;
        if (clamped) {
            s = cap / lum_p;
            c.x = c.x * s; c.y = c.y * s; c.z = c.z * s;        // (alpha keeps its bits)
        }
        out[i] = c;
        if (scale) scale[i] = s;
    }
    const unsigned long long voted = __ballot(clamped);
    if ((tid & 63) == 0 && voted != 0ull) {
        const uint32_t wave = ((uint32_t)blockIdx.y * (uint32_t)gridDim.x + (uint32_t)blockIdx.x) * 4u + (uint32_t)(tid >> 6);
        atomicAdd(count + (size_t)(wave % DESPIKE_SLOTS) * DESPIKE_SLOT_WORDS, (uint32_t)__popcll(voted));
    }
}

void launch_guided_despike(const float4 *accum, const float4 *ids, float4 *out, float *scale, uint32_t *count, int width, int rows, hipStream_t s)
{
    if (width <= 0 || rows <= 0) return;
    // (at most 32768 x 32768: 1024 x 4096 blocks, inside the grid's limits)
    const dim3 grid((uint32_t)((width + D_W - 1) / D_W), (uint32_t)((rows + D_H - 1) / D_H));
    hipLaunchKernelGGL(k_guided_despike, grid, dim3(256), 0, s, accum, ids, out, scale, count, width, rows);
}

void launch_guided_variance_young(const GuidedLaunch &G, const float4 *accum, const float4 *moments, float *var, const float *scale, hipStream_t s)
{
    if (G.width <= 0 || G.rows <= 0) return;
    // (at most 32768 x 32768: 1024 x 4096 blocks, inside the grid's limits)
    const dim3 grid((uint32_t)((G.width + Y_W - 1) / Y_W), (uint32_t)((G.rows + Y_H - 1) / Y_H));
    if (scale)
        hipLaunchKernelGGL(k_guided_variance_young_despiked, grid, dim3(256), 0, s, G, accum, moments, var, scale);
    else
        hipLaunchKernelGGL(k_guided_variance_young, grid, dim3(256), 0, s, G, accum, moments, var);
}

void launch_guided_variance(const float4 *moments, const float4 *normal_hit, float *var, const float *scale, int width, int rows, hipStream_t s)
{
    const size_t texels = (size_t)width * (size_t)rows;
    if (width <= 0 || rows <= 0) return;
    const dim3 grid((unsigned)((texels + 255) / 256));
    if (scale)
        hipLaunchKernelGGL(k_guided_variance_despiked, grid, dim3(256), 0, s, moments, normal_hit, var, scale, width, rows);
    else
        hipLaunchKernelGGL(k_guided_variance, grid, dim3(256), 0, s, moments, normal_hit, var, width, rows);
}

void launch_guided_level_variance(const GuidedLaunch &G, const float4 *src, float4 *dst, const float *var_src, float *var_dst, int level,
                                  float sigma_color, hipStream_t s)
{
    if (G.width <= 0 || G.rows <= 0) return;
    const int step = 1 << level;
    const int tx = ((G.width + step - 1) / step + G_TILE - 1) / G_TILE, ty = ((G.rows + step - 1) / step + G_TILE - 1) / G_TILE;      // (as launch_guided_level)
    hipLaunchKernelGGL(k_guided_level_variance, dim3((unsigned)(tx * step), (unsigned)(ty * step)), dim3(256), 0, s, G, src, dst, var_src, var_dst,
                       step, sigma_color * sigma_color, sigma_color == 0.0f ? 0 : 1);
}

void launch_guided_pack(const float4 *normal, const float4 *ids, float4 *out, size_t texels, hipStream_t s)
{
    if (texels == 0) return;
    hipLaunchKernelGGL(k_guided_pack, dim3((unsigned)((texels + 255) / 256)), dim3(256), 0, s, normal, ids, out, texels);
}

void launch_guided_level(const GuidedLaunch &G, const float4 *src, float4 *dst, int level, hipStream_t s)
{
    if (G.width <= 0 || G.rows <= 0) return;
    const int step = 1 << level;
    // per axis: `step` classes x the tiles of the longest class (ceil(size / step) texels); blocks of a shorter class find no texel of theirs
    const int tx = ((G.width + step - 1) / step + G_TILE - 1) / G_TILE, ty = ((G.rows + step - 1) / step + G_TILE - 1) / G_TILE;
    const float inv_c = G.inv_color * (float)(1u << (2 * level));       // 4^level: sigma_color halves per level
    hipLaunchKernelGGL(k_guided_level, dim3((unsigned)(tx * step), (unsigned)(ty * step)), dim3(256), 0, s, G, src, dst, step, inv_c);
}

}  // namespace pt
