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

// var_0: v (moments_variance, pt_moments.h) averaged over the 3 x 3 neighbours of the centre's hit class, g = [1/4, 1/2, 1/4]
__global__ void __launch_bounds__(256) k_guided_variance(const float4 *__restrict__ moments, const float4 *__restrict__ normal_hit,
                                                         float *__restrict__ var, const int width, const int rows)
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
    var[i] = num / den;
}

__global__ void __launch_bounds__(256) k_guided_level_variance(const GuidedLaunch G, const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                               const float *__restrict__ var_src, float *__restrict__ var_dst, const int s,
                                                               const float k_c, const int color_on)
{
    guided_level<true>(G, src, dst, var_src, var_dst, s, k_c, color_on);
}

void launch_guided_variance(const float4 *moments, const float4 *normal_hit, float *var, int width, int rows, hipStream_t s)
{
    const size_t texels = (size_t)width * (size_t)rows;
    if (width <= 0 || rows <= 0) return;
    hipLaunchKernelGGL(k_guided_variance, dim3((unsigned)((texels + 255) / 256)), dim3(256), 0, s, moments, normal_hit, var, width, rows);
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
