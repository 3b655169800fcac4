// pt_converge.hip -- the per-tile error estimate of the running mean (include/mi3pt.h: mi3pt_estimate_convergence).
//
// A streaming reduction of (accumulation image, moments image) to one record per 8 x 8 tile and one summary: 32 B read per texel, 16 B
// written per 64 texels.  The arithmetic is the header's, operation for operation (DESIGN.md "Pinned arithmetic": fp32, nothing contracted,
// correctly rounded division); tests/convergence_reference.py restates it in numpy and tests/test_gpu_convergence.py holds this file to it
// bit for bit.
//
// One wave per tile: lane j = 8 * (row in tile) + (column in tile), so a lane's two loads are 16 B each and a tile row is 128 contiguous
// bytes.  The tile's sum is the header's halving tree as a xor-butterfly of wave shuffles (lane 0 ends with the tree's bits), max / min /
// count likewise: no LDS for the tile.  A block's four waves take four neighbouring tiles at a time (512 contiguous bytes per row), four
// times over, every load issued before the first reduction.  What the block's sixteen tiles add to the summary -- counts, and maxima of
// the bit patterns of non-negative floats -- is combined through 4 x 32 B of LDS and stored as ONE 32-byte record per block; a second,
// one-block kernel folds the records into the summary.  No atomics: the first version added each block's record to the summary with up
// to six integer atomics on one 64-byte line, 2025 blocks at 1920 x 1080, and took 137 us of which the reads are 11
// (profiles/convergence.log).  Integer sums and maxima: the summary does not depend on the order in which the records are folded.
#include "../../include/mi3pt.h"
#include "pt_kernels.h"
#include "pt_devmath.h"
#include "pt_moments.h"

namespace pt {

constexpr int CV_WAVES = 4, CV_ROUNDS = 4, CV_BLOCK_TILES = CV_WAVES * CV_ROUNDS;

// what one wave, then one block, adds to the summary: ConvergePart (pt_kernels.h)
PT_DEV void fold(ConvergePart &a, const ConvergePart &o)
{
    a.tiles += o.tiles; a.above += o.above; a.young += o.young; a.nonfinite += o.nonfinite; a.texels += o.texels;
    a.worst_tile = max(a.worst_tile, o.worst_tile);
    a.worst_texel = max(a.worst_texel, o.worst_texel);
    a.n_min_inv = max(a.n_min_inv, o.n_min_inv);
}

__global__ void __launch_bounds__(256) k_converge_tiles(const float4 *__restrict__ accum, const float4 *__restrict__ moments, float4 *__restrict__ tiles,
                                                        ConvergePart *__restrict__ parts, const int width, const int rows, const int tiles_x,
                                                        const uint32_t ntiles, const float t2, const float min_frames)
{
    __shared__ ConvergePart l_part[CV_WAVES];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    // every load of the wave's four tiles first: a texel outside the image, or of a tile past the last, reads as "never accumulated"
    float4 mo[CV_ROUNDS], c[CV_ROUNDS];
#pragma unroll
    for (int round = 0; round < CV_ROUNDS; round++) {
        const uint32_t t = (uint32_t)blockIdx.x * CV_BLOCK_TILES + (uint32_t)(round * CV_WAVES + wave);
        const int x = (int)(t % (uint32_t)tiles_x) * 8 + (lane & 7), y = (int)(t / (uint32_t)tiles_x) * 8 + (lane >> 3);
        mo[round] = c[round] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (t < ntiles && x < width && y < rows) {
            const size_t i = (size_t)y * (size_t)width + (size_t)x;
            mo[round] = moments[i];
            c[round] = accum[i];
        }
    }
    ConvergePart part = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };      // (lane 0's counts)
#pragma unroll
    for (int round = 0; round < CV_ROUNDS; round++) {
        const uint32_t t = (uint32_t)blockIdx.x * CV_BLOCK_TILES + (uint32_t)(round * CV_WAVES + wave);
        if (t >= ntiles) continue;      // (the whole wave)
        float sum = 0.0f, peak = 0.0f, n_min = __uint_as_float(0x7f800000u);
        const bool counts = mo[round].w >= 1.0f;         // (a NaN n does not count)
        if (counts) {
            const float v = moments_variance(mo[round]);
            const float s = ((c[round].x + c[round].y) + c[round].z) * (1.0f / 3.0f);
            const float m = s < 0.0f ? 0.0f : s;       // (a NaN mean stays a NaN)
            const float d = 1.0f + m;
            const float d2 = d * d;
            const float d4 = d2 * d2;
            const float r = v / d4;
            sum = r;
            peak = fmaxf(r, 0.0f);
            n_min = mo[round].w;
        }
        const uint32_t count = (uint32_t)__popcll(__ballot(counts));
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            sum = sum + __shfl_xor(sum, s);
            peak = fmaxf(peak, __shfl_xor(peak, s));
            n_min = fminf(n_min, __shfl_xor(n_min, s));
        }
        if (lane != 0) continue;
        if (count == 0u) {
            tiles[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            continue;
        }
        const float fcount = (float)count;
        tiles[t] = make_float4(sum, peak, fcount, n_min);
        const bool young = n_min < min_frames;
        const bool above = young || !(sum <= t2 * fcount);
        const bool nonfinite = !(fabsf(sum) < __uint_as_float(0x7f800000u));
        const float per_texel = sum / fcount;
        part.tiles += 1u;
        part.above += above ? 1u : 0u;
        part.young += young ? 1u : 0u;
        part.nonfinite += nonfinite ? 1u : 0u;
        part.texels += count;
        // (only a value above zero moves a maximum that starts at zero: a NaN and -0 never reach the bit patterns)
        part.worst_tile = max(part.worst_tile, per_texel > 0.0f ? __float_as_uint(per_texel) : 0u);
        part.worst_texel = max(part.worst_texel, peak > 0.0f ? __float_as_uint(peak) : 0u);
        part.n_min_inv = max(part.n_min_inv, ~__float_as_uint(n_min));      // (n_min >= 1: the smallest n has the largest complement)
    }
    if (lane == 0) l_part[wave] = part;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < CV_WAVES; w++) fold(part, l_part[w]);
    parts[blockIdx.x] = part;
}

// the blocks' records folded into the summary: one block, each thread a strided share, then the 256 threads through LDS
__global__ void __launch_bounds__(256) k_converge_summary(const ConvergePart *__restrict__ parts, const uint32_t nparts, ConvergeSummary *__restrict__ summary)
{
    __shared__ ConvergePart l_part[256];
    ConvergePart part = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };      // (texels: at most 32768 x 32768 = 2^30, mi3pt_resize's limit)
    for (uint32_t i = threadIdx.x; i < nparts; i += 256u) fold(part, parts[i]);
    l_part[threadIdx.x] = part;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) fold(l_part[threadIdx.x], l_part[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const ConvergePart all = l_part[0];
    ConvergeSummary out;
    out.tiles = all.tiles; out.above = all.above; out.young = all.young; out.nonfinite = all.nonfinite;
    out.texels = all.texels;
    out.worst_tile = all.worst_tile; out.worst_texel = all.worst_texel; out.n_min_inv = all.n_min_inv; out.pad = 0u;
    *summary = out;
}

uint32_t converge_blocks(int width, int rows)
{
    if (width <= 0 || rows <= 0) return 0u;
    const uint32_t ntiles = (uint32_t)((width + 7) / 8) * (uint32_t)((rows + 7) / 8);      // (at most 4096 x 4096: the grid is never capped)
    return (ntiles + CV_BLOCK_TILES - 1) / CV_BLOCK_TILES;
}

void launch_converge(const float4 *accum, const float4 *moments, float4 *tiles, ConvergePart *parts, ConvergeSummary *summary, int width,
                     int rows, float t2, float min_frames, hipStream_t s)
{
    const uint32_t nblocks = converge_blocks(width, rows);
    const int tiles_x = (width + 7) / 8, tiles_y = (rows + 7) / 8;
    if (nblocks)
        hipLaunchKernelGGL(k_converge_tiles, dim3(nblocks), dim3(256), 0, s, accum, moments, tiles, parts, width, rows, tiles_x,
                           (uint32_t)tiles_x * (uint32_t)tiles_y, t2, min_frames);
    hipLaunchKernelGGL(k_converge_summary, dim3(1), dim3(256), 0, s, parts, nblocks, summary);      // (no rows: the zero summary)
}

}  // namespace pt
