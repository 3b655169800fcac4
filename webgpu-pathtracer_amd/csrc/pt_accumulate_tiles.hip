// pt_accumulate_tiles.hip -- the ordered running mean over a LIST of 8 x 8 tiles (include/mi3pt.h: mi3pt_set_sample_mask).
//
// k_accumulate_frames (pt_kernels.hip) walks the whole image; under a sample mask the mean of a frozen tile must keep its bits and the
// pass's work must fall with the sampled tiles, so this kernel steps the listed tiles only.  The arithmetic of a texel is that kernel's,
// function for function (pt_accum.h: mean_step; frame order, the weight from the block's `frame` -- or, <true, true>, from the texel's count), and
// so are its tests, in its order: inside the image, the image row of the local row, the accumulate block's rectangle.
//
// pt_converge.hip's shape: one wave per listed tile, lane j = 8 * (row in tile) + (column in tile), so a lane's loads and stores are 16 B
// and a tile row is 128 contiguous bytes (one aligned line when the width is a multiple of 8); a block's four waves take four
// consecutive list entries.  The tile index is wave-uniform and read once.  A texel's mean is a dependent chain over the frames, its
// radiance loads are not: four slots are loaded before the chain consumes them, then a remainder loop.
#include "../../include/mi3pt.h"
#include "pt_kernels.h"
#include "pt_devmath.h"
#include "pt_accum.h"

namespace pt {

constexpr int AT_WAVES = 4, AT_UNROLL = 4;

template <bool MOMENTS, bool BY_COUNT>
PT_DEV void mean_step_k(const AccUniforms &acc0, int k, const float4 &slot, f3 &p, float4 &m, int store_f16)
{
    AccUniforms a = acc0;
    a.frame = acc0.frame + (uint32_t)k;
    mean_step<MOMENTS, BY_COUNT>(a, xyz(slot), p, m, store_f16);
}

template <bool MOMENTS, bool BY_COUNT = false>
__global__ void __launch_bounds__(256) k_accumulate_tiles(const AccUniforms acc0, const Tile tile, const uint32_t *__restrict__ list,
                                                          const uint32_t ntiles, const float4 *__restrict__ slots, const size_t slot_pixels,
                                                          const int nframes, float4 *__restrict__ accum, float4 *__restrict__ moments,
                                                          const int store_f16)
{
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const uint32_t entry = (uint32_t)blockIdx.x * AT_WAVES + (uint32_t)wave;
    if (entry >= ntiles) return;        // (the whole wave)
    const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[entry]);
    const uint32_t tiles_x = (uint32_t)(tile.tex_w + 7) >> 3, tiles_y = (uint32_t)(tile.local_rows + 7) >> 3;
    const uint32_t trow = t / tiles_x;
    if (trow >= tiles_y) return;        // (not a tile of this image: nothing is touched)
    const int gx = (int)(t - trow * tiles_x) * 8 + (lane & 7), ly = (int)trow * 8 + (lane >> 3);
    if (gx >= tile.tex_w || ly >= tile.local_rows) return;
    const int gy = local_to_global_row(ly, tile);
    if ((uint32_t)gx >= acc0.res_w || (uint32_t)gy >= acc0.res_h) return;
    const size_t i = (size_t)ly * (size_t)tile.tex_w + (size_t)gx;
    f3 p = xyz(accum[i]);
    float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (MOMENTS) m = moments[i];
    const float4 *s = slots + i;
    int k = 0;
    for (; k + AT_UNROLL <= nframes; k += AT_UNROLL) {
        float4 c[AT_UNROLL];
#pragma unroll
        for (int j = 0; j < AT_UNROLL; j++) c[j] = s[(size_t)(k + j) * slot_pixels];
#pragma unroll
        for (int j = 0; j < AT_UNROLL; j++) mean_step_k<MOMENTS, BY_COUNT>(acc0, k + j, c[j], p, m, store_f16);
    }
    for (; k < nframes; k++) mean_step_k<MOMENTS, BY_COUNT>(acc0, k, s[(size_t)k * slot_pixels], p, m, store_f16);
    accum[i] = make_float4(p.x, p.y, p.z, 1.0f);
    if (MOMENTS) moments[i] = m;
}

void launch_accumulate_tiles(const AccUniforms &acc0, const Tile &tile, const uint32_t *list, int ntiles, const float4 *slots,
                             size_t slot_pixels, int nframes, float4 *accum, float4 *moments, int store_f16, bool by_count, hipStream_t s)
{
    if (ntiles <= 0 || nframes <= 0 || !list || tile.local_rows <= 0 || tile.tex_w <= 0) return;
    const unsigned blocks = ((unsigned)ntiles + AT_WAVES - 1) / AT_WAVES;      // (at most 4096 x 4096 / 4 tiles: the grid is never capped)
    if (moments && by_count)      // (the mean by count: mi3pt_set_mean_by_count)
        hipLaunchKernelGGL((k_accumulate_tiles<true, true>), dim3(blocks), dim3(256), 0, s, acc0, tile, list, (uint32_t)ntiles, slots, slot_pixels, nframes,
                           accum, moments, store_f16);
    else if (moments)
        hipLaunchKernelGGL(k_accumulate_tiles<true>, dim3(blocks), dim3(256), 0, s, acc0, tile, list, (uint32_t)ntiles, slots, slot_pixels, nframes,
                           accum, moments, store_f16);
    else
        hipLaunchKernelGGL(k_accumulate_tiles<false>, dim3(blocks), dim3(256), 0, s, acc0, tile, list, (uint32_t)ntiles, slots, slot_pixels, nframes,
                           accum, moments, store_f16);
}

}  // namespace pt
