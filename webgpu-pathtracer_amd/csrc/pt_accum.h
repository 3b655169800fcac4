// pt_accum.h -- the ordered running mean's device functions (accumulate.wgsl:12-29 for one texel, the moments image's step beside it, the
// tile split's row rule), shared by the kernels that WRITE the accumulation image: pt_kernels.hip (k_raytrace's fused pass,
// k_accumulate_frames) and pt_accumulate_tiles.hip (k_accumulate_tiles).  One copy: a masked run steps a texel with the very functions
// an unmasked run steps it with.
#pragma once
#include "pt_kernels.h"
#include "pt_devmath.h"

namespace pt {

struct f3 { float x, y, z; };

PT_DEV f3 F3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
PT_DEV f3 xyz(const float4 &v) { return F3(v.x, v.y, v.z); }
// pinned: mix(a, b, t) = a * (1 - t) + b * t
PT_DEV float mix1(float a, float b, float t) { return a * (1.0f - t) + b * t; }
PT_DEV f3 mix(f3 a, f3 b, float t) { return F3(mix1(a.x, b.x, t), mix1(a.y, b.y, t), mix1(a.z, b.z, t)); }

PT_DEV int local_to_global_row(int ly, const Tile &t)
{
    // The tile split (pt_kernels.h, Tile): local block b of rank r is block b * nranks + pos of the image, pos = r in even rounds of the
    // deal and nranks - 1 - r in odd ones -- back and forth, so that a cost that rises or falls down the image (floor, model, sky)
    // is shared out evenly (dealt one way only, rank 0 of eight got 5 % more work than rank 6: profiles/r04_rejected_and_adopted.log)
    if (t.nranks == 1) return ly;                     // (wave-uniform fast paths: no division for the whole image ...
    if (t.block_rows == 8) {                          // ... nor for the usual 8-row blocks)
        const int b = ly >> 3;
        return (((b * t.nranks + ((b & 1) ? t.nranks - 1 - t.rank : t.rank)) << 3) | (ly & 7));
    }
    const int b = ly / t.block_rows;
    return (b * t.nranks + ((b & 1) ? t.nranks - 1 - t.rank : t.rank)) * t.block_rows + (ly - b * t.block_rows);
}

PT_DEV float store_round(float v, int store_f16) { return store_f16 ? ptm::round_f16(v) : v; }

// accumulate.wgsl:18-28 for one texel
PT_DEV f3 accumulate_texel(const AccUniforms &acc, f3 color, f3 prev)
{
    float weight = 1.0f;
    if (acc.frame > 0u) weight = 1.0f / (float)acc.frame;
    weight = (acc.enabled == 1u) ? weight : 1.0f;
    return mix(prev, color, weight);
}

// The moments image (include/mi3pt.h: mi3pt_set_moments): (M2.rgb, n) kept beside the mean in the same pass.  Welford's update written
// around the mean as it is STORED: c the frame's radiance, p the mean before the step, pn the mean after it (after store_round); a step
// of weight 1 (accumulate_texel) restarts the sums.
PT_DEV float4 moments_step(const AccUniforms &acc, f3 c, f3 p, f3 pn, float4 m)
{
    if (acc.frame <= 1u || acc.enabled != 1u) return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    return make_float4(m.x + (c.x - p.x) * (c.x - pn.x), m.y + (c.y - p.y) * (c.y - pn.y), m.z + (c.z - p.z) * (c.z - pn.z), m.w + 1.0f);
}

// The mean BY COUNT (include/mi3pt.h: mi3pt_set_mean_by_count): the twins of the two functions above whose weight comes from the
// texel's own sample count n (the moments texel's w) instead of the block's `frame`.  A texel without history -- n NaN, zero or
// negative -- restarts like a step of weight 1; for n = frame - 1 the quotient and the restart are the default law's, bit for bit.
PT_DEV bool count_restarts(const AccUniforms &acc, float n) { return acc.enabled != 1u || !(n >= 1.0f); }

PT_DEV f3 accumulate_texel_by_count(const AccUniforms &acc, f3 color, f3 prev, float n)
{
    const float weight = count_restarts(acc, n) ? 1.0f : 1.0f / (n + 1.0f);
    return mix(prev, color, weight);
}

PT_DEV float4 moments_step_by_count(const AccUniforms &acc, f3 c, f3 p, f3 pn, float4 m)
{
    if (count_restarts(acc, m.w)) return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    return make_float4(m.x + (c.x - p.x) * (c.x - pn.x), m.y + (c.y - p.y) * (c.y - pn.y), m.z + (c.z - p.z) * (c.z - pn.z), m.w + 1.0f);
}

// one accumulate step of a texel: the mean p and, with MOMENTS, its moments texel m; BY_COUNT (needs MOMENTS) takes the weight from m.w
template <bool MOMENTS, bool BY_COUNT>
PT_DEV void mean_step(const AccUniforms &a, f3 c, f3 &p, float4 &m, int store_f16)
{
    static_assert(MOMENTS || !BY_COUNT, "the count is the moments texel's");
    const f3 nc = BY_COUNT ? accumulate_texel_by_count(a, c, p, m.w) : accumulate_texel(a, c, p);
    const f3 pn = F3(store_round(nc.x, store_f16), store_round(nc.y, store_f16), store_round(nc.z, store_f16));
    if (MOMENTS) m = BY_COUNT ? moments_step_by_count(a, c, p, pn, m) : moments_step(a, c, p, pn, m);
    p = pn;
}

}  // namespace pt
