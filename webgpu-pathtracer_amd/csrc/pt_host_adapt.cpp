// pt_host_adapt.cpp -- adaptive sampling's host side (include/mi3pt.h: mi3pt_set_sample_mask): the rule that freezes converged tiles, and
// the composition of a launch's tile lists from the sample mask and the view's empty tiles.  Plain C++, no device: the CPU builds and
// tests/adaptive_reference.py cover it.
#include "pt_internal.h"

// The rule, as the header pins it.  records: tiles_y x tiles_x x (sum_r, max_r, count, n_min), mi3pt_read_convergence_tiles' layout.
extern "C" int mi3pt_host_freeze_tiles(const float *records, int tiles_x, int tiles_y, float threshold, int min_frames, int guard,
                                       uint8_t *mask_inout, uint32_t *sampled_out)
{
    if (tiles_x < 0 || tiles_y < 0) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_freeze_tiles: a negative map size");
    if (guard != 0 && guard != 1) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_freeze_tiles: guard must be 0 or 1");
    const size_t n = (size_t)tiles_x * (size_t)tiles_y;
    if (n != 0 && (!records || !mask_inout)) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    const float t2 = (threshold * threshold) * 3.0f;
    const float young_below = (float)min_frames;
    // 0: nothing counted (count == 0), 1: under the threshold, 2: above it
    std::vector<uint8_t> state(n);
    for (size_t t = 0; t < n; t++) {
        const float sum_r = records[4 * t], count = records[4 * t + 2], n_min = records[4 * t + 3];
        if (!(count > 0.0f)) { state[t] = 0; continue; }
        const bool young = n_min < young_below;
        const bool above = young || !(sum_r <= t2 * count);
        state[t] = above ? 2 : 1;
    }
    uint32_t sampled = 0;
    std::vector<uint8_t> next(n);
    for (int y = 0; y < tiles_y; y++)
        for (int x = 0; x < tiles_x; x++) {
            const size_t t = (size_t)y * (size_t)tiles_x + (size_t)x;
            bool keep = mask_inout[t] != 0;
            if (keep && state[t] == 0) keep = false;                     // nothing to sample
            else if (keep && state[t] == 1) {
                bool ring_quiet = true;
                if (guard == 1)
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++) {
                            const int ux = x + dx, uy = y + dy;
                            if ((dx == 0 && dy == 0) || ux < 0 || uy < 0 || ux >= tiles_x || uy >= tiles_y) continue;
                            if (state[(size_t)uy * (size_t)tiles_x + (size_t)ux] == 2) ring_quiet = false;
                        }
                keep = !ring_quiet;
            }
            next[t] = keep ? 1 : 0;
            sampled += keep ? 1u : 0u;
        }
    if (n) std::memcpy(mask_inout, next.data(), n);
    if (sampled_out) *sampled_out = sampled;
    return MI3PT_OK;
}

namespace pt {

// A launch's tile lists: A = sampled and not empty, S = sampled and empty, laid out [A, ascending | S, ascending].  mask: one byte per
// tile (null: every tile is sampled); empty: pt::sky_classify's map (null: no tile is empty).  sky_pixels: the in-bounds pixels of S (the
// refill's test, raytrace.wgsl:425-427) -- each is one ray, one miss and one pixel per frame.  With neither map the list is every tile.
void compose_tile_lists(const TileListInput &in, const uint8_t *mask, const uint8_t *empty, TileLists &out)
{
    const int tiles_x = (in.tex_w + 7) / 8, tiles_y = (in.local_rows + 7) / 8;
    const int ntiles = in.tex_w > 0 && in.local_rows > 0 ? tiles_x * tiles_y : 0;
    out.list.assign((size_t)ntiles, 0u);
    size_t at = 0;
    for (int t = 0; t < ntiles; t++)
        if ((!mask || mask[t]) && !(empty && empty[t])) out.list[at++] = (uint32_t)t;
    out.active = (int)at;
    uint64_t pixels = 0;
    for (int t = 0; t < ntiles; t++) {
        if (!((!mask || mask[t]) && empty && empty[t])) continue;
        out.list[at++] = (uint32_t)t;
        const int trow = t / tiles_x, tcol = t - trow * tiles_x;
        int cols = 0;
        for (int px = tcol * 8; px < tcol * 8 + 8; px++) cols += px < in.tex_w && (long long)px < in.res_w ? 1 : 0;
        for (int ply = trow * 8; ply < trow * 8 + 8; ply++) {
            if (ply >= in.local_rows) continue;
            const int pgy = in.nranks <= 1 ? ply : mi3pt_tile_global_row(ply, in.rank, in.nranks, in.block_rows);
            if (pgy >= 0 && pgy < in.tex_h && (long long)pgy < in.res_h) pixels += (uint64_t)cols;
        }
    }
    out.sky = (int)at - out.active;
    out.sky_pixels = pixels;
    out.list.resize(at);
}

}  // namespace pt
