// pt_host_sky.cpp -- which 8x8 tiles of an image hold only camera rays that can reach no geometry ("empty tiles", PROOFS.md section 5).
//
// The persistent raytrace kernel's worst customer is a sample whose camera ray misses the scene: one ray, one miss, one
// environment lookup, served at half a wave's width.  For a pinhole camera the set of such pixels depends on camera, image size,
// tile split and tree only -- not on the frame -- so it is found here, on the host, once per camera and scene, and the launch
// hands those tiles to a plain streaming kernel (pt_kernels.hip: k_sky_samples) instead of to the state machine.
//
//   sky_cut_of      a CUT of the uploaded tree: a few dozen nodes that together cover every leaf.  A ray that fails the
//                   reference's slab test on a node's box fails it on every box nested in that box, so a ray that fails every
//                   box of the cut reaches no leaf and the reference returns a miss.  Needs every node's box to contain its
//                   children's: checked here for the whole tree; a tree that fails has no cut and therefore no empty tiles.
//   sky_classify    per tile: an enclosure of the directions of all its camera rays (every pixel, every frame's jitter) in the
//                   camera's plane coordinates, against the projected, grown boxes of the cut.  Double precision, interval
//                   bounds, margins orders above the fp32 rounding of the kernel's ray formula.
//
// Everything here is conservative: a tile is called empty only if NO ray of it can pass the fp32 slab test of ANY cut box.
#include "../../include/mi3pt.h"
#include "pt_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <queue>

namespace pt {

static bool finite3(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

static void node_box(const uint8_t *src, size_t i, double *mn, double *mx)
{
    const uint8_t *r = src + i * MI3PT_BVHNODE_STRIDE;
    for (int k = 0; k < 3; k++) { mn[k] = (double)ldf(r, 4 * (size_t)k); mx[k] = (double)ldf(r, 16 + 4 * (size_t)k); }
}

// `boxes`: 6 floats per cut node (min xyz, max xyz), bit copies of the uploaded records.  false (and no boxes): the tree has a
// node whose box does not contain a child's, a box that is not finite or ordered, or a child index outside the buffer.
bool sky_cut_of(const uint8_t *src, size_t n, std::vector<float> &boxes)
{
    boxes.clear();
    if (!src || n == 0) return false;
    auto is_leaf = [&](size_t i) { return ldi(src + i * MI3PT_BVHNODE_STRIDE, 28) == 1; };
    for (size_t i = 0; i < n; i++) {
        double mn[3], mx[3];
        node_box(src, i, mn, mx);
        if (!finite3(mn) || !finite3(mx) || mn[0] > mx[0] || mn[1] > mx[1] || mn[2] > mx[2]) return false;
        if (is_leaf(i)) continue;
        for (size_t off : { (size_t)32, (size_t)36 }) {
            const int32_t c = ldi(src + i * MI3PT_BVHNODE_STRIDE, off);
            if (c < 0) continue;                        // (an absent child: nothing below it)
            if ((size_t)c >= n || (size_t)c <= i) return false;
            double cmn[3], cmx[3];
            node_box(src, (size_t)c, cmn, cmx);
            for (int k = 0; k < 3; k++)
                if (!(cmn[k] >= mn[k] && cmx[k] <= mx[k])) return false;
        }
    }
    // expand from the root, largest surface area first, up to SKY_CUT_NODES entries; a leaf stays
    constexpr size_t SKY_CUT_NODES = 48;
    auto area = [&](size_t i) {
        double mn[3], mx[3];
        node_box(src, i, mn, mx);
        const double ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
        return ex * ey + ey * ez + ez * ex;
    };
    std::priority_queue<std::pair<double, size_t>> open;      // internal nodes of the cut
    std::vector<size_t> cut;                                  // its leaves
    if (is_leaf(0)) cut.push_back(0); else open.emplace(area(0), 0);
    while (!open.empty() && cut.size() + open.size() < SKY_CUT_NODES) {
        const size_t i = open.top().second;
        open.pop();
        for (size_t off : { (size_t)32, (size_t)36 }) {
            const int32_t c = ldi(src + i * MI3PT_BVHNODE_STRIDE, off);
            if (c < 0) continue;
            if (is_leaf((size_t)c)) cut.push_back((size_t)c); else open.emplace(area((size_t)c), (size_t)c);
        }
    }
    for (; !open.empty(); open.pop()) cut.push_back(open.top().second);
    for (size_t i : cut) {
        const uint8_t *r = src + i * MI3PT_BVHNODE_STRIDE;
        for (size_t off : { (size_t)0, (size_t)4, (size_t)8, (size_t)16, (size_t)20, (size_t)24 }) boxes.push_back(ldf(r, off));
    }
    return true;      // (a tree without a reachable leaf has an empty cut: every ray misses)
}

static int global_row(int ly, int rank, int nranks, int block_rows)
{
    return nranks <= 1 ? ly : mi3pt_tile_global_row(ly, rank, nranks, block_rows);
}

// empty[tile] = 1 for the empty tiles of this rank's image (tiles_x x tiles_y, row-major over LOCAL rows: the kernels' tile
// numbering); returns how many.  `u` = the 96-byte raytrace uniform block.  All zero unless the launch is one the split is
// proven for: pinhole (aperture 0, no -0 camera coordinate), one sample per frame, at least one bounce, sane camera numbers.
size_t sky_classify(const std::vector<float> &boxes, bool have_cut, const uint8_t *u, int width, int local_rows, int height,
                    int rank, int nranks, int block_rows, std::vector<uint8_t> &empty)
{
    const int tiles_x = (width + 7) / 8, tiles_y = (local_rows + 7) / 8;
    empty.assign((size_t)tiles_x * (size_t)(tiles_y > 0 ? tiles_y : 0), 0);
    if (!have_cut || empty.empty()) return 0;
    const double res_x = ldf(u, 0), res_y = ldf(u, 4), aspect = ldf(u, 8);
    const int32_t max_bounces = ldi(u, 16), spf = ldi(u, 20);
    const double fov = ldf(u, 60), F = ldf(u, 64);
    const float aperture = ldf(u, 68);
    double o[3], cd[3];
    for (int k = 0; k < 3; k++) {
        if (ldu(u, 32 + 4 * (size_t)k) == 0x80000000u) return 0;      // a -0 camera coordinate: the kernel's thin-lens branch runs
        o[k] = ldf(u, 32 + 4 * (size_t)k);
        cd[k] = ldf(u, 48 + 4 * (size_t)k);
    }
    if (!(aperture == 0.0f) || spf != 1 || max_bounces < 1) return 0;
    if (!finite3(o) || !finite3(cd) || !(res_x >= 1.0 && res_x <= 65536.0) || !(res_y >= 1.0 && res_y <= 65536.0) ||
        !(aspect >= 1e-3 && aspect <= 1e3) || !(fov >= 1.0 && fov <= 150.0) || !(F >= 1e-4 && F <= 1e6) ||
        !(std::fabs(o[0]) + std::fabs(o[1]) + std::fabs(o[2]) <= 1e6))
        return 0;
    // the camera's frame (pt_kernels.hip: camera_frame), in double
    const double len = std::sqrt(cd[0] * cd[0] + cd[1] * cd[1] + cd[2] * cd[2]);
    if (!(len >= 1e-12 && len <= 1e12)) return 0;
    const double w[3] = { -cd[0] / len, -cd[1] / len, -cd[2] / len };
    // (camera_frame switches its `up` vector where |w.y| > 0.99999, and u_dir = normalize(up x w) loses digits as that is approached:
    // views that steep get no split)
    if (std::fabs(w[1]) > 0.999) return 0;
    const double up[3] = { 0.0, 1.0, 0.0 };
    double ud[3] = { up[1] * w[2] - up[2] * w[1], up[2] * w[0] - up[0] * w[2], up[0] * w[1] - up[1] * w[0] };
    const double ul = std::sqrt(ud[0] * ud[0] + ud[1] * ud[1] + ud[2] * ud[2]);
    if (!(ul >= 1e-6)) return 0;
    for (double &x : ud) x /= ul;
    const double vd[3] = { w[1] * ud[2] - w[2] * ud[1], w[2] * ud[0] - w[0] * ud[2], w[0] * ud[1] - w[1] * ud[0] };
    const double t = std::tan(fov * 3.14159265358979323846 / 180.0 / 2.0), r = aspect * t;

    // the cut's boxes, grown, as rectangles in plane coordinates (q.u_dir / -q.w, q.v_dir / -q.w), q = corner - camera
    constexpr double GROW = 1e-4, MARGIN = 1e-4;
    struct Rect { double a0, a1, b0, b1; };
    std::vector<Rect> rects;
    for (size_t k = 0; k + 6 <= boxes.size(); k += 6) {
        double reach = 0.0;
        for (int i = 0; i < 3; i++)
            reach = std::max(reach, std::max(std::fabs((double)boxes[k + i] - o[i]), std::fabs((double)boxes[k + 3 + i] - o[i])));
        const double grow = GROW * reach + 1e-30;
        Rect rc = { INFINITY, -INFINITY, INFINITY, -INFINITY };
        for (int c = 0; c < 8; c++) {
            double q[3];
            for (int i = 0; i < 3; i++) q[i] = ((c >> i) & 1 ? (double)boxes[k + 3 + i] + grow : (double)boxes[k + i] - grow) - o[i];
            const double depth = -(q[0] * w[0] + q[1] * w[1] + q[2] * w[2]);
            const double ql = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
            if (!(depth > 1e-3 * ql)) return 0;        // a corner not in front of the camera: the box may cover any direction
            const double a = (q[0] * ud[0] + q[1] * ud[1] + q[2] * ud[2]) / depth, b = (q[0] * vd[0] + q[1] * vd[1] + q[2] * vd[2]) / depth;
            rc.a0 = std::min(rc.a0, a); rc.a1 = std::max(rc.a1, a);
            rc.b0 = std::min(rc.b0, b); rc.b1 = std::max(rc.b1, b);
        }
        const double ma = MARGIN * (1.0 + std::max(std::fabs(rc.a0), std::fabs(rc.a1))), mb = MARGIN * (1.0 + std::max(std::fabs(rc.b0), std::fabs(rc.b1)));
        rc.a0 -= ma; rc.a1 += ma; rc.b0 -= mb; rc.b1 += mb;
        rects.push_back(rc);
    }

    // what the jitter -- a point of the unit disk scaled to (1 / res_x, 1 / res_y, 0), added in WORLD x, y -- can add along the frame's axes
    const double ju = (std::fabs(ud[0]) / res_x + std::fabs(ud[1]) / res_y) * (1.0 + 1e-6);
    const double jv = (std::fabs(vd[0]) / res_x + std::fabs(vd[1]) / res_y) * (1.0 + 1e-6);
    const double jw = (std::fabs(w[0]) / res_x + std::fabs(w[1]) / res_y) * (1.0 + 1e-6);
    const double cam1 = std::fabs(o[0]) + std::fabs(o[1]) + std::fabs(o[2]);
    auto sq_max = [](double lo, double hi) { return std::max(lo * lo, hi * hi); };
    size_t count = 0;
    for (int ty = 0; ty < tiles_y; ty++) {
        // the tile's rows of the image: a tile split may deal its eight local rows to rows far apart
        int g0 = INT32_MAX, g1 = INT32_MIN;
        for (int ly = ty * 8; ly < std::min(ty * 8 + 8, local_rows); ly++) {
            const int g = global_row(ly, rank, nranks, block_rows);
            if (g >= height) continue;
            g0 = std::min(g0, g); g1 = std::max(g1, g);
        }
        if (g0 > g1) continue;          // (no row of the image: nothing is rendered here, the tile stays with the persistent kernel)
        const double v0 = -t + 2.0 * t * ((double)(g0 - 1) / res_y), v1 = -t + 2.0 * t * ((double)(g1 + 1) / res_y);
        for (int tx = 0; tx < tiles_x; tx++) {
            const int p0 = tx * 8, p1 = std::min(tx * 8 + 7, width - 1);
            const double u0 = -r + 2.0 * r * ((double)(p0 - 1) / res_x), u1 = -r + 2.0 * r * ((double)(p1 + 1) / res_x);
            // direction = A + g J up to scale: A = u u_dir + v v_dir - aspect w, |A| = n, g = n / focalDistance, J the jitter
            const double nmax = std::sqrt(sq_max(u0, u1) + sq_max(v0, v1) + aspect * aspect);
            const double gmax = nmax / F;
            const double err = gmax * 1e-6 * (cam1 + F + 1.0);      // fp32 rounding of cam_pos + dir0 * focalDistance, + jitter, - cam_pos
            const double a0 = u0 - gmax * ju - err, a1 = u1 + gmax * ju + err;
            const double b0 = v0 - gmax * jv - err, b1 = v1 + gmax * jv + err;
            const double c0 = aspect - gmax * jw - err, c1 = aspect + gmax * jw + err;
            if (!(c0 > 0.05 * aspect)) continue;         // (a focal distance so short that the jitter turns rays sideways)
            double pa0 = std::min(a0 / c0, a0 / c1), pa1 = std::max(a1 / c0, a1 / c1);
            double pb0 = std::min(b0 / c0, b0 / c1), pb1 = std::max(b1 / c0, b1 / c1);
            const double ma = MARGIN * (1.0 + std::max(std::fabs(pa0), std::fabs(pa1))), mb = MARGIN * (1.0 + std::max(std::fabs(pb0), std::fabs(pb1)));
            pa0 -= ma; pa1 += ma; pb0 -= mb; pb1 += mb;
            bool hit = false;
            for (const Rect &rc : rects)
                if (pa0 <= rc.a1 && pa1 >= rc.a0 && pb0 <= rc.b1 && pb1 >= rc.b0) { hit = true; break; }
            if (!hit) { empty[(size_t)ty * tiles_x + tx] = 1; count++; }
        }
    }
    return count;
}

}  // namespace pt

extern "C" int mi3pt_host_sky_tiles(const void *nodes, size_t nodes_bytes, const void *raytrace_uniforms, int width, int height,
                                    int rank, int nranks, int block_rows, uint8_t *empty_out, size_t capacity, size_t *ntiles_out)
{
    if (!nodes || !raytrace_uniforms || nodes_bytes == 0 || nodes_bytes % MI3PT_BVHNODE_STRIDE)
        return pt_set_error(MI3PT_ERR_INVALID, "sky tiles: BVH bytes must be a non-zero multiple of 48");
    if (width <= 0 || height <= 0 || width > 32768 || height > 32768 || nranks < 1 || rank < 0 || rank >= nranks || block_rows < 1)
        return pt_set_error(MI3PT_ERR_INVALID, "sky tiles: bad image size or tile split");
    const int local_rows = mi3pt_tile_local_rows(height, rank, nranks, block_rows);
    const size_t ntiles = (size_t)((width + 7) / 8) * (size_t)((local_rows + 7) / 8);
    if (ntiles_out) *ntiles_out = ntiles;
    if (!empty_out) return MI3PT_OK;
    if (capacity < ntiles) return pt_set_error(MI3PT_ERR_INVALID, "sky tiles: output too small");
    std::vector<float> boxes;
    const bool have = pt::sky_cut_of(static_cast<const uint8_t *>(nodes), nodes_bytes / MI3PT_BVHNODE_STRIDE, boxes);
    std::vector<uint8_t> empty;
    pt::sky_classify(boxes, have, static_cast<const uint8_t *>(raytrace_uniforms), width, local_rows, height, rank, nranks, block_rows, empty);
    std::memcpy(empty_out, empty.data(), ntiles);
    return MI3PT_OK;
}
