// pt_internal.h -- small helpers shared by the translation units of libmi3pt.so
#pragma once
#include <string>

// Records `msg` as the calling thread's last error and returns `code`.
int pt_set_error(int code, const std::string &msg);
// The calling thread's last error as recorded (what mi3pt_last_error hands out); the string itself lives in pt_context.hip alone.
const std::string &pt_last_error();

// pt_lbvh.hip: device-side linear BVH over n 112-byte triangle records at d_tris; writes (2n - 1)
// 48-byte node records to the HOST buffer nodes_out.  Returns 0, or -1 with `err` set.
#include <hip/hip_runtime.h>
#include <cstdint>
namespace pt {
int lbvh_build(const void *d_tris, size_t n, void *nodes_out, float *build_ms, hipStream_t stream, std::string &err);
// pt_ploc.hip: the same contract for the locally-ordered clustering of include/mi3pt.h (mi3pt_device_build_bvh_ex, method 1); radius 1 .. 64;
// the iteration counts are optional.  Everything it allocates is freed before it returns.
int ploc_build(const void *d_tris, size_t n, int radius, int max_search_iterations, void *nodes_out, float *build_ms,
               uint32_t *search_iterations, uint32_t *forced_iterations, hipStream_t stream, std::string &err);
// pt_refit.hip: the boxes of the n 48-byte node records at d_nodes re-fitted, bottom-up, to the ntris 112-byte triangle records at d_tris
// (both on the device, neither is written); the re-fitted records go to the HOST buffer nodes_out.  The caller vouches for a proper tree
// whose every record the root reaches and whose leaves name triangles below ntris.  Returns 0, or -1 with `err` set.
int refit_bvh(const void *d_tris, size_t ntris, const void *d_nodes, size_t n, void *nodes_out, float *refit_ms, hipStream_t stream, std::string &err);
}

// ---- host-side helpers shared by the context's units (pt_context.hip, pt_ctx_*.hip) and the pt_host_*.cpp files (plain C++: the CPU sanitizer builds cover them)
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>
#include "pt_kernels.h"
#include "../../include/mi3pt.h"
static inline float ldf(const uint8_t *p, size_t off) { float f; std::memcpy(&f, p + off, 4); return f; }
static inline int32_t ldi(const uint8_t *p, size_t off) { int32_t v; std::memcpy(&v, p + off, 4); return v; }
static inline uint32_t ldu(const uint8_t *p, size_t off) { uint32_t v; std::memcpy(&v, p + off, 4); return v; }
// precondition of the exact fast slab test (pt_kernels.hip, RayPre): per box, every coordinate is 0 or within [2^-70, 2^60]
bool node_box_safe(const uint8_t *src, size_t node);
// the compressed packets' outward rounding, decided EXACTLY: is the plane b at least / at most k cells above the grid origin o, i.e.
// b - o >= kc (at_least) or b - o <= kc (!at_least), with kc = k x cell exact in double?  b - o as an error-free pair (TwoSum): the rounded
// difference alone calls a plane 3e-15 cells short of an index line "on" it (a sphere's 1e-17 residue beside an origin at -0.5), and the
// decoded box then misses its whole cell of margin by that much
static inline bool plane_cells_from_origin(float b, float o, double kc, bool at_least)
{
    const double x = (double)b, y = -(double)o;
    const double s = x + y, bb = s - x, e = (x - (s - bb)) + (y - bb);
    if (s != kc) return at_least ? s > kc : s < kc;
    return at_least ? e >= 0.0 : e <= 0.0;
}
// the SAH-optimal grouping of a binary tree's nodes into W-wide packets, and the eight-wide packets of kernel variant 14 (pt_host_wide.cpp)
struct WideCollapse {
    int W = 4;
    std::vector<uint8_t> k0;         // per node: how many of its packet's W entries go to the left child's side
    std::vector<uint8_t> split;      // [node][i], i = 2 .. W-1: entries for the left side when the node is opened into i entries; 0 = "as with i - 1"
    const uint8_t *src = nullptr;
    bool leaf(size_t i) const { return ldi(src + i * MI3PT_BVHNODE_STRIDE, 28) == 1; }
    int32_t left(size_t i) const { return ldi(src + i * MI3PT_BVHNODE_STRIDE, 32); }
    int32_t right(size_t i) const { return ldi(src + i * MI3PT_BVHNODE_STRIDE, 36); }
    // the entries of node x's packet (binary node indices)
    void children_of(size_t x, std::vector<int32_t> &out) const
    {
        out.clear();
        std::vector<std::pair<int32_t, int>> work;      // (node, entries it may use)
        work.emplace_back(right(x), W - (int)k0[x]);
        work.emplace_back(left(x), (int)k0[x]);
        while (!work.empty()) {
            auto [c, i] = work.back();
            work.pop_back();
            if (leaf((size_t)c) || i <= 1) { out.push_back(c); continue; }
            int k = 0;
            while (i >= 2 && (k = split[(size_t)c * (size_t)W + (size_t)i]) == 0) i--;
            if (i < 2) { out.push_back(c); continue; }
            work.emplace_back(right((size_t)c), i - k);
            work.emplace_back(left((size_t)c), k);
        }
    }
};
bool collapse_optimal(const uint8_t *src, size_t n, int W, const std::vector<uint8_t> *closed, WideCollapse &out);
struct Cw8Build {
    std::vector<pt::CW8Packet> packets;
    std::vector<pt::TriPacket64> records;
    int height = 0;             // levels of packets: the walk's node stack never holds more entries (one per level)
    double mean_children = 0.0;
};
bool build_cw8(const uint8_t *src, size_t n, const float *verts /* 12 floats per triangle: a, pad, b, pad, c, pad */, size_t nt,
               const std::vector<float> &wmax, Cw8Build &out, bool greedy = false);
// pt_host_compile.cpp: the scene compile -- what mi3pt_upload_bvh, mi3pt_upload_triangles and the context's lazy analysis (prepare_cull)
// hand to the device, computed from the uploaded records alone
#include <functional>
namespace pt {
// child reference of the packet walk: leaf -> 0x80000000 | triangle (renumbered by tri_new when given), else packet_of[]
uint32_t child_ref(const uint8_t *src, const std::vector<uint32_t> &packet_of, const uint32_t *tri_new, int32_t child);
// one 64-byte packet per internal node, at the index packet_of[] gives it: bit copies of both children's boxes, their references, the
// guard bits of the fast slab test
void build_packets(const uint8_t *src, size_t n, const std::vector<uint32_t> &packet_of, size_t npackets, const uint32_t *tri_new,
                   std::vector<NodePacket> &pk);
struct TreeCompile {
    std::vector<uint32_t> packet_of;        // per node: its packet (internal nodes in index order), REF_NONE for a leaf
    size_t npackets = 0;
    std::vector<NodePacket> packets;
    std::vector<uint32_t> leaf_rank;        // per triangle: its leaf's place in the reference's visiting order
    int leaf_cap = 0, walk_stack_worst = 64;
    bool tree_proper = false, cull_stack_ok = false;
    uint32_t root_ref = REF_NONE, scene_flags = 0;
    int64_t max_tri_ref = -1;
    size_t reached = 0;                     // records the walk from the root visited (== the record count: no record is out of its reach)
};
// nullptr, or why the tree is refused (MI3PT_ERR_INVALID)
const char *compile_tree(const uint8_t *src, size_t n, TreeCompile &out);
// the 48-byte intersection record of a 112-byte triangle record: a, the material index, and the edges b - a, c - a -- the two subtractions
// Moller-Trumbore starts with (raytrace.wgsl:82-83), each ONE fp32 rounding (round-to-nearest-even, subnormals kept, like the device's
// v_sub_f32), so the kernels start from the same operands
TriPacket tri_packet_of(const uint8_t *rec);
const char *compile_triangles(const uint8_t *src, size_t n, std::vector<TriPacket> &pk, int64_t &max_mat_ref);
// the three vertices of a triangle: the first 48 of a record's 112 bytes (raytrace.wgsl:40-49)
struct TriVerts { float a[3], pa, b[3], pb, c[3], pc; };
static_assert(sizeof(TriVerts) == 48, "three vec3f + padding");
std::vector<TriVerts> triangle_verts(const uint8_t *triangles, size_t nt);
struct WalkOptions {
    int collapse = -1, packet_order = 0;        // MI3PT_OPT_COLLAPSE, MI3PT_OPT_PACKET_ORDER
    bool eight_wide = false;                    // build kernel variant 14's packets too
    bool eight_wide_any_height = false;         // ... and emit them even when the walk's stack cannot hold their levels (the host-side self-check)
    double cull_scale = 1.0;                    // < 1 VOIDS the proof of DESIGN.md 3a (experiment build only)
};
struct WalkCompile {
    bool analysed = false;                      // false: a leaf names a triangle that was not uploaded -- nothing was emitted
    float cull_ka = 0.0f, cull_kb = 0.0f;
    bool wide_ok = false, cwide_ok = false, cw8_ok = false, wide_root_nested = false;
    size_t nwide = 0, ncw8 = 0, cw8_records = 0;
    int wide_stack_worst = 0, cw8_height = 0, auto_wide_variant = 10;
    double cw8_mean_children = 0.0;
};
// the buffers of compile_walk, in the order they are emitted: uint32 cull words per node packet, WidePacket, CWidePacket, TriPacket64 per
// triangle, CW8Packet, TriPacket64 per 8-wide record
enum WalkBuffer { WALK_CULL, WALK_WIDE, WALK_CWIDE, WALK_TRI64, WALK_CW8, WALK_TRI8 };
// called with each buffer as it becomes ready (valid during the call only: it is freed before the next stage); non-zero stops the compile
using WalkSink = std::function<int(WalkBuffer kind, const void *data, size_t bytes)>;
// 0, the sink's status, or MI3PT_ERR_STATE when npackets is not the tree's
int compile_walk(const uint8_t *src, size_t n, const TriVerts *tris, size_t nt, size_t npackets, const WalkOptions &opt, const WalkSink &emit,
                 WalkCompile &out);
}
// pt_host_sky.cpp: the tiles whose camera rays can reach no geometry (PROOFS.md section 5).  sky_cut_of: a cut of the tree as boxes (6 floats
// each), false if a node's box does not contain its children's; sky_classify: empty[tile] = 1 per 8x8 tile of this rank's image, returns the count
namespace pt {
bool sky_cut_of(const uint8_t *src, size_t n, std::vector<float> &boxes);
size_t sky_classify(const std::vector<float> &boxes, bool have_cut, const uint8_t *u, int width, int local_rows, int height,
                    int rank, int nranks, int block_rows, std::vector<uint8_t> &empty);
}
// pt_host_adapt.cpp: a launch's tile lists from the sample mask (mi3pt_set_sample_mask; null: every tile) and the view's empty tiles
// (sky_classify's map; null: none) -- list = [A: sampled, not empty | S: sampled, empty], both ascending; active = |A|, sky = |S|,
// sky_pixels = the in-bounds pixels of S for the raytrace uniforms' resolution res_w x res_h
namespace pt {
struct TileListInput { int tex_w, tex_h, local_rows, rank, nranks, block_rows; long long res_w, res_h; };
struct TileLists { std::vector<uint32_t> list; int active = 0, sky = 0; uint64_t sky_pixels = 0; };
void compose_tile_lists(const TileListInput &in, const uint8_t *mask, const uint8_t *empty, TileLists &out);
}
