// pt_host_compile.cpp -- the scene compile: everything the walks' device buffers hold, computed from the uploaded records (plain C++, no
// device calls, no context: the CPU tests and the sanitizer builds of tests/tools/sanitize_cpu.sh run it as it ships)
//   compile_tree               packet numbering, node packets, leaf ranks, the stack bounds of the binary walks   (mi3pt_upload_bvh)
//   compile_triangles          the 48-byte intersection records                                                    (mi3pt_upload_triangles)
//   compile_walk               culling weights, 4-ary packets (exact + compressed), 64-byte records, 8-wide packets, what `auto` means
//                              (the context's lazy analysis, prepare_cull); buffers leave through a sink as each becomes ready
//   mi3pt_host_scene_compile   all three with a hashing sink
//   mi3pt_host_walk_buffer     the tree and walk compiles with a sink that copies ONE of the walk's buffers out (what the CPU tests decode)
#include "../../include/mi3pt.h"
#include "pt_internal.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>

namespace pt {

namespace {

inline const uint8_t *rec_of(const uint8_t *src, size_t node) { return src + node * MI3PT_BVHNODE_STRIDE; }
inline bool is_leaf(const uint8_t *src, size_t node) { return ldi(rec_of(src, node), 28) == 1; }

// a node's box: bit copies of the record's coordinates
struct Box { float mn[3], mx[3]; };
inline Box box_of(const uint8_t *src, size_t node)
{
    Box b;
    std::memcpy(b.mn, rec_of(src, node), 12);
    std::memcpy(b.mx, rec_of(src, node) + 16, 12);
    return b;
}
inline void put_box(float *mn, float *mx, const Box &b) { std::memcpy(mn, b.mn, 12); std::memcpy(mx, b.mx, 12); }
inline bool contains(const Box &outer, const Box &in)
{
    for (int k = 0; k < 3; k++)
        if (!(outer.mn[k] <= in.mn[k] && outer.mx[k] >= in.mx[k])) return false;     // false for NaNs too
    return true;
}
inline double half_area(const Box &b)
{
    const double x = (double)b.mx[0] - b.mn[0], y = (double)b.mx[1] - b.mn[1], z = (double)b.mx[2] - b.mn[2];
    return x * y + x * z + y * z;
}

// Worst-case node-stack occupancy of a near-first walk from node 0, whatever the order its children are pushed in (every box hit, nothing
// skipped): the culling walks push the nearer child last, so ANY child may be the one that is descended first with all its internal siblings
// still stacked: occupancy(child) = occupancy(parent) - 1 + (internal children of the parent).  Internal entries only.
template <class InternalChildren>      // int internal_children(uint32_t node, uint32_t out[4])
size_t worst_stack_any_order(InternalChildren internal_children)
{
    size_t worst = 1;
    std::vector<std::pair<uint32_t, uint32_t>> work;      // (node, occupancy with it on top)
    work.emplace_back(0u, 1u);
    while (!work.empty()) {
        const auto [node, occ] = work.back();
        work.pop_back();
        uint32_t ks[4];
        const uint32_t m = (uint32_t)internal_children(node, ks);
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t oc = occ - 1u + m;
            if (oc > worst) worst = oc;
            work.emplace_back(ks[i], oc);
        }
    }
    return worst;
}

// a culling weight as the top half of a binary32 value, rounded up; 0x7f80 = +infinity = never skip
inline uint32_t round_up_16(float f)
{
    uint32_t b;
    std::memcpy(&b, &f, 4);
    if (!(f == f) || (b & 0x7f800000u) == 0x7f800000u || (b >> 31)) return 0x7f80u;   // NaN / inf / negative: never skip
    const uint32_t r = (b + 0xffffu) >> 16;
    return r > 0x7f80u ? 0x7f80u : r;
}

}  // namespace

uint32_t child_ref(const uint8_t *src, const std::vector<uint32_t> &packet_of, const uint32_t *tri_new, int32_t child)
{
    if (child < 0) return REF_NONE;
    if (is_leaf(src, (size_t)child)) {
        const uint32_t ti = (uint32_t)ldi(rec_of(src, (size_t)child), 40);
        return 0x80000000u | (tri_new ? tri_new[ti] : ti);
    }
    return packet_of[(size_t)child];
}

void build_packets(const uint8_t *src, size_t n, const std::vector<uint32_t> &packet_of, size_t npackets, const uint32_t *tri_new,
                   std::vector<NodePacket> &pk)
{
    pk.assign(npackets ? npackets : 1, NodePacket());
    std::memset(pk.data(), 0, pk.size() * sizeof(NodePacket));
    for (auto &p : pk) p.cull = 0x7f807f80u;        // never skip, until the cull analysis has run
    for (size_t i = 0; i < n; i++) {
        if (packet_of[i] == REF_NONE) continue;
        NodePacket &p = pk[packet_of[i]];
        const int32_t left = ldi(rec_of(src, i), 32), right = ldi(rec_of(src, i), 36);
        if (left >= 0) put_box(p.lmin, p.lmax, box_of(src, (size_t)left));
        if (right >= 0) put_box(p.rmin, p.rmax, box_of(src, (size_t)right));
        p.lref = child_ref(src, packet_of, tri_new, left);
        p.rref = child_ref(src, packet_of, tri_new, right);
        p.flags = ((left >= 0 && !node_box_safe(src, (size_t)left)) ? 1u : 0u) | ((right >= 0 && !node_box_safe(src, (size_t)right)) ? 2u : 0u) |
                  ((left < 0 || right < 0) ? 4u : 0u);      // bit2: a child is missing (never from flattenBVH)
    }
}

const char *compile_tree(const uint8_t *src, size_t n, TreeCompile &out)
{
    // Validate and number the internal nodes.  A child must come after its parent
    // (true of flattenBVH's breadth-first order, raytrace.ts:667-678); that bounds the
    // walk, so a malformed tree cannot hang the device.
    out.packet_of.assign(n, REF_NONE);
    out.npackets = 0;
    out.max_tri_ref = -1;
    for (size_t i = 0; i < n; i++) {
        const uint8_t *r = rec_of(src, i);
        if (ldi(r, 28) == 1) {
            const int32_t ti = ldi(r, 40);
            if (ti < 0) return "leaf node with negative triangleIndex";
            if (ti > out.max_tri_ref) out.max_tri_ref = ti;
        } else {
            for (size_t off : { (size_t)32, (size_t)36 }) {
                const int32_t c = ldi(r, off);
                if (c >= 0 && ((size_t)c >= n || (size_t)c <= i))
                    return "BVH child index must be greater than its parent's and inside the buffer "
                           "(breadth-first order, raytrace.ts:667-694)";
            }
            out.packet_of[i] = (uint32_t)out.npackets++;
        }
    }
    build_packets(src, n, out.packet_of, out.npackets, nullptr, out.packets);
    // Order analysis for the deferred-leaf kernel (pt_kernels.hip, DEFER): the reference walk
    // visits leaves in a fixed order (node, right subtree, left subtree: left is pushed first,
    // raytrace.wgsl:184-198) and keeps the FIRST of equal-t hits.  If the buffer is a proper
    // tree (every node reached exactly once, every triangle owned by at most one leaf, no
    // missing child) that order is a per-triangle rank, and testing leaves in any order and
    // resolving ties by rank gives the same hit -- provided the 64-entry abort cannot fire,
    // i.e. the walk's worst-case stack occupancy (every box hit) stays below 64.
    out.leaf_rank.assign((size_t)(out.max_tri_ref + 1 > 0 ? out.max_tri_ref + 1 : 1), 0xffffffffu);
    std::vector<uint32_t> st;
    std::vector<uint8_t> seen(n, 0);
    st.push_back(0);
    size_t worst = 0, worst_internal = 0, internal = is_leaf(src, 0) ? 0 : 1;     // stack occupancy: all entries / internal nodes only
    uint32_t rank = 0;
    bool proper = true;
    while (!st.empty() && proper) {      // (nodes the root does not reach are never walked by the reference either)
        if (st.size() > worst) worst = st.size();
        if (internal > worst_internal) worst_internal = internal;
        const uint32_t node = st.back();
        st.pop_back();
        if (seen[node]) { proper = false; break; }
        seen[node] = 1;
        const uint8_t *r = rec_of(src, node);
        if (ldi(r, 28) == 1) {
            const int32_t ti = ldi(r, 40);
            if (out.leaf_rank[(size_t)ti] != 0xffffffffu) { proper = false; break; }
            out.leaf_rank[(size_t)ti] = rank++;
        } else {
            internal--;
            const int32_t left = ldi(r, 32), right = ldi(r, 36);
            if (left < 0 || right < 0) { proper = false; break; }
            st.push_back((uint32_t)left);
            st.push_back((uint32_t)right);
            internal += (is_leaf(src, (size_t)left) ? 0 : 1) + (is_leaf(src, (size_t)right) ? 0 : 1);
        }
    }
    // The 64-entry abort (raytrace.wgsl:167-171) counts leaves too: it cannot fire while the
    // worst case stays below 64.  LDS holds SM_LDS_DEPTH (24) entries per lane: the node stack (internal
    // nodes only in the deferred walk) from the bottom, parked leaves from the top.
    out.tree_proper = proper && worst < 64;
    out.reached = 0;
    for (size_t i = 0; i < n; i++) out.reached += seen[i];
    out.leaf_cap = out.tree_proper && (int)worst_internal <= SM_LDS_DEPTH - 4 ? SM_LDS_DEPTH - (int)worst_internal : 0;
    out.walk_stack_worst = out.tree_proper ? (int)worst : 64;      // (every box hit: the real walk's stack is a subset of this one's at every node it visits)
    // the culling walks' node stack has to fit the LDS slots plus the overflow slice (pt_kernels.h SM_CULL_STACK_MAX)
    out.cull_stack_ok = out.tree_proper && !is_leaf(src, 0) &&
        worst_stack_any_order([&](uint32_t node, uint32_t *ks) {
            int m = 0;
            for (size_t off : { (size_t)32, (size_t)36 }) {
                const uint32_t c = (uint32_t)ldi(rec_of(src, node), off);
                if (!is_leaf(src, c)) ks[m++] = c;
            }
            return m;
        }) <= (size_t)SM_CULL_STACK_MAX;
    out.root_ref = child_ref(src, out.packet_of, nullptr, 0);
    out.scene_flags = node_box_safe(src, 0) ? 1u : 0u;
    return nullptr;
}

TriPacket tri_packet_of(const uint8_t *rec)
{
    TriPacket p;
    for (int k = 0; k < 3; k++) {
        const float a = ldf(rec, 4 * (size_t)k), b = ldf(rec, 16 + 4 * (size_t)k), c = ldf(rec, 32 + 4 * (size_t)k);
        volatile float e1 = b - a, e2 = c - a;      // (volatile: each difference is rounded to binary32 here, whatever the host's evaluation method)
        p.a[k] = a; p.e1[k] = e1; p.e2[k] = e2;
    }
    p.material = (uint32_t)ldi(rec, 92);
    p.pad0 = p.pad1 = 0;
    return p;
}

const char *compile_triangles(const uint8_t *src, size_t n, std::vector<TriPacket> &pk, int64_t &max_mat_ref)
{
    pk.resize(n);
    max_mat_ref = -1;
    for (size_t i = 0; i < n; i++) {
        const uint8_t *t = src + i * MI3PT_TRIANGLE_STRIDE;
        const int32_t mi = ldi(t, 92);
        if (mi < 0) return "triangle with negative materialIndex";
        pk[i] = tri_packet_of(t);
        if (mi > max_mat_ref) max_mat_ref = mi;
    }
    return nullptr;
}

std::vector<TriVerts> triangle_verts(const uint8_t *src, size_t nt)
{
    std::vector<TriVerts> v(nt);
    for (size_t t = 0; t < nt; t++) std::memcpy(&v[t], src + t * MI3PT_TRIANGLE_STRIDE, sizeof(TriVerts));
    return v;
}

// Analysis for the distance-culling walk (kernel variant 9; pt_kernels.hip k_raytrace_sm<.., CULL>,
// proof in DESIGN.md section 3a).  The rounding error of the reference's Moller-Trumbore code
// scales with E = |e1| * |e2| of the triangle (through kappa = E |d| / |det| <= 2 E / EPSILON for
// |d| <= 2): a triangle it accepts with t <= tau lies within
//     delta = W(E) * (u / EPSILON) * (tau |d|^2 + 1.65 L |d|),   W(E) = E * c1(E),  u = 2^-24,
// of the point o + t d, with c1(E) = (11.7 b + 3.04) / (1 - (11.7 b + 1.02) u kappa),
// b = (1 + A) / (1 - A) + 1, A = 5.85 u kappa (c1 = 26.4 for small triangles, growing with E),
// and L = |e1| + |e2|.  Per child of every internal node this bounds W over the triangles below
// that child and writes the two bounds, rounded up to 16 bits each, into the node packet.  A
// child gets +infinity (never skipped) when something below it is outside the analysis: a
// triangle too large for it (A >= 1/4 or the denominator below 1/2: E above ~0.17), one with
// |e1| + |e2| above 16 x the scene's mean (it would loosen the L term for every other one), a
// non-finite coordinate, or a box that does not contain what is below it (the walk bounds
// distances by boxes; the reference does not care whether its boxes bound anything).
// The tree must have passed compile_tree (children after their parent, inside the buffer).
int compile_walk(const uint8_t *src, size_t n, const TriVerts *tris, size_t nt, size_t npackets, const WalkOptions &opt,
                 const WalkSink &emit, WalkCompile &out)
{
    out = WalkCompile();
    // per triangle: E and L in double from the fp32 vertices
    auto tri_el = [&](size_t ti, double &E, double &Lsum) {
        const TriVerts &t = tris[ti];
        double e1 = 0, e2 = 0;
        for (int k = 0; k < 3; k++) {
            const double u = (double)t.b[k] - (double)t.a[k], v = (double)t.c[k] - (double)t.a[k];
            e1 += u * u; e2 += v * v;
        }
        e1 = std::sqrt(e1); e2 = std::sqrt(e2);
        E = e1 * e2; Lsum = e1 + e2;
    };
    // The nodes the root reaches (children come after their parent: one forward pass).  No walk visits any other node, so no other node
    // enters the statistics, denies the compressed packets or writes a triangle's record -- a buffer may carry records nobody walks,
    // with any box and any (uploaded) triangle.  What the UPLOAD checks it checks on every record, and so does the line below.
    std::vector<uint8_t> reached(n, 0);
    reached[0] = 1;
    for (size_t i = 0; i < n; i++) {
        if (!reached[i] || is_leaf(src, i)) continue;
        for (int32_t c : { ldi(rec_of(src, i), 32), ldi(rec_of(src, i), 36) })
            if (c >= 0 && (size_t)c < n) reached[(size_t)c] = 1;
    }
    double mean_l = 0.0;
    size_t counted = 0;
    for (size_t i = 0; i < n; i++) {
        if (!is_leaf(src, i)) continue;
        const int32_t ti = ldi(rec_of(src, i), 40);
        if (ti < 0 || (size_t)ti >= nt) return MI3PT_OK;      // (the context's check_scene reports it, reachable or not; no analysis)
        if (!reached[i]) continue;
        double E, Ls;
        tri_el((size_t)ti, E, Ls);
        if (Ls == Ls && Ls < 1e30) { mean_l += Ls; counted++; }
    }
    mean_l = counted ? mean_l / (double)counted : 0.0;
    const double lcap = 16.0 * mean_l;
    const double u = std::ldexp(1.0, -24), inv_eps = 1.0 / (double)1e-6f;
    // W(E) = E * c1(E); < 0: the triangle is outside the analysis
    auto weight = [&](double E) -> double {
        const double kappa = E * 2.0 * inv_eps;
        const double A = 5.85 * u * kappa;
        if (!(A < 0.25)) return -1.0;
        const double b = (1.0 + A) / (1.0 - A) + 1.0;
        const double den = 1.0 - (11.7 * b + 1.02) * u * kappa;
        if (!(den > 0.5)) return -1.0;
        return E * (11.7 * b + 3.04) / den;
    };

    // per internal node: its box contains both children's; over the tree: every internal node is nested and every coordinate is
    // finite and of ordinary magnitude (what the compressed packets, 4-ary and 8-wide, ask for)
    std::vector<uint8_t> nested(n, 0);
    bool compressible = true;
    for (size_t i = 0; i < n; i++) {
        if (!reached[i]) continue;          // (nested stays 0: never absorbed, never opened)
        const Box b = box_of(src, i);
        for (int k = 0; k < 3; k++)
            if (!(std::fabs(b.mn[k]) < 1e30f && std::fabs(b.mx[k]) < 1e30f)) compressible = false;
        if (is_leaf(src, i)) continue;
        bool ok = true;
        for (int32_t c : { ldi(rec_of(src, i), 32), ldi(rec_of(src, i), 36) })
            if (c < 0 || !contains(b, box_of(src, (size_t)c))) ok = false;
        nested[i] = ok ? 1 : 0;
        if (!ok) compressible = false;
    }

    std::vector<float> wmax(n, 0.0f);       // +inf = never skip
    const float inf = __builtin_inff();
    double lmax = 0.0;
    for (size_t i = n; i-- > 0;) {          // children come after their parent
        const uint8_t *r = rec_of(src, i);
        if (is_leaf(src, i)) {
            const TriVerts &t = tris[(size_t)ldi(r, 40)];
            Box tb;
            for (int k = 0; k < 3; k++) {
                tb.mn[k] = std::fmin(std::fmin(t.a[k], t.b[k]), t.c[k]);
                tb.mx[k] = std::fmax(std::fmax(t.a[k], t.b[k]), t.c[k]);
            }
            double E, Ls;
            tri_el((size_t)ldi(r, 40), E, Ls);
            const double W = (E == E && Ls == Ls) ? weight(E) : -1.0;
            if (W >= 0.0 && Ls <= lcap && contains(box_of(src, i), tb)) {
                wmax[i] = (float)(W * (1.0 + 1e-6));
                if ((double)wmax[i] < W) wmax[i] = std::nextafter(wmax[i], inf);
                if (Ls > lmax) lmax = Ls;
            } else {
                wmax[i] = inf;
            }
        } else {
            wmax[i] = nested[i] ? std::max(wmax[(size_t)ldi(r, 32)], wmax[(size_t)ldi(r, 36)]) : inf;
        }
    }
    {
        // packet numbering of compile_tree: internal nodes in index order
        std::vector<uint32_t> cull(npackets, 0x7f807f80u);
        size_t pk = 0;
        for (size_t i = 0; i < n; i++) {
            if (is_leaf(src, i)) continue;
            const int32_t left = ldi(rec_of(src, i), 32), right = ldi(rec_of(src, i), 36);
            const uint32_t hl = left >= 0 ? round_up_16(wmax[(size_t)left]) : 0x7f80u;
            const uint32_t hr = right >= 0 ? round_up_16(wmax[(size_t)right]) : 0x7f80u;
            if (pk < cull.size()) cull[pk] = (hl << 16) | hr;
            pk++;
        }
        if (pk != npackets) return pt_set_error(MI3PT_ERR_STATE, "cull analysis: packet count mismatch");
        if (int rc = emit(WALK_CULL, cull.data(), cull.size() * 4)) return rc;
    }
    // scene constants of the bound: u / EPSILON and 1.65 L_max u / EPSILON, rounded up (the 1.001 covers the
    // handful of fp32 roundings the kernel adds when it forms delta from them)
    {
        const double ka = u * inv_eps * 1.001 * opt.cull_scale, kb = 1.65 * lmax * u * inv_eps * 1.001 * opt.cull_scale;
        out.cull_ka = std::nextafter((float)ka, inf);
        out.cull_kb = std::nextafter((float)kb, inf);
    }
    // ---- wide (4-ary) packets for the WIDE walk: absorb internal children into their parent, largest
    // surface area first, while the node has fewer than four entries.  Only a child whose box contains
    // its own children's boxes may be absorbed (pt_kernels.h, WidePacket: the monotonicity argument).
    if (!is_leaf(src, 0)) {
        auto area = [&](size_t i) { const double a = half_area(box_of(src, i)); return a == a ? a : 0.0; };
        std::vector<uint32_t> wide_of(n, REF_NONE);            // binary node -> wide packet index
        std::vector<std::array<int32_t, 4>> kids;              // per wide packet: binary child nodes (-1: empty)
        std::vector<uint32_t> queue;                           // breadth-first numbering
        queue.push_back(0);
        wide_of[0] = 0;
        // which descendants a packet holds: the SAH-optimal collapse (pt_host_wide.cpp; a node whose box does not contain its children's is
        // never opened) -- or, MI3PT_OPT_COLLAPSE != 1, the greedy one
        WideCollapse plan4;
        std::vector<int32_t> entries4;
        bool optimal4 = opt.collapse == 1;
        if (optimal4) {
            std::vector<uint8_t> closed(n, 0);
            for (size_t i = 0; i < n; i++) closed[i] = nested[i] ? 0 : 1;
            optimal4 = collapse_optimal(src, n, 4, &closed, plan4);
        }
        for (size_t qi = 0; qi < queue.size(); qi++) {
            const uint32_t x = queue[qi];
            int32_t set[4] = { ldi(rec_of(src, x), 32), ldi(rec_of(src, x), 36), -1, -1 };
            int cnt = 2;
            if (optimal4 && set[0] >= 0 && set[1] >= 0) {
                plan4.children_of(x, entries4);
                if (entries4.size() >= 2 && entries4.size() <= 4) {
                    cnt = (int)entries4.size();
                    for (int k = 0; k < cnt; k++) set[k] = entries4[(size_t)k];
                }
            } else
            while (cnt < 4) {
                int pick = -1;
                double best_area = -1.0;
                for (int k = 0; k < cnt; k++) {
                    const int32_t c = set[k];
                    if (c < 0 || is_leaf(src, (size_t)c) || !nested[(size_t)c] || wide_of[(size_t)c] != REF_NONE) continue;
                    const double a = area((size_t)c);
                    if (a > best_area) { best_area = a; pick = k; }
                }
                if (pick < 0) break;
                const uint8_t *cr = rec_of(src, (size_t)set[pick]);
                set[pick] = ldi(cr, 32);
                set[cnt++] = ldi(cr, 36);
            }
            kids.push_back({ set[0], set[1], set[2], set[3] });
            for (int k = 0; k < cnt; k++) {
                const int32_t c = set[k];
                if (c >= 0 && !is_leaf(src, (size_t)c) && wide_of[(size_t)c] == REF_NONE) {
                    wide_of[(size_t)c] = (uint32_t)queue.size();
                    queue.push_back((uint32_t)c);
                }
            }
        }
        const size_t worst = worst_stack_any_order([&](uint32_t w, uint32_t *ks) {
            int m = 0;
            for (int k = 0; k < 4; k++) {
                const int32_t c = kids[w][(size_t)k];
                if (c >= 0 && !is_leaf(src, (size_t)c)) ks[m++] = wide_of[(size_t)c];
            }
            return m;
        });
        if (worst <= (size_t)SM_CULL_STACK_MAX && kids.size() < 0x7fffffffu) {
            std::vector<WidePacket> wp(kids.size());
            std::memset(wp.data(), 0, wp.size() * sizeof(WidePacket));
            for (size_t w = 0; w < kids.size(); w++) {
                WidePacket &p = wp[w];
                uint32_t cw[4] = { 0x7f80u, 0x7f80u, 0x7f80u, 0x7f80u };
                for (int k = 0; k < 4; k++) {
                    const int32_t c = kids[w][(size_t)k];
                    float *box = k < 2 ? p.b01 + 6 * k : p.b23 + 6 * (k - 2);
                    if (c < 0) { p.ref[k] = REF_NONE; continue; }
                    put_box(box, box + 3, box_of(src, (size_t)c));
                    p.ref[k] = is_leaf(src, (size_t)c) ? (0x80000000u | (uint32_t)ldi(rec_of(src, (size_t)c), 40)) : wide_of[(size_t)c];
                    cw[k] = round_up_16(wmax[(size_t)c]);
                    if (!node_box_safe(src, (size_t)c)) p.flags |= 1u << k;
                    p.flags += 16u;              // bits 4..6: the number of children (the walk's box-test count)
                }
                p.cull01 = (cw[0] << 16) | cw[1];
                p.cull23 = (cw[2] << 16) | cw[3];
            }
            // ---- numbering of the packets in memory (MI3PT_OPT_PACKET_ORDER; the walk follows references, so any numbering with
            // the root at 0 renders the same bits).  Breadth-first (the reference's flattenBVH order carried over, raytrace.ts:667-694)
            // keeps each LEVEL together; depth-first (pre-order) keeps each SUBTREE together: the deep part of a walk -- most of the
            // distinct packets it touches in a tree of millions -- then stays within a few pages; treelets: the top three levels of a
            // subtree breadth-first (up to 21 packets, 1.3 KB), then each of its frontier subtrees the same way.
            if (opt.packet_order != 0 && wp.size() > 1) {
                const size_t nw = wp.size();
                std::vector<uint32_t> order;
                order.reserve(nw);
                auto internal_kids = [&](uint32_t w, uint32_t *ks) { int m = 0; for (int k = 0; k < 4; k++) { const uint32_t r = wp[w].ref[k]; if (r != REF_NONE && !(r & REF_LEAF)) ks[m++] = r; } return m; };
                std::vector<uint32_t> work;
                work.push_back(0u);
                while (!work.empty()) {
                    const uint32_t top = work.back();
                    work.pop_back();
                    if (opt.packet_order == 1) {
                        order.push_back(top);
                        uint32_t ks[4];
                        const int m = internal_kids(top, ks);
                        for (int k = m - 1; k >= 0; k--) work.push_back(ks[k]);          // (first child next)
                    } else {
                        std::vector<uint32_t> level(1, top), next;
                        for (int depth = 0; depth < 3; depth++) {
                            next.clear();
                            for (uint32_t w : level) {
                                order.push_back(w);
                                uint32_t ks[4];
                                const int m = internal_kids(w, ks);
                                for (int k = 0; k < m; k++) next.push_back(ks[k]);
                            }
                            level.swap(next);
                        }
                        for (size_t k = level.size(); k-- > 0;) work.push_back(level[k]);
                    }
                }
                if (order.size() == nw) {
                    std::vector<uint32_t> newid(nw);
                    for (size_t i = 0; i < nw; i++) newid[order[i]] = (uint32_t)i;
                    std::vector<WidePacket> moved(nw);
                    for (size_t w = 0; w < nw; w++) {
                        WidePacket q = wp[w];
                        for (int k = 0; k < 4; k++)
                            if (q.ref[k] != REF_NONE && !(q.ref[k] & REF_LEAF)) q.ref[k] = newid[q.ref[k]];
                        moved[newid[w]] = q;
                    }
                    wp.swap(moved);
                }
            }
            if (int rc = emit(WALK_WIDE, wp.data(), wp.size() * sizeof(WidePacket))) return rc;
            // ---- compressed wide packets + 64-byte triangle records (kernel variant 13): the same packets with the boxes on a
            // per-node 8-bit grid, rounded outward by at least one cell; the exact test moves to the leaf's own box, which travels
            // with the triangle.  Offered when every internal box contains its children's (the reference then reaches a leaf iff
            // the leaf's box passes) and every coordinate is finite and of ordinary magnitude.
            {
                bool ok = compressible;
                std::vector<CWidePacket> cp(ok ? wp.size() : 0);
                for (size_t w = 0; w < cp.size() && ok; w++) {
                    const WidePacket &p = wp[w];
                    CWidePacket &c = cp[w];
                    std::memset(&c, 0, sizeof c);
                    const int nk = (int)((p.flags >> 4) & 7u);
                    c.cull01 = p.cull01; c.cull23 = p.cull23;
                    for (int k = 0; k < 4; k++) c.ref[k] = p.ref[k];
                    uint32_t meta = (uint32_t)nk << 24;
                    for (int ax = 0; ax < 3; ax++) {
                        double lo = 1e300, hi = -1e300, maxabs = 0.0;
                        auto box_at = [&](int k) { return k < 2 ? p.b01 + 6 * k : p.b23 + 6 * (k - 2); };
                        for (int k = 0; k < 4; k++) {
                            if (p.ref[k] == REF_NONE) continue;
                            const float *b = box_at(k);
                            lo = std::min(lo, (double)b[ax]); hi = std::max(hi, (double)b[3 + ax]);
                            maxabs = std::max({ maxabs, std::fabs((double)b[ax]), std::fabs((double)b[3 + ax]) });
                        }
                        if (!(lo <= hi)) { lo = hi = 0.0; }
                        // cell = 2^e: the extent in at most 248 cells (2 below the lowest coordinate for the origin, 1 + 1 of outward rounding
                        // on either side, 254 the largest index used), and no finer than 2^-20 of the largest coordinate (the origin and
                        // the cell boundaries must be far above the fp32 grid of the coordinates themselves)
                        int e = -100;
                        if (hi > lo) e = std::max(e, (int)std::ceil(std::log2((hi - lo) / 248.0)));
                        if (maxabs > 0.0) e = std::max(e, (int)std::floor(std::log2(maxabs)) - 20);
                        double cell = std::ldexp(1.0, e);
                        float o = 0.0f;
                        for (;; e++, cell *= 2.0) {         // (at most a step or two: until the fp32 origin and every index fit)
                            o = (float)(lo - 2.0 * cell);
                            if ((double)o > lo - cell) continue;                         // the origin must leave room for a whole cell of outward rounding
                            if (std::ceil((hi - (double)o) / cell) + 1.0 <= 254.0) break;
                        }
                        if (e + 127 < 1 || e + 127 > 254) { ok = false; break; }
                        c.o[ax] = o;
                        meta |= (uint32_t)(e + 127) << (8 * ax);
                        uint32_t qlo = 0, qhi = 0;
                        for (int k = 0; k < 4; k++) {
                            uint32_t a = 255u, z = 0u;                                   // empty slot: an inverted box; the box test may pass it (PROOFS.md 4a): its ref, REF_NONE, is what makes the pushed entry empty
                            if (p.ref[k] != REF_NONE) {
                                const float *b = box_at(k);
                                const double x0 = ((double)b[ax] - (double)o) / cell, x1 = ((double)b[3 + ax] - (double)o) / cell;     // (the difference is rounded once; the division by a power of two is exact)
                                double f0 = std::floor(x0) - 1.0, f1 = std::ceil(x1) + 1.0;
                                // (x0 / x1 are rounded quotients: a whole cell of margin is decided exactly, see plane_cells_from_origin)
                                if (!plane_cells_from_origin(b[ax], o, (f0 + 1.0) * cell, true)) f0 -= 1.0;
                                if (!plane_cells_from_origin(b[3 + ax], o, (f1 - 1.0) * cell, false)) f1 += 1.0;
                                if (!(f0 >= 0.0 && f1 <= 254.0 && f0 < f1)) { ok = false; break; }
                                a = (uint32_t)f0; z = (uint32_t)f1;
                                // ... and checked the way the kernel's plain-division path DECODES a plane, one fp32 fma: RN(o + cell q) is not
                                // exact in general (o is an arbitrary fp32 value, not a multiple of the cell), but round-to-nearest is monotone and
                                // the child's plane is itself an fp32 value, so a real plane a whole cell outside it cannot round to its inside.
                                // Verified per plane rather than argued: a packet that failed would send the tree to the exact packets.
                                const float cf = (float)cell;
                                if (!(std::fma((float)a, cf, o) <= b[ax] && std::fma((float)z, cf, o) >= b[3 + ax])) { ok = false; break; }
                            }
                            qlo |= a << (8 * k); qhi |= z << (8 * k);
                        }
                        c.qlo[ax] = qlo; c.qhi[ax] = qhi;
                    }
                    c.meta = meta;
                }
                std::vector<TriPacket64> t64(ok ? nt : 0);
                if (ok) {
                    std::vector<uint8_t> seen(nt, 0);
                    // (only the leaves the root reaches: a node nobody walks may name a reachable leaf's triangle with another box, and
                    // the record's box is the exact test of the REACHABLE leaf)
                    for (size_t i = 0; i < n; i++) {
                        if (!is_leaf(src, i) || !reached[i]) continue;
                        const size_t ti = (size_t)ldi(rec_of(src, i), 40);
                        const TriVerts &v = tris[ti];
                        TriPacket64 &q = t64[ti];
                        for (int k = 0; k < 3; k++) {
                            volatile float e1 = v.b[k] - v.a[k], e2 = v.c[k] - v.a[k];        // one fp32 rounding each (see tri_packet_of)
                            q.a[k] = v.a[k]; q.e1[k] = e1; q.e2[k] = e2;
                        }
                        put_box(q.bmin, q.bmax, box_of(src, i));
                        // (the word the 48-byte records keep the material index in: here a flag -- the leaf's box has a coordinate outside the
                        // guard range of the reduced-instruction slab tests, e.g. the 1e-33 residues three.js leaves at a sphere's poles:
                        // its exact test takes the plain divisions.  Internal boxes live on the packets' grids: no such range.)
                        q.unsafe = node_box_safe(src, i) ? 0u : 1u;
                        seen[ti] = 1;
                    }
                    for (size_t t = 0; t < nt; t++)
                        if (!seen[t]) {        // a triangle no leaf refers to is never tested: an empty box keeps its record inert
                            for (int k = 0; k < 3; k++) { t64[t].a[k] = t64[t].e1[k] = t64[t].e2[k] = 0.0f; t64[t].bmin[k] = 1.0f; t64[t].bmax[k] = -1.0f; }
                            t64[t].unsafe = 0;
                        }
                    if (int rc = emit(WALK_CWIDE, cp.data(), cp.size() * sizeof(CWidePacket))) return rc;
                    if (int rc = emit(WALK_TRI64, t64.data(), t64.size() * sizeof(TriPacket64))) return rc;
                    out.cwide_ok = true;
                }
            }
            out.nwide = wp.size();
            out.wide_stack_worst = (int)worst;
            out.wide_ok = true;
            out.wide_root_nested = nested[0] != 0;
        }
    }
    // ---- the 8-wide packets of kernel variant 14: the preconditions of the compressed 4-ary packets, and its own stack bound: the walk's
    // node stack holds one entry per packet LEVEL, whatever the order (the 4-ary walk's bound, up to three entries per level, does not apply).
    // Built only when asked for: an option nobody selected must not cost every scene's first submit the second collapse.
    if (opt.eight_wide && !is_leaf(src, 0) && nt < 0x7fffffffu && compressible) {
        Cw8Build b8;
        if (build_cw8(src, n, reinterpret_cast<const float *>(tris), nt, wmax, b8, opt.collapse == 0)) {
            out.cw8_ok = b8.height <= SM_W8_MIN_LDS_NODES + SM_W8_OVERFLOW_NODES;
            out.cw8_height = b8.height;
            out.cw8_mean_children = b8.mean_children;
            if (out.cw8_ok || opt.eight_wide_any_height) {
                if (int rc = emit(WALK_CW8, b8.packets.data(), b8.packets.size() * sizeof(CW8Packet))) return rc;
                if (int rc = emit(WALK_TRI8, b8.records.data(), b8.records.size() * sizeof(TriPacket64))) return rc;
                out.ncw8 = b8.packets.size();
                out.cw8_records = b8.records.size();
            }
        }
    }
    // ---- which wide walk `auto` means for this scene (variants 10 / 11 / 12 render the same bits; this is speed only).
    // The filtered slab test (11, 12) saves ~45 of a wide step's ~290 vector instructions, but a box that is thin on an
    // axis and entered through that face -- the two triangles of a floor, axis-aligned quads -- has a zero-length
    // approximate interval and always takes the exact test on top: ~30 more instructions for the whole wave.  Estimate
    // of such encounters per wide step: the surface-area share of the thin leaves (the chance that a ray through the
    // root box meets the leaf's box) over the depth of the 4-ary tree.  Measured: demo scene 0.33 -> 10 is 1.5 % faster
    // than 11; dragon-class 0.15 -> 11 is 2-3 % faster than 10 (profiles/r03_a_slab_filter_ab.log).
    // The one-axis culling condition (12) is one operation per child instead of four but skips less; it is chosen when
    // the margins it inflates are negligible anyway: 95th percentile of the leaves' W times k_a times 16 below 2^-10
    // (dragon-class: 4e-4, +1.4 %; the 10 M-triangle forest: 0.5 -- there it doubles the boxes tested).
    out.auto_wide_variant = 10;
    if (out.wide_ok) {
        const Box root = box_of(src, 0);
        double diag = 0.0;
        for (int k = 0; k < 3; k++) { const double ext = (double)root.mx[k] - root.mn[k]; diag += ext * ext; }
        diag = std::sqrt(diag);
        const double area0 = half_area(root);
        const double thin = std::ldexp(diag, -20);
        double thin_share = 0.0;
        std::vector<float> ws;
        ws.reserve(nt);
        for (size_t i = 0; i < n; i++) {
            if (!is_leaf(src, i) || !reached[i]) continue;
            const Box b = box_of(src, i);
            const double x = (double)b.mx[0] - b.mn[0], y = (double)b.mx[1] - b.mn[1], z = (double)b.mx[2] - b.mn[2];
            if ((x <= thin || y <= thin || z <= thin) && area0 > 0.0) {
                const double a = (x * y + x * z + y * z) / area0;
                if (a == a) thin_share += a < 1.0 ? a : 1.0;
            }
            if (wmax[i] < inf) ws.push_back(wmax[i]);
        }
        const double depth = std::log((double)(out.nwide > 4 ? out.nwide : 4)) / std::log(4.0);
        const double thin_per_step = thin_share / depth;
        double w95 = __builtin_inf();
        if (!ws.empty()) {
            const size_t k95 = (ws.size() - 1) * 95 / 100;
            std::nth_element(ws.begin(), ws.begin() + (std::ptrdiff_t)k95, ws.end());
            w95 = ws[k95];
        }
        const double margin = w95 * u * inv_eps * 16.0;
        if (thin_per_step < 0.25) out.auto_wide_variant = margin < std::ldexp(1.0, -10) ? 12 : 11;
    }
    out.analysed = true;
    return MI3PT_OK;
}

}  // namespace pt

// Host-only scene compile (no device, no context: `-m "not gpu"` tests and the sanitizer builds call it): the tree, triangle and walk
// compiles as the context runs them, every buffer reduced to a 64-bit FNV-1a digest of its bytes.  out[] (MI3PT_SCENE_COMPILE_WORDS):
//   0 nodes, 1 triangles, 2 packets, 3 leaf_cap, 4 tree_proper, 5 walk_stack_worst, 6 cull_stack_ok, 7 root_ref, 8 scene_flags, 9 max_tri_ref,
//   10 max_mat_ref, 11 analysed (the walk compile ran: the tree admits the culling walks and its leaves name uploaded triangles), 12 / 13 the
//   bits of cull_ka / cull_kb, 14 wide_ok, 15 cwide_ok, 16 cw8_ok, 17 wide_root_nested, 18 wide_stack_worst, 19 auto_wide_variant, 20 wide
//   packets, 21 8-wide packets, 22 8-wide records, 23 8-wide levels; digests (0: not built): 24 node packets with their final cull words,
//   25 leaf ranks, 26 48-byte triangle packets, 27 wide packets, 28 compressed packets, 29 64-byte records, 30 8-wide packets, 31 8-wide records
extern "C" int mi3pt_host_scene_compile(const void *nodes, size_t nodes_bytes, const void *triangles, size_t triangles_bytes, int collapse,
                                        int packet_order, int want_eight_wide, uint64_t *out, size_t out_capacity)
{
    if (!nodes || !triangles || !out || nodes_bytes == 0 || nodes_bytes % MI3PT_BVHNODE_STRIDE || triangles_bytes == 0 ||
        triangles_bytes % MI3PT_TRIANGLE_STRIDE || out_capacity < MI3PT_SCENE_COMPILE_WORDS || collapse < -1 || collapse > 1 ||
        packet_order < 0 || packet_order > 2)
        return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_scene_compile: bad argument");
    const size_t n = nodes_bytes / MI3PT_BVHNODE_STRIDE, nt = triangles_bytes / MI3PT_TRIANGLE_STRIDE;
    if (n > 0x7fffffffu || nt > 0x7fffffffu) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_scene_compile: too many nodes or triangles");
    const uint8_t *src = static_cast<const uint8_t *>(nodes), *tsrc = static_cast<const uint8_t *>(triangles);
    auto fnv = [](const void *p, size_t bytes) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (size_t i = 0; i < bytes; i++) { h ^= static_cast<const uint8_t *>(p)[i]; h *= 0x100000001b3ull; }
        return h;
    };
    auto bits = [](float f) { uint32_t b; std::memcpy(&b, &f, 4); return (uint64_t)b; };
    for (size_t k = 0; k < MI3PT_SCENE_COMPILE_WORDS; k++) out[k] = 0;
    pt::TreeCompile tree;
    if (const char *e = pt::compile_tree(src, n, tree)) return pt_set_error(MI3PT_ERR_INVALID, e);
    std::vector<pt::TriPacket> tripk;
    int64_t max_mat = -1;
    if (const char *e = pt::compile_triangles(tsrc, nt, tripk, max_mat)) return pt_set_error(MI3PT_ERR_INVALID, e);
    pt::WalkCompile walk;
    if (tree.cull_stack_ok && tree.npackets != 0) {      // (what the context asks of the scene before it runs the analysis)
        pt::WalkOptions opt;
        opt.collapse = collapse; opt.packet_order = packet_order; opt.eight_wide = want_eight_wide != 0;
        const std::vector<pt::TriVerts> verts = pt::triangle_verts(tsrc, nt);
        auto sink = [&](pt::WalkBuffer kind, const void *p, size_t bytes) {
            if (kind == pt::WALK_CULL)
                for (size_t i = 0; i < tree.npackets; i++) tree.packets[i].cull = static_cast<const uint32_t *>(p)[i];
            else
                out[27 + (kind - pt::WALK_WIDE)] = fnv(p, bytes);
            return MI3PT_OK;
        };
        if (int rc = pt::compile_walk(src, n, verts.data(), nt, tree.npackets, opt, sink, walk)) return rc;
    }
    const uint64_t scalars[24] = {
        n, nt, tree.npackets, (uint64_t)tree.leaf_cap, tree.tree_proper, (uint64_t)tree.walk_stack_worst, tree.cull_stack_ok, tree.root_ref,
        tree.scene_flags, (uint64_t)tree.max_tri_ref, (uint64_t)max_mat, walk.analysed, bits(walk.cull_ka), bits(walk.cull_kb), walk.wide_ok,
        walk.cwide_ok, walk.cw8_ok, walk.wide_root_nested, (uint64_t)walk.wide_stack_worst, walk.analysed ? (uint64_t)walk.auto_wide_variant : 0, walk.nwide,
        walk.ncw8, walk.cw8_records, walk.cw8_ok ? (uint64_t)walk.cw8_height : 0 };
    for (int k = 0; k < 24; k++) out[k] = scalars[k];
    out[24] = fnv(tree.packets.data(), tree.packets.size() * sizeof(pt::NodePacket));
    out[25] = fnv(tree.leaf_rank.data(), tree.leaf_rank.size() * sizeof(uint32_t));
    out[26] = fnv(tripk.data(), tripk.size() * sizeof(pt::TriPacket));
    return MI3PT_OK;
}

// Host-only: the bytes of one of the buffers compile_walk emits (kind: pt::WalkBuffer -- 0 cull words, 1 wide packets, 2 compressed packets,
// 3 64-byte records, 4 8-wide packets, 5 8-wide records), for the same arguments and by the same calls as mi3pt_host_scene_compile: they
// hash to its words 27 .. 31.  *bytes_out = the buffer's size (0: not built for this tree); copied to `out` when it is given.
extern "C" int mi3pt_host_walk_buffer(const void *nodes, size_t nodes_bytes, const void *triangles, size_t triangles_bytes, int collapse,
                                      int packet_order, int kind, void *out, size_t capacity, size_t *bytes_out)
{
    if (!nodes || !triangles || !bytes_out || nodes_bytes == 0 || nodes_bytes % MI3PT_BVHNODE_STRIDE || triangles_bytes == 0 ||
        triangles_bytes % MI3PT_TRIANGLE_STRIDE || collapse < -1 || collapse > 1 || packet_order < 0 || packet_order > 2 ||
        kind < (int)pt::WALK_CULL || kind > (int)pt::WALK_TRI8)
        return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_walk_buffer: bad argument");
    const size_t n = nodes_bytes / MI3PT_BVHNODE_STRIDE, nt = triangles_bytes / MI3PT_TRIANGLE_STRIDE;
    if (n > 0x7fffffffu || nt > 0x7fffffffu) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_walk_buffer: too many nodes or triangles");
    const uint8_t *src = static_cast<const uint8_t *>(nodes), *tsrc = static_cast<const uint8_t *>(triangles);
    *bytes_out = 0;
    pt::TreeCompile tree;
    if (const char *e = pt::compile_tree(src, n, tree)) return pt_set_error(MI3PT_ERR_INVALID, e);
    if (!(tree.cull_stack_ok && tree.npackets != 0)) return MI3PT_OK;
    pt::WalkOptions opt;
    opt.collapse = collapse; opt.packet_order = packet_order; opt.eight_wide = kind >= (int)pt::WALK_CW8;
    const std::vector<pt::TriVerts> verts = pt::triangle_verts(tsrc, nt);
    std::vector<uint8_t> kept;
    auto sink = [&](pt::WalkBuffer k, const void *p, size_t bytes) {
        if ((int)k == kind) kept.assign(static_cast<const uint8_t *>(p), static_cast<const uint8_t *>(p) + bytes);
        return MI3PT_OK;
    };
    pt::WalkCompile walk;
    if (int rc = pt::compile_walk(src, n, verts.data(), nt, tree.npackets, opt, sink, walk)) return rc;
    *bytes_out = kept.size();
    if (out) {
        if (capacity < kept.size()) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_walk_buffer: the buffer is larger than `capacity`");
        if (!kept.empty()) std::memcpy(out, kept.data(), kept.size());
    }
    return MI3PT_OK;
}
