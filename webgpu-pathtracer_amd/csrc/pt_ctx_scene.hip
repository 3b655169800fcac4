// pt_ctx_scene.hip -- the scene a context holds (uploads, the kept geometry, the device builders) and its lazy analyses.
#include "../../include/mi3pt.h"
#include "pt_ctx_calls.h"

#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

// Replace *dst with a device copy of `bytes`.
static int replace_buffer(mi3pt_ctx *ctx, DevBuf<void> &dst, const void *bytes, size_t nbytes)
{
    DevBuf<void> fresh;
    HIP_TRY(fresh.alloc(nbytes));
    hipError_t e = ctx_stream_sync(ctx, ctx->stream, "upload");      // (bounded; a large copy from pageable memory blocks the host until the stream gets there)
    if (e == hipSuccess) e = hipMemcpyAsync(fresh, bytes, nbytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = ctx_stream_sync(ctx, ctx->stream);   // copy-on-call: caller may reuse `bytes`
    if (e != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, std::string("upload: ") + hipGetErrorString(e));
    dst = std::move(fresh);
    ctx->scene_epoch++;
    return MI3PT_OK;
}

extern "C" int mi3pt_upload_triangles(mi3pt_ctx *ctx, const void *bytes, size_t nbytes)
{
    PT_GROUP(ctx, mi3pt_upload_triangles(group_member0(ctx), bytes, nbytes));      // (a group's scene lives in member 0; the others receive device copies: group_sync_scene)
    if (int rc = require_idle(ctx)) return rc;
    if (!bytes || nbytes == 0 || nbytes % MI3PT_TRIANGLE_STRIDE)
        return pt_set_error(MI3PT_ERR_INVALID, "triangle bytes must be a non-zero multiple of 112");
    const size_t n = nbytes / MI3PT_TRIANGLE_STRIDE;
    if (n > 0x7fffffffu) return pt_set_error(MI3PT_ERR_INVALID, "too many triangles");
    std::vector<pt::TriPacket> pk;
    int64_t max_mat = -1;
    if (const char *e = pt::compile_triangles(static_cast<const uint8_t *>(bytes), n, pk, max_mat)) return pt_set_error(MI3PT_ERR_INVALID, e);
    // (mi3pt_keep_geometry: the first upload after it hands the records over as the previous geometry instead of freeing them)
    const bool hand_over = ctx->geometry_kept && !ctx->d_tris_kept;
    DevBuf<void> tris;
    if (int rc = replace_buffer(ctx, tris, bytes, nbytes)) return rc;
    if (hand_over) ctx->d_tris_kept = std::move(ctx->d_tris);
    ctx->d_tris = std::move(tris);
    ctx->upload_epoch++;
    if (int rc = replace_buffer(ctx, ctx->d_tripk, pk.data(), n * sizeof(pt::TriPacket))) return rc;
    ctx->ntris = n;
    ctx->host_analyses++;
    ctx->max_mat_ref = max_mat;
    ctx->cull_dirty = true;
    ctx->cost_state = 0;            // (the tiles' costs were measured on another scene)
    if (ctx->layout_active && ctx->nnodes > 0) {
        // The device holds node packets, leaf ranks and the root reference in the visiting-order numbering of the debug
        // layout, while the triangles just uploaded are in uploaded order again: rebuild the tree's side from the node
        // records, which are kept as uploaded (round-2 advice: leaves referenced the wrong triangles after a
        // triangles-only upload that followed mi3pt_debug_set_packet_layout(ctx, 0)).
        std::vector<uint8_t> nodes(ctx->nnodes * MI3PT_BVHNODE_STRIDE);
        HIP_TRY(hipMemcpy(nodes.data(), ctx->d_nodes, nodes.size(), hipMemcpyDeviceToHost));
        ctx->layout_active = false;
        return mi3pt_upload_bvh(ctx, nodes.data(), nodes.size());
    }
    ctx->layout_active = false;
    ctx->layout_dirty = ctx->layout != 0;
    return MI3PT_OK;
}

extern "C" int mi3pt_upload_materials(mi3pt_ctx *ctx, const void *bytes, size_t nbytes)
{
    PT_GROUP(ctx, mi3pt_upload_materials(group_member0(ctx), bytes, nbytes));      // (a group's scene lives in member 0; the others receive device copies: group_sync_scene)
    if (int rc = require_idle(ctx)) return rc;
    if (!bytes || nbytes == 0 || nbytes % MI3PT_MATERIAL_STRIDE)
        return pt_set_error(MI3PT_ERR_INVALID, "material bytes must be a non-zero multiple of 64");
    if (int rc = replace_buffer(ctx, ctx->d_mats, bytes, nbytes)) return rc;
    ctx->upload_epoch++;
    ctx->nmats = nbytes / MI3PT_MATERIAL_STRIDE;
    return MI3PT_OK;
}

extern "C" int mi3pt_upload_bvh(mi3pt_ctx *ctx, const void *bytes, size_t nbytes)
{
    PT_GROUP(ctx, mi3pt_upload_bvh(group_member0(ctx), bytes, nbytes));      // (a group's scene lives in member 0; the others receive device copies: group_sync_scene)
    if (int rc = require_idle(ctx)) return rc;
    if (!bytes || nbytes == 0 || nbytes % MI3PT_BVHNODE_STRIDE)
        return pt_set_error(MI3PT_ERR_INVALID, "BVH bytes must be a non-zero multiple of 48");
    const size_t n = nbytes / MI3PT_BVHNODE_STRIDE;
    if (n > 0x7fffffffu) return pt_set_error(MI3PT_ERR_INVALID, "too many BVH nodes");
    const uint8_t *src = static_cast<const uint8_t *>(bytes);
    pt::TreeCompile t;
    if (const char *e = pt::compile_tree(src, n, t)) return pt_set_error(MI3PT_ERR_INVALID, e);
    if (int rc = replace_buffer(ctx, ctx->d_nodes, bytes, nbytes)) return rc;
    ctx->upload_epoch++;
    if (int rc = replace_buffer(ctx, ctx->d_packets, t.packets.data(), t.packets.size() * sizeof(pt::NodePacket))) return rc;
    if (int rc = replace_buffer(ctx, ctx->d_leaf_rank, t.leaf_rank.data(), t.leaf_rank.size() * sizeof(uint32_t))) return rc;
    ctx->leaf_cap = t.leaf_cap;
    ctx->cull_stack_ok = t.cull_stack_ok;
    ctx->tree_proper = t.tree_proper;
    ctx->nodes_reached = t.reached;
    ctx->walk_stack_worst = t.walk_stack_worst;
    ctx->nnodes = n;
    ctx->npackets = t.npackets;
    ctx->root_ref = t.root_ref;
    ctx->scene_flags = t.scene_flags;
    ctx->max_tri_ref = t.max_tri_ref;
    // the cut behind the empty tiles of a view: the nesting of EVERY node's box is checked (the collapse checks it for the nodes it absorbs only)
    ctx->sky_cut_ok = t.tree_proper && pt::sky_cut_of(src, n, ctx->sky_cut);
    ctx->sky_host_valid = false;
    ctx->cull_dirty = true;
    ctx->cost_state = 0;            // (the tiles' costs were measured on another scene)
    ctx->layout_active = false;
    ctx->layout_dirty = ctx->layout != 0;
    ctx->scene_epoch++;
    ctx->host_analyses++;
    return MI3PT_OK;
}

static int upload_env_like(mi3pt_ctx *ctx, void *dst, const float *rgba, int width, int height)
{
    if (int rc = require_idle(ctx)) return rc;
    if (!rgba) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (width != MI3PT_ENV_WIDTH || height != MI3PT_ENV_HEIGHT)   // renderer.ts:133-137
        return pt_set_error(MI3PT_ERR_INVALID,
                            "Environment texture must be 1024x512 pixels. Please resize the texture and try again.");
    const size_t nbytes = (size_t)width * height * 16;
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream, "upload"));
    HIP_TRY(hipMemcpyAsync(dst, rgba, nbytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    ctx->scene_epoch++;
    return MI3PT_OK;
}

extern "C" int mi3pt_upload_environment(mi3pt_ctx *ctx, const float *rgba, int width, int height)
{
    PT_GROUP(ctx, mi3pt_upload_environment(group_member0(ctx), rgba, width, height));      // (a group's scene lives in member 0; the others receive device copies: group_sync_scene)
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    return upload_env_like(ctx, ctx->d_env, rgba, width, height);
}

extern "C" int mi3pt_upload_environment_cdf(mi3pt_ctx *ctx, const float *rgba, int width, int height)
{
    PT_GROUP(ctx, mi3pt_upload_environment_cdf(group_member0(ctx), rgba, width, height));      // (a group's scene lives in member 0; the others receive device copies: group_sync_scene)
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    return upload_env_like(ctx, ctx->d_cdf, rgba, width, height);
}

pt::SceneRefs scene_refs(const mi3pt_ctx *ctx)
{
    pt::SceneRefs s;
    s.tris = (ctx->layout_active ? ctx->d_tris_perm : ctx->d_tris).as<const float4>();
    s.nodes = ctx->d_nodes.as<const float4>();
    s.mats = ctx->d_mats.as<const float4>();
    s.env = ctx->d_env.as<const float4>();
    s.packets = ctx->d_packets.as<const float4>();
    s.tripk = ctx->d_tripk.as<const float4>();
    s.leaf_rank = ctx->d_leaf_rank.as<const uint32_t>();
    s.leaf_cap = ctx->leaf_cap;
    s.wide = ctx->d_wide.as<const float4>();
    s.cwide = ctx->cwide_ok ? ctx->d_cwide.as<const float4>() : nullptr;
    s.tripk64 = ctx->cwide_ok ? ctx->d_tripk64.as<const float4>() : nullptr;
    s.cw8 = ctx->cw8_ok ? ctx->d_cw8.as<const float4>() : nullptr;
    s.tripk8 = ctx->cw8_ok ? ctx->d_tripk8.as<const float4>() : nullptr;
    s.wide_leaf_cap = ctx->wide_ok ? ctx->wide_leaf_cap : 0;
    s.wide_root = ctx->wide_root;
    s.cdf = ctx->d_cdf.as<const float4>();
    s.env_sampling = (ctx->env_sampling && ctx->d_cdf) ? 1 : 0;
    s.ntris = (uint32_t)ctx->ntris; s.nnodes = (uint32_t)ctx->nnodes; s.nmats = (uint32_t)ctx->nmats;
    s.npackets = (uint32_t)ctx->npackets;
    s.root_ref = ctx->root_ref;
    s.flags = ctx->scene_flags;
    if ((ctx->wide_ok && ctx->wide_root_nested) || ctx->cw8_ok) s.flags |= 2u;      // (pt_kernels.h SceneRefs::flags bit 1; the 8-wide packets are only built for trees whose every box is nested)
    if (ctx->wide_ok && ctx->auto_wide_variant == 12) s.flags |= 4u;  // (bit 2: the one-axis culling condition suits this scene -- variant 13 takes the hint)
    s.cull_ka = ctx->cull_ka; s.cull_kb = ctx->cull_kb;
#ifdef MI3PT_EXPERIMENTS
    if (ctx->exp_force_slow_slab) s.flags = 0;
#endif
    s.env_w = MI3PT_ENV_WIDTH; s.env_h = MI3PT_ENV_HEIGHT;
    return s;
}

// The scene is complete when the three buffers agree with each other.  An empty
// scene (no BVH uploaded) is legal: every ray misses (raytrace.wgsl:206-207).
int check_scene(const mi3pt_ctx *ctx)
{
    if (ctx->nnodes == 0) return MI3PT_OK;
    if (ctx->max_tri_ref >= (int64_t)ctx->ntris)
        return pt_set_error(MI3PT_ERR_STATE, "BVH references a triangle index beyond the triangle buffer");
    if (ctx->max_tri_ref >= 0 && ctx->max_mat_ref >= (int64_t)ctx->nmats)
        return pt_set_error(MI3PT_ERR_STATE, "a triangle references a material index beyond the material buffer");
    return MI3PT_OK;
}

// Debug relabelling (mi3pt_debug_set_packet_layout(ctx, 1)): node packets numbered in the reference's
// visiting order (node, right subtree, left subtree: left is pushed first, raytrace.wgsl:184-198)
// and triangles -- 112-B records, 48-B packets, leaf ranks -- stored in leaf-visiting order.  Only
// names change: every packet holds the same boxes, every leaf the same triangle, so images and
// counters must be bit-identical to the breadth-first layout in every packet-walking kernel
// (tests/test_gpu_parity.py::test_depth_first_relabelling_is_bit_identical).  Applied lazily
// because it needs both uploads; needs a proper tree (tree_proper).  The distance-culling walk
// is not offered in this layout (variant 0 / 9 run 7).
int prepare_layout(mi3pt_ctx *ctx)
{
    if (!ctx->layout_dirty) return MI3PT_OK;
    if (ctx->layout == 0 || ctx->nnodes == 0 || ctx->ntris == 0 || !ctx->tree_proper || ctx->max_tri_ref >= (int64_t)ctx->ntris)
        return MI3PT_OK;       // stays dirty; the uploaded (breadth-first) arrangement is complete by itself
    if (int rc = flush_pending(ctx)) return rc;
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    for (int k = 0; k < 2; k++) HIP_TRY(ctx_stream_sync(ctx, ctx->rt_stream[k]));
    const size_t n = ctx->nnodes, nt = ctx->ntris;
    std::vector<uint8_t> nodes(n * MI3PT_BVHNODE_STRIDE), tris(nt * MI3PT_TRIANGLE_STRIDE);
    HIP_TRY(hipMemcpy(nodes.data(), ctx->d_nodes, nodes.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tris.data(), ctx->d_tris, tris.size(), hipMemcpyDeviceToHost));
    const uint8_t *src = nodes.data();
    std::vector<uint32_t> packet_of(n, pt::REF_NONE), tri_new(nt, 0xffffffffu);
    uint32_t npk = 0, ntri = 0;
    std::vector<uint32_t> st;
    st.push_back(0);
    while (!st.empty()) {
        const uint32_t node = st.back();
        st.pop_back();
        const uint8_t *r = src + (size_t)node * MI3PT_BVHNODE_STRIDE;
        if (ldi(r, 28) == 1) {
            tri_new[(size_t)ldi(r, 40)] = ntri++;
        } else {
            packet_of[node] = npk++;
            st.push_back((uint32_t)ldi(r, 32));
            st.push_back((uint32_t)ldi(r, 36));
        }
    }
    for (size_t i = 0; i < n; i++)        // internal nodes the root does not reach keep a packet (never walked)
        if (ldi(src + i * MI3PT_BVHNODE_STRIDE, 28) != 1 && packet_of[i] == pt::REF_NONE) packet_of[i] = npk++;
    for (size_t t = 0; t < nt; t++)
        if (tri_new[t] == 0xffffffffu) tri_new[t] = ntri++;
    if (npk != ctx->npackets || ntri != nt) return pt_set_error(MI3PT_ERR_STATE, "packet layout: counts do not match the upload");
    std::vector<pt::NodePacket> pk;
    pt::build_packets(src, n, packet_of, npk, tri_new.data(), pk);
    std::vector<uint8_t> tris_perm(tris.size());
    std::vector<pt::TriPacket> tripk(nt);
    std::vector<uint32_t> rank(nt);
    for (size_t t = 0; t < nt; t++) {
        const uint8_t *rec = tris.data() + t * MI3PT_TRIANGLE_STRIDE;
        const size_t to = tri_new[t];
        std::memcpy(tris_perm.data() + to * MI3PT_TRIANGLE_STRIDE, rec, MI3PT_TRIANGLE_STRIDE);
        tripk[to] = pt::tri_packet_of(rec);
        rank[to] = (uint32_t)to;          // leaf-visiting order IS the new numbering
    }
    if (int rc = replace_buffer(ctx, ctx->d_packets, pk.data(), pk.size() * sizeof(pt::NodePacket))) return rc;
    if (int rc = replace_buffer(ctx, ctx->d_tripk, tripk.data(), nt * sizeof(pt::TriPacket))) return rc;
    if (int rc = replace_buffer(ctx, ctx->d_leaf_rank, rank.data(), nt * sizeof(uint32_t))) return rc;
    if (int rc = replace_buffer(ctx, ctx->d_tris_perm, tris_perm.data(), tris_perm.size())) return rc;
    ctx->root_ref = pt::child_ref(src, packet_of, tri_new.data(), 0);
    ctx->layout_active = true;
    ctx->layout_dirty = false;
    ctx->scene_epoch++;
    ctx->host_analyses++;
    ctx->cull_ok = false;           // the analysis below works on the uploaded numbering
    ctx->cull_dirty = true;
    ctx->cost_state = 0;            // (the tiles' costs were measured on another scene)
    ctx->main_dirty = true;
    return MI3PT_OK;
}

extern "C" int mi3pt_debug_set_packet_layout(mi3pt_ctx *ctx, int layout)
{
    PT_GROUP(ctx, mi3pt_debug_set_packet_layout(group_member0(ctx), layout));
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    if (layout != 0 && layout != 1) return pt_set_error(MI3PT_ERR_INVALID, "layout must be 0 (breadth-first) or 1 (visiting order)");
    if (int rc = require_idle(ctx)) return rc;
    // (switching back to 0 leaves a relabelled scene on the device as it is -- it is complete and
    // consistent -- until the BVH or the triangles are uploaded again)
    ctx->layout = layout;
    ctx->layout_dirty = layout != 0 && !ctx->layout_active;
    return MI3PT_OK;
}

// The lazy scene analysis behind the culling walks (kernel variants 9 .. 14): pt::compile_walk (pt_host_compile.cpp) on the device's own
// copies of the tree and the vertices; runs when the triangles, the tree or an option that shapes the packets changed.
int prepare_cull(mi3pt_ctx *ctx)
{
    if (!ctx->cull_dirty) return MI3PT_OK;
    const bool wanted = (ctx->variant >= 9 && ctx->variant <= 14) || (ctx->variant == 0 && ctx->cull_enabled);
    if (!wanted || ctx->layout_active || !ctx->cull_stack_ok || ctx->env_sampling || ctx->nnodes == 0 || ctx->ntris == 0 || ctx->npackets == 0)
        return MI3PT_OK;       // stays dirty: pick_variant falls back to the reference-counter walk
    if (int rc = flush_pending(ctx)) return rc;
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    for (int k = 0; k < 2; k++) HIP_TRY(ctx_stream_sync(ctx, ctx->rt_stream[k]));
    const size_t n = ctx->nnodes, nt = ctx->ntris;
    std::vector<uint8_t> nodes(n * MI3PT_BVHNODE_STRIDE);
    // the three vertices of every triangle: the first 48 of every 112 bytes of the records, packed by a small kernel (the 48-B
    // triangle packets hold edges, not b and c; uploaded numbering -- the analysis does not run on a relabelled scene)
    std::vector<pt::TriVerts> tris(nt);
    HIP_TRY(hipMemcpy(nodes.data(), ctx->d_nodes, nodes.size(), hipMemcpyDeviceToHost));
    {
        DevBuf<float4> packed;
        HIP_TRY(packed.alloc(nt * sizeof(pt::TriVerts)));
        pt::launch_pack_vertices(ctx->d_tris.as<const float4>(), packed, (uint32_t)nt, ctx->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = read_plane(ctx, packed, nt * sizeof(pt::TriVerts), tris.data());
        if (e != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, std::string("cull analysis: reading the vertices back: ") + hipGetErrorString(e));
    }
    pt::WalkOptions opt;
    opt.collapse = ctx->collapse;
    opt.packet_order = ctx->packet_order;
    // (the 8-wide packets only for a context that has asked for the walk: mi3pt_set_kernel_variant(ctx, 14) marks the analysis dirty when they are missing)
    opt.eight_wide = ctx->variant == 14;
#ifdef MI3PT_EXPERIMENTS
    opt.cull_scale = ctx->exp_cull_scale;
#endif
    DevBuf<void> *const buffer_of[] = { nullptr, &ctx->d_wide, &ctx->d_cwide, &ctx->d_tripk64, &ctx->d_cw8, &ctx->d_tripk8 };
    auto upload = [&](pt::WalkBuffer kind, const void *data, size_t bytes) -> int {
        if (kind != pt::WALK_CULL) return replace_buffer(ctx, *buffer_of[kind], data, bytes);
        // the first buffer out: from here on the device no longer holds the walks' packets of the scene before
        ctx->wide_ok = ctx->cwide_ok = ctx->cw8_ok = false;
        DevBuf<uint32_t> d_cull;
        HIP_TRY(d_cull.alloc(bytes));
        hipError_t e = hipMemcpyAsync(d_cull, data, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            pt::launch_patch_cull(ctx->d_packets.as<float4>(), d_cull, (uint32_t)ctx->npackets, ctx->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = ctx_stream_sync(ctx, ctx->stream);
        if (e != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, std::string("cull analysis: ") + hipGetErrorString(e));
        return MI3PT_OK;
    };
    pt::WalkCompile w;
    if (int rc = pt::compile_walk(nodes.data(), n, tris.data(), nt, ctx->npackets, opt, upload, w)) return rc;
    if (!w.analysed) return MI3PT_OK;       // a leaf names a triangle that was not uploaded: check_scene reports it; stays dirty
    ctx->cull_ka = w.cull_ka; ctx->cull_kb = w.cull_kb;
    ctx->wide_ok = w.wide_ok;
    ctx->cwide_ok = w.cwide_ok;
    if (w.wide_ok) {
        ctx->nwide = w.nwide;
        ctx->wide_leaf_cap = pt::SM_CULL_LEAF_CAP;
        ctx->wide_root = 0;
        ctx->wide_stack_worst = w.wide_stack_worst;
        ctx->wide_root_nested = w.wide_root_nested;
    }
    ctx->cw8_ok = w.cw8_ok;
    ctx->cw8_tried = opt.eight_wide;
    if (w.cw8_ok) {
        ctx->ncw8 = w.ncw8;
        ctx->cw8_height = w.cw8_height;
        ctx->cw8_records = w.cw8_records;
    }
    ctx->auto_wide_variant = w.auto_wide_variant;
    ctx->cull_ok = true;
    ctx->deep_by_view = false;           // (another scene: judged anew from its first launch)
    ctx->cull_dirty = false;
    ctx->main_dirty = true;
    ctx->scene_epoch++;
    ctx->host_analyses++;
    return MI3PT_OK;
}

extern "C" int mi3pt_keep_geometry(mi3pt_ctx *ctx, int keep)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_keep_geometry: not built for a device group (mi3pt_reproject_scene is not)"));
    if (int rc = require_ctx(ctx)) return rc;
    if (keep && (!ctx->d_tris || ctx->ntris == 0))
        return pt_set_error(MI3PT_ERR_STATE, "mi3pt_keep_geometry: no triangles uploaded (mi3pt_upload_triangles)");
    if (ctx->d_tris_kept) {        // (a second keep, or the release: behind whatever still reads the buffer)
        HIP_TRY(ctx_stream_sync(ctx, ctx->stream, "mi3pt_keep_geometry"));
        ctx->d_tris_kept.reset();
    }
    ctx->geometry_kept = keep != 0;
    ctx->ntris_kept = keep ? ctx->ntris : 0;
    ctx->kept_epoch = keep ? ctx->upload_epoch : 0;
    return MI3PT_OK;
}

extern "C" int mi3pt_device_build_bvh(mi3pt_ctx *ctx, void *nodes_out, size_t nodes_capacity_bytes, size_t *nnodes_out, float *build_ms)
{
    PT_GROUP(ctx, mi3pt_device_build_bvh(group_member0(ctx), nodes_out, nodes_capacity_bytes, nnodes_out, build_ms));
    if (int rc = require_idle(ctx)) return rc;
    if (!nodes_out || !nnodes_out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (!ctx->d_tris || ctx->ntris == 0) return pt_set_error(MI3PT_ERR_STATE, "no triangles uploaded (mi3pt_upload_triangles)");
    const size_t nodes = 2 * ctx->ntris - 1;
    if (nodes_capacity_bytes < nodes * MI3PT_BVHNODE_STRIDE) return pt_set_error(MI3PT_ERR_INVALID, "node buffer too small");
    std::string err;
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    if (pt::lbvh_build(ctx->d_tris, ctx->ntris, nodes_out, build_ms, ctx->stream, err) != 0)
        return pt_set_error(MI3PT_ERR_HIP, "device BVH build: " + err);
    *nnodes_out = nodes;
    return MI3PT_OK;
}

// The device builders by name (pt_lbvh.hip, pt_ploc.hip).  Reads d_tris, writes temporaries of its own: no field of the context moves.
extern "C" int mi3pt_device_build_bvh_ex(mi3pt_ctx *ctx, const mi3pt_bvh_build_params *params, void *nodes_out, size_t nodes_capacity_bytes,
                                         size_t *nnodes_out, mi3pt_bvh_build_info *info)
{
    PT_GROUP(ctx, mi3pt_device_build_bvh_ex(group_member0(ctx), params, nodes_out, nodes_capacity_bytes, nnodes_out, info));
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    if (!params || !nodes_out || !nnodes_out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (params->method != MI3PT_BVH_METHOD_LBVH && params->method != MI3PT_BVH_METHOD_PLOC)
        return pt_set_error(MI3PT_ERR_INVALID, "device BVH build: unknown method");
    if (params->flags != 0) return pt_set_error(MI3PT_ERR_INVALID, "device BVH build: flags must be 0");
    if (params->method == MI3PT_BVH_METHOD_PLOC) {
        if (params->radius < 1 || params->radius > 64) return pt_set_error(MI3PT_ERR_INVALID, "device BVH build: radius must be 1 .. 64");
        if (params->max_search_iterations < 0 || params->max_search_iterations > 65535)
            return pt_set_error(MI3PT_ERR_INVALID, "device BVH build: max_search_iterations must be 0 .. 65535");
    }
    if (int rc = require_idle(ctx)) return rc;
    if (!ctx->d_tris || ctx->ntris == 0) return pt_set_error(MI3PT_ERR_STATE, "no triangles uploaded (mi3pt_upload_triangles)");
    const size_t nodes = 2 * ctx->ntris - 1;
    if (nodes_capacity_bytes < nodes * MI3PT_BVHNODE_STRIDE) return pt_set_error(MI3PT_ERR_INVALID, "node buffer too small");
    std::string err;
    mi3pt_bvh_build_info got = { 0.0f, 0u, 0u };
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    const int rc = params->method == MI3PT_BVH_METHOD_LBVH
        ? pt::lbvh_build(ctx->d_tris, ctx->ntris, nodes_out, &got.build_ms, ctx->stream, err)
        : pt::ploc_build(ctx->d_tris, ctx->ntris, params->radius, params->max_search_iterations, nodes_out, &got.build_ms,
                         &got.search_iterations, &got.forced_iterations, ctx->stream, err);
    if (rc != 0) return pt_set_error(MI3PT_ERR_HIP, "device BVH build: " + err);
    *nnodes_out = nodes;
    if (info) *info = got;
    return MI3PT_OK;
}

// The boxes of the uploaded tree re-fitted to the uploaded triangles (pt_refit.hip).  Reads d_nodes and d_tris, writes temporaries of its own:
// no field of the context moves.
extern "C" int mi3pt_device_refit_bvh(mi3pt_ctx *ctx, void *nodes_out, size_t nodes_capacity_bytes, size_t *nnodes_out, float *refit_ms)
{
    PT_GROUP(ctx, mi3pt_device_refit_bvh(group_member0(ctx), nodes_out, nodes_capacity_bytes, nnodes_out, refit_ms));
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    if (!nodes_out || !nnodes_out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = require_idle(ctx)) return rc;
    if (!ctx->d_nodes || ctx->nnodes == 0) return pt_set_error(MI3PT_ERR_STATE, "no BVH uploaded (mi3pt_upload_bvh)");
    if (!ctx->d_tris || ctx->ntris == 0) return pt_set_error(MI3PT_ERR_STATE, "no triangles uploaded (mi3pt_upload_triangles)");
    if (!ctx->tree_proper)
        return pt_set_error(MI3PT_ERR_STATE, "refit needs a proper tree: every node reached once from node 0, one leaf per triangle, depth under 64");
    if (ctx->nodes_reached != ctx->nnodes)
        return pt_set_error(MI3PT_ERR_STATE, "refit needs every record of the buffer within reach of node 0: the uploaded tree holds records the root does not reach");
    if (ctx->max_tri_ref >= (int64_t)ctx->ntris)
        return pt_set_error(MI3PT_ERR_STATE, "BVH references a triangle index beyond the triangle buffer");
    if (nodes_capacity_bytes < ctx->nnodes * MI3PT_BVHNODE_STRIDE) return pt_set_error(MI3PT_ERR_INVALID, "node buffer too small");
    std::string err;
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    if (pt::refit_bvh(ctx->d_tris, ctx->ntris, ctx->d_nodes, ctx->nnodes, nodes_out, refit_ms, ctx->stream, err) != 0)
        return pt_set_error(MI3PT_ERR_HIP, "device BVH refit: " + err);
    *nnodes_out = ctx->nnodes;
    return MI3PT_OK;
}
