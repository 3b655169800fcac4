// pt_ctx_image.hip -- the images of a context (resize, reset, read / write / hand out) and the features that work on them.
#include "../../include/mi3pt.h"
#include "pt_ctx_calls.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

static hipError_t write_plane(mi3pt_ctx *ctx, void *dst, const void *src, size_t nbytes)
{
    if (nbytes == 0) return hipSuccess;
    hipError_t e = ctx_stream_sync(ctx, ctx->stream, "write-back");
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src, nbytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = ctx_stream_sync(ctx, ctx->stream);      // copy-on-call
    return e;
}

// what every *_device_ptr entry point ends with
static int hand_out_plane(const mi3pt_ctx *ctx, const void *plane, void **dev_ptr, size_t *nbytes)
{
    *dev_ptr = const_cast<void *>(plane);
    if (nbytes) *nbytes = plane_bytes(ctx);
    return MI3PT_OK;
}

static int zero_textures(mi3pt_ctx *ctx)
{
    const size_t tex_bytes = plane_bytes(ctx);
    const size_t canvas_px = (size_t)ctx->width * ctx->height;
    if (tex_bytes) {
        // (the batch slots need no clearing: a launch writes every texel the ordered mean reads)
        HIP_TRY(hipMemsetAsync(ctx->d_radiance, 0, tex_bytes, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->d_accum, 0, tex_bytes, ctx->stream));
        if (ctx->d_moments) HIP_TRY(hipMemsetAsync(ctx->d_moments, 0, tex_bytes, ctx->stream));
    }
    if (canvas_px) {
        HIP_TRY(hipMemsetAsync(ctx->d_canvas, 0, canvas_px * 16, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->d_canvas8, 0, canvas_px * 4, ctx->stream));
    }
    ctx->history_held = false;        // (mi3pt_reset, mi3pt_resize: a held history goes with the mean)
    ctx->output_is_accum = false;
    ctx->last_radiance = ctx->d_radiance;
    ctx->main_dirty = true;
    ctx->accum_version++;
    ctx->presented_version = 0;       // the canvas was cleared
    ctx->want_present = false;
    return MI3PT_OK;
}

// mi3pt_resize / mi3pt_reset: no mask, every tile sampled (the queue has been launched under the old one)
static void drop_sample_mask(mi3pt_ctx *ctx)
{
    ctx->mask.clear();
    ctx->mask_epoch = 0;
    ctx->mask_sampled = 0;
}

// A context without textures: everything that lives from resize to resize is let go of (what that is: ImageState's members).
static void free_textures(mi3pt_ctx *ctx) { ctx->images() = ImageState(); }

extern "C" int mi3pt_resize(mi3pt_ctx *ctx, int width, int height)
{
    PT_GROUP(ctx, group_resize(ctx, width, height));
    if (int rc = require_idle(ctx)) return rc;
    if (width <= 0 || height <= 0 || width > 32768 || height > 32768)
        return pt_set_error(MI3PT_ERR_INVALID, "width/height must be in [1, 32768]");
    drop_sample_mask(ctx);
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    for (int k = 0; k < 2; k++) HIP_TRY(ctx_stream_sync(ctx, ctx->rt_stream[k]));
    // Transactional: the new images are allocated into a local and the context only changes once
    // every allocation has succeeded; a failure leaves it WITHOUT textures (width = height = 0,
    // every later submit / read reports "before resize") instead of with dangling pointers.
    free_textures(ctx);
    const int rank = ctx->next_rank, nranks = ctx->next_nranks, block_rows = ctx->next_block_rows;
    const int local_rows = mi3pt_tile_local_rows(height, rank, nranks, block_rows);
    const size_t tex_bytes = (size_t)local_rows * width * 16;
    const size_t canvas_px = (size_t)width * height;
    pt::Tile t;
    t.tex_w = width; t.tex_h = height; t.local_rows = local_rows; t.rank = rank; t.nranks = nranks; t.block_rows = block_rows;
    // per-wave counter slots: one per tile for the per-pixel kernels' grids, one per resident wave for the persistent kernels'
    // (whose grid is capped by the launch's JOBS -- tiles x frames -- and may exceed the tiles of one frame)
    const int ntiles_frame = pt::raytrace_grid_blocks(t);
    const int nblocks = ntiles_frame > 0 ? std::max(ntiles_frame, pt::PT_MAX_RESIDENT_WAVES) : 0;
    // two counter sets: overlapping raytrace kernels of consecutive frames use alternate halves
    const size_t cbytes = 2 * (size_t)(nblocks ? nblocks : 1) * pt::CNT_COUNT * sizeof(uint64_t);
    ImageState fresh;
    hipError_t e = fresh.d_radiance.alloc(tex_bytes);
    if (e == hipSuccess) e = fresh.d_accum_own.alloc(tex_bytes);
    if (e == hipSuccess) e = fresh.d_canvas.alloc(canvas_px * 16);
    if (e == hipSuccess) e = fresh.d_canvas8.alloc(canvas_px * 4);
    if (e == hipSuccess) e = fresh.d_block_counters.alloc(cbytes);
    if (e == hipSuccess && ctx->moments) e = fresh.d_moments.alloc(tex_bytes);
    if (e == hipSuccess) e = hipMemsetAsync(fresh.d_block_counters, 0, cbytes, ctx->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return pt_set_error(MI3PT_ERR_HIP, std::string("mi3pt_resize: allocating the textures failed: ") + hipGetErrorString(e));
    }
    fresh.width = width; fresh.height = height; fresh.local_rows = local_rows;
    fresh.d_accum = fresh.d_accum_own;
    fresh.nblocks = nblocks;
    ctx->rank = rank; ctx->nranks = nranks; ctx->block_rows = block_rows;
    ctx->images() = std::move(fresh);
    // batch depth: the limit for this tile split, capped so that the slot sets together take
    // at most a quarter of the memory that is free now (slots are allocated when first needed)
    recompute_batch_cap(ctx);
    return zero_textures(ctx);
}

extern "C" int mi3pt_reset(mi3pt_ctx *ctx)
{
    PT_GROUP(ctx, group_reset(ctx));
    if (int rc = require_idle(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "reset before resize");
    drop_sample_mask(ctx);          // a new accumulation starts whole
    return zero_textures(ctx);
}

extern "C" int mi3pt_set_uniforms(mi3pt_ctx *ctx, int pass, const void *bytes, size_t nbytes)
{
    PT_GROUP(ctx, group_set_uniforms(ctx, pass, bytes, nbytes));
    if (!ctx || !bytes) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    switch (pass) {
    case MI3PT_PASS_RAYTRACE:
        if (nbytes != sizeof ctx->u_rt) return pt_set_error(MI3PT_ERR_INVALID, "raytrace uniforms are 96 bytes");
        std::memcpy(ctx->u_rt, bytes, nbytes);
        return MI3PT_OK;
    case MI3PT_PASS_ACCUMULATE:
        if (nbytes != sizeof ctx->u_acc) return pt_set_error(MI3PT_ERR_INVALID, "accumulate uniforms are 16 bytes");
        std::memcpy(ctx->u_acc, bytes, nbytes);
        return MI3PT_OK;
    case MI3PT_PASS_FULLSCREEN:
        if (nbytes != sizeof ctx->u_fs) return pt_set_error(MI3PT_ERR_INVALID, "fullscreen uniforms are 24 bytes");
        std::memcpy(ctx->u_fs, bytes, nbytes);
        return MI3PT_OK;
    default:
        return pt_set_error(MI3PT_ERR_INVALID, "unknown pass");
    }
}

// LATEST presentation: the draw a queued frame asked for happens before the canvas is looked at.
static int settle_canvas(mi3pt_ctx *ctx)
{
    if (ctx->present_mode != MI3PT_PRESENT_LATEST || !ctx->want_present || ctx->width == 0 || ctx->partial()) return MI3PT_OK;
    ctx->want_present = false;
    return run_fullscreen(ctx, ctx->u_fs);
}

extern "C" int mi3pt_read_texture(mi3pt_ctx *ctx, int which, float *dst, size_t nfloats)
{
    PT_GROUP(ctx, group_read_texture(ctx, which, dst, nfloats));
    if (int rc = require_idle(ctx)) return rc;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "read before resize");
    const float4 *src;
    size_t need;
    switch (which) {
    case MI3PT_TEX_OUTPUT:
        src = ctx->output_is_accum ? ctx->d_accum : ctx->last_radiance;
        need = plane_texels(ctx) * 4;
        break;
    case MI3PT_TEX_ACCUMULATION:
        src = ctx->d_accum;
        need = plane_texels(ctx) * 4;
        break;
    case MI3PT_TEX_CANVAS:
        if (int rc = settle_canvas(ctx)) return rc;
        src = ctx->d_canvas;
        need = (size_t)ctx->height * ctx->width * 4;
        break;
    default:
        return pt_set_error(MI3PT_ERR_INVALID, "unknown texture");
    }
    if (nfloats != need) return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the texture");
    HIP_TRY(read_plane(ctx, src, need * 4, dst));
    return MI3PT_OK;
}

// Host -> device counterpart of mi3pt_read_texture for the accumulation image: restores a
// saved running mean (checkpoint / resume) or hands a gathered multi-GPU image to a 1-rank
// context for the fullscreen pass.
extern "C" int mi3pt_write_texture(mi3pt_ctx *ctx, int which, const float *src, size_t nfloats)
{
    PT_GROUP(ctx, group_write_texture(ctx, which, src, nfloats));
    if (int rc = require_idle(ctx)) return rc;
    if (!src) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "write before resize");
    if (which != MI3PT_TEX_ACCUMULATION && which != MI3PT_TEX_OUTPUT)
        return pt_set_error(MI3PT_ERR_INVALID, "only the accumulation / output image can be written");
    const size_t need = plane_bytes(ctx);
    if (nfloats != need / 4) return pt_set_error(MI3PT_ERR_INVALID, "source size does not match the texture");
    if (ctx->d_moments && need) HIP_TRY(hipMemsetAsync(ctx->d_moments, 0, need, ctx->stream));      // (a mean from outside: its spread is unknown)
    HIP_TRY(write_plane(ctx, ctx->d_accum, src, need));
    ctx->output_is_accum = true;      // like the copy-back of accumulate.ts:171-175
    ctx->main_dirty = true;
    ctx->accum_version++;
    return MI3PT_OK;
}

extern "C" int mi3pt_read_canvas_rgba8(mi3pt_ctx *ctx, uint8_t *dst, size_t nbytes)
{
    PT_GROUP(ctx, group_read_canvas(ctx, dst, nbytes));
    if (int rc = require_idle(ctx)) return rc;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "read before resize");
    const size_t need = (size_t)ctx->width * ctx->height * 4;
    if (nbytes != need) return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the canvas");
    if (int rc = settle_canvas(ctx)) return rc;
    HIP_TRY(read_plane(ctx, ctx->d_canvas8, need, dst));
    return MI3PT_OK;
}

extern "C" int mi3pt_accumulation_device_ptr(mi3pt_ctx *ctx, void **dev_ptr, size_t *nbytes)
{
    PT_GROUP(ctx, group_accumulation_ptr(ctx, dev_ptr, nbytes));
    if (!ctx || !dev_ptr) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "no textures before resize");
    if (int rc = require_idle(ctx)) return rc;
    return hand_out_plane(ctx, ctx->d_accum, dev_ptr, nbytes);
}

extern "C" int mi3pt_bind_accumulation(mi3pt_ctx *ctx, void *dev_ptr, size_t nbytes)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_bind_accumulation: a device group gathers into its own image (mi3pt_accumulation_device_ptr)"));
    if (int rc = require_idle(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "bind before resize");
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    ctx->main_dirty = true;
    ctx->accum_version++;
    // (another image becomes the mean: like a mean written from outside, its spread is unknown -- the moments start over)
    auto zero_moments = [&]() -> int {
        if (ctx->d_moments && plane_bytes(ctx)) HIP_TRY(hipMemsetAsync(ctx->d_moments, 0, plane_bytes(ctx), ctx->stream));
        return MI3PT_OK;
    };
    if (!dev_ptr) {
        ctx->d_accum = ctx->d_accum_own;
        return zero_moments();
    }
    if (nbytes != plane_bytes(ctx))
        return pt_set_error(MI3PT_ERR_INVALID, "external accumulation buffer must be local_rows*width*16 bytes");
    if (reinterpret_cast<uintptr_t>(dev_ptr) % 16)
        return pt_set_error(MI3PT_ERR_INVALID, "external accumulation buffer must be 16-byte aligned");
    ctx->d_accum = static_cast<float4 *>(dev_ptr);
    return zero_moments();
}

// ---- first-hit feature images (include/mi3pt.h: mi3pt_aov, mi3pt_render_aovs) ----
// Whether a first-hit pass walks the shipped walk's data (walk 13) -- after prepare_layout and prepare_cull: asked by mi3pt_render_aovs and
// by the probe of that walk, mi3pt_debug_intersect_shipped.
bool first_hit_walk_is_shipped(const mi3pt_ctx *ctx)
{
    return !ctx->env_sampling && !ctx->layout_active && ctx->cull_enabled && ctx->wide_enabled && ctx->cull_stack_ok &&
           ctx->cull_ok && !ctx->cull_dirty && ctx->wide_ok && ctx->cwide_ok && ctx->d_leaf_rank;
}

// Not require_idle: the queued sample frames stay queued and keep their batching.  The pass is enqueued on the context's stream;
// every path that frees or replaces a scene buffer waits for that stream first (replace_buffer, clone_scene, mi3pt_resize).
extern "C" int mi3pt_render_aovs(mi3pt_ctx *ctx, unsigned aov_mask)
{
    PT_GROUP(ctx, group_render_aovs(ctx, aov_mask));
    if (int rc = require_ctx(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_render_aovs before resize");
    if (aov_mask == 0 || (aov_mask >> MI3PT_AOV_COUNT)) return pt_set_error(MI3PT_ERR_INVALID, "aov_mask must be a non-empty OR of (1u << mi3pt_aov)");
    if (int rc = check_scene(ctx)) return rc;
    if (int rc = prepare_layout(ctx)) return rc;    // (what a raytrace submit does: no-ops unless the scene changed -- and then no frame is queued)
    if (int rc = prepare_cull(ctx)) return rc;
    const size_t tex_bytes = plane_bytes(ctx);
    for (int k = 0; k < MI3PT_AOV_COUNT; k++)
        if (((aov_mask >> k) & 1u) && !ctx->d_aov[k]) HIP_TRY(ctx->d_aov[k].alloc(tex_bytes));
    pt::AovLaunch A;
    A.scene = scene_refs(ctx);
    const uint8_t *u = ctx->u_rt;
    A.un.res_x = ldf(u, 0); A.un.res_y = ldf(u, 4); A.un.aspect = ldf(u, 8);
    A.un.frame = 0; A.un.max_bounces = 0; A.un.samples_per_frame = 0;          // (do not enter)
    for (int k = 0; k < 3; k++) { A.un.cam_pos[k] = ldf(u, 32 + 4 * k); A.un.cam_dir[k] = ldf(u, 48 + 4 * k); }
    A.un.fov = ldf(u, 60); A.un.focal_distance = 0.0f; A.un.aperture = 0.0f; A.un.env_intensity = 0.0f; A.un.env_rotation = 0.0f;
    A.tile = tile_of(ctx);
    for (int k = 0; k < MI3PT_AOV_COUNT; k++) A.image[k] = ((aov_mask >> k) & 1u) ? ctx->d_aov[k] : nullptr;
    // The walk.  Where `auto` would render sample frames with the shipped walk (variant 13: the scene admits distance culling and the
    // compressed wide packets, MI3PT_OPT_CULL / MI3PT_OPT_WIDE are on, no debug layout), the first-hit walk on that walk's data.
    // Else the reference's un-culled one on node / triangle packets with the prepared-reciprocal slab test (what the probe runs;
    // bit-identical on every tree the context accepts).  The debug packet layout renumbers the triangles its packets name: there
    // the walk on the uploaded records runs, so that the ids image holds uploaded indices.  One set of bits whichever runs.
    int walk = 3, stack_worst = ctx->walk_stack_worst;
    if (first_hit_walk_is_shipped(ctx)) { walk = 13; stack_worst = ctx->wide_stack_worst; }
    else if (ctx->layout_active) { walk = 1; A.scene.tris = ctx->d_tris.as<const float4>(); }
    if (tex_bytes) {
        if (ctx->timing) HIP_TRY(ctx->aov_timer.begin(ctx->stream));
        pt::launch_aovs(A, walk, stack_worst, ctx->leaf_min, ctx->stream);
        HIP_TRY(hipGetLastError());
        if (ctx->timing) HIP_TRY(ctx->aov_timer.end(ctx->stream));
    }
    for (int k = 0; k < MI3PT_AOV_COUNT; k++)
        if ((aov_mask >> k) & 1u) {
            ctx->aov_valid[k] = true;
            std::memcpy(ctx->aov_u[k], ctx->u_rt, sizeof ctx->u_rt);      // (the view this image belongs to: mi3pt_reproject's old view)
            ctx->aov_epoch[k] = ctx->upload_epoch;                       // (and the geometry: mi3pt_reproject_scene's previous one)
        }
    return MI3PT_OK;
}

static int aov_image(mi3pt_ctx *ctx, int which, const char *what)
{
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + " before resize");
    if (which < 0 || which >= MI3PT_AOV_COUNT) return pt_set_error(MI3PT_ERR_INVALID, "unknown feature image");
    if (!ctx->aov_valid[which] || !ctx->d_aov[which])
        return pt_set_error(MI3PT_ERR_STATE, std::string(what) + ": this image has not been rendered since the last resize (mi3pt_render_aovs)");
    return MI3PT_OK;
}

extern "C" int mi3pt_read_aov(mi3pt_ctx *ctx, int which, void *dst, size_t nbytes)
{
    PT_GROUP(ctx, group_read_aov(ctx, which, dst, nbytes));
    if (int rc = require_ctx(ctx)) return rc;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = aov_image(ctx, which, "mi3pt_read_aov")) return rc;
    if (nbytes != plane_bytes(ctx)) return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the image (rows x width x 16 bytes)");
    HIP_TRY(read_plane(ctx, ctx->d_aov[which], nbytes, dst));
    return MI3PT_OK;
}

extern "C" int mi3pt_aov_device_ptr(mi3pt_ctx *ctx, int which, void **dev_ptr, size_t *nbytes)
{
    PT_GROUP(ctx, group_aov_ptr(ctx, which, dev_ptr, nbytes));
    if (int rc = require_ctx(ctx)) return rc;
    if (!dev_ptr) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = aov_image(ctx, which, "mi3pt_aov_device_ptr")) return rc;
    return hand_out_plane(ctx, ctx->d_aov[which], dev_ptr, nbytes);
}

// ---- the feature-guided a-trous de-noise of the running mean (include/mi3pt.h: mi3pt_denoise_guided; pt_guided.hip) ----
// 1 / (sigma * sigma) in fp32; a sigma of 0 switches its term off
static float guided_inv(float sigma) { return sigma == 0.0f ? 0.0f : 1.0f / (sigma * sigma); }

extern "C" int mi3pt_denoise_guided(mi3pt_ctx *ctx, const mi3pt_guided_params *params)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_denoise_guided: not built for a device group (the members would have to exchange a 32-row halo)"));
    if (!ctx || !params) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (params->levels < 1 || params->levels > 5) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_denoise_guided: levels must be 1 .. 5");
    for (float sigma : { params->sigma_color, params->sigma_normal, params->sigma_albedo, params->sigma_plane })
        if (!(sigma >= 0.0f) || std::isinf(sigma)) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_denoise_guided: every sigma must be finite and >= 0");
    // (a context that never opted into the moments image answers as it always did: the variance bit is unknown to it)
    if (params->flags & ~(MI3PT_GUIDED_PRESENT | (ctx->moments_opted ? MI3PT_GUIDED_VARIANCE | MI3PT_GUIDED_YOUNG : 0u)))
        return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_denoise_guided: unknown flag bits (MI3PT_GUIDED_VARIANCE, MI3PT_GUIDED_YOUNG: only on a context that has enabled the moments image, mi3pt_set_moments)");
    const bool by_variance = (params->flags & MI3PT_GUIDED_VARIANCE) != 0, young = (params->flags & MI3PT_GUIDED_YOUNG) != 0;
    if (young && !by_variance)
        return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_denoise_guided: MI3PT_GUIDED_YOUNG only together with MI3PT_GUIDED_VARIANCE (it changes that mode's initial variance)");
    if (int rc = require_ctx(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_denoise_guided before resize");
    if (ctx->partial())
        return pt_set_error(MI3PT_ERR_STATE, "mi3pt_denoise_guided needs the whole image: not built for a rank of a tile split (a 32-row halo would have to be exchanged)");
    for (int k = 0; k < MI3PT_AOV_COUNT; k++)
        if (!ctx->aov_valid[k] || !ctx->d_aov[k])
            return pt_set_error(MI3PT_ERR_STATE, "mi3pt_denoise_guided: the four feature images have not all been rendered since the last resize (mi3pt_render_aovs)");
    if (by_variance && !ctx->d_moments)
        return pt_set_error(MI3PT_ERR_STATE, "mi3pt_denoise_guided: MI3PT_GUIDED_VARIANCE needs the moments image (mi3pt_set_moments(ctx, 1) before the frames are accumulated)");
    if (int rc = flush_pending(ctx)) return rc;      // the mean a read-back would return now: the accumulate passes run on this stream
    const size_t texels = plane_texels(ctx);
    for (DevBuf<float4> *p : { &ctx->d_guided[0], &ctx->d_guided[1], &ctx->d_guided_nh })
        if (!*p) HIP_TRY(p->alloc(plane_bytes(ctx)));
    if (by_variance)
        for (DevBuf<float> &p : ctx->d_guided_var)
            if (!p) HIP_TRY(p.alloc(texels * 4));
    pt::GuidedLaunch G;
    G.normal_hit = ctx->d_guided_nh; G.position = ctx->d_aov[MI3PT_AOV_POSITION]; G.albedo = ctx->d_aov[MI3PT_AOV_ALBEDO];
    G.width = ctx->width; G.rows = ctx->local_rows;
    G.inv_color = guided_inv(params->sigma_color); G.inv_normal = guided_inv(params->sigma_normal);
    G.inv_albedo = guided_inv(params->sigma_albedo); G.inv_plane = guided_inv(params->sigma_plane);
    const bool despike = ctx->guided_despike;
    if (despike) {
        if (!ctx->d_guided_despike) HIP_TRY(ctx->d_guided_despike.alloc(plane_bytes(ctx)));
        constexpr size_t count_bytes = (size_t)pt::DESPIKE_SLOTS * pt::DESPIKE_SLOT_WORDS * 4;
        if (!ctx->d_guided_despike_count) HIP_TRY(ctx->d_guided_despike_count.alloc(count_bytes));
        HIP_TRY(hipMemsetAsync(ctx->d_guided_despike_count, 0, count_bytes, ctx->stream));      // (outside the timed span: the pre-pass is one launch)
    }
    ctx->guided_despiked = false;
    if (ctx->timing) HIP_TRY(ctx->guided_timer.begin(ctx->stream));
    pt::launch_guided_pack(ctx->d_aov[MI3PT_AOV_NORMAL], ctx->d_aov[MI3PT_AOV_IDS], ctx->d_guided_nh, texels, ctx->stream);
    const float4 *src = ctx->d_accum;
    const float *var = nullptr;
    float *scale = nullptr;
    if (despike) {
        // the pre-pass: c' in the accumulation image's place from here on; s into the variance image var_0 does not use (level 0 writes
        // it after the var_0 kernel has read it)
        if (by_variance) scale = ctx->d_guided_var[0];
        pt::launch_guided_despike(src, ctx->d_aov[MI3PT_AOV_IDS], ctx->d_guided_despike, scale, ctx->d_guided_despike_count, ctx->width,
                                  ctx->local_rows, ctx->stream);
        src = ctx->d_guided_despike;
    }
    if (by_variance) {
        // var_0 into the image level 0 does not write; level i then reads image (i + 1) & 1 and writes image i & 1
        if (young)
            pt::launch_guided_variance_young(G, src, ctx->d_moments, ctx->d_guided_var[1], scale, ctx->stream);
        else
            pt::launch_guided_variance(ctx->d_moments, ctx->d_guided_nh, ctx->d_guided_var[1], scale, ctx->width, ctx->local_rows, ctx->stream);
        var = ctx->d_guided_var[1];
    }
    for (int level = 0; level < params->levels; level++) {
        float4 *dst = ctx->d_guided[level & 1];
        if (by_variance) {
            float *var_dst = ctx->d_guided_var[level & 1];
            pt::launch_guided_level_variance(G, src, dst, var, var_dst, level, params->sigma_color, ctx->stream);
            var = var_dst;
        } else {
            pt::launch_guided_level(G, src, dst, level, ctx->stream);
        }
        src = dst;
    }
    HIP_TRY(hipGetLastError());
    if (ctx->timing) HIP_TRY(ctx->guided_timer.end(ctx->stream));
    ctx->guided_result = src;
    ctx->guided_var_result = var;
    ctx->guided_despiked = despike;
    if (params->flags & MI3PT_GUIDED_PRESENT) {
        // the fullscreen pass on the filtered image, with the pass's uniforms as they are and its own de-noiser off.  The canvas then shows
        // no state of the running mean: the next fullscreen submit draws again whatever it showed before, and a draw still owed to queued
        // frames (MI3PT_PRESENT_LATEST) is dropped -- those frames are in the mean this call filtered.
        pt::FsUniforms fs;
        const uint8_t *u_fs = ctx->u_fs;
        fs.res_x = ldf(u_fs, 0); fs.res_y = ldf(u_fs, 4); fs.aspect = ldf(u_fs, 8);
        fs.scaling = ldf(u_fs, 12); fs.denoise = 0u; fs.tonemapping = ldu(u_fs, 20);
        pt::launch_fullscreen(fs, src, ctx->width, ctx->height, ctx->width, ctx->height, ctx->d_fs_taps, true, ctx->d_canvas, ctx->d_canvas8, ctx->stream);
        HIP_TRY(hipGetLastError());
        ctx->presented_version = 0;
        ctx->want_present = false;
    }
    return MI3PT_OK;
}

static int guided_image(mi3pt_ctx *ctx, const char *what)
{
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + " before resize");
    if (!ctx->guided_result) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + ": nothing has been filtered since the last resize (mi3pt_denoise_guided)");
    return MI3PT_OK;
}

extern "C" int mi3pt_read_guided(mi3pt_ctx *ctx, void *dst, size_t nbytes)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_read_guided: mi3pt_denoise_guided is not built for a device group"));
    if (int rc = require_ctx(ctx)) return rc;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = guided_image(ctx, "mi3pt_read_guided")) return rc;
    if (nbytes != plane_bytes(ctx)) return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the image (rows x width x 16 bytes)");
    HIP_TRY(read_plane(ctx, ctx->guided_result, nbytes, dst));
    return MI3PT_OK;
}

extern "C" int mi3pt_guided_device_ptr(mi3pt_ctx *ctx, void **dev_ptr, size_t *nbytes)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_guided_device_ptr: mi3pt_denoise_guided is not built for a device group"));
    if (int rc = require_ctx(ctx)) return rc;
    if (!dev_ptr) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = guided_image(ctx, "mi3pt_guided_device_ptr")) return rc;
    return hand_out_plane(ctx, ctx->guided_result, dev_ptr, nbytes);
}

extern "C" int mi3pt_read_guided_variance(mi3pt_ctx *ctx, float *dst, size_t nfloats)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_read_guided_variance: mi3pt_denoise_guided is not built for a device group"));
    if (int rc = require_ctx(ctx)) return rc;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = guided_image(ctx, "mi3pt_read_guided_variance")) return rc;
    if (!ctx->guided_var_result) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_read_guided_variance: the last filter ran without MI3PT_GUIDED_VARIANCE");
    if (nfloats != plane_texels(ctx)) return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the image (rows x width floats)");
    HIP_TRY(read_plane(ctx, ctx->guided_var_result, nfloats * 4, dst));
    return MI3PT_OK;
}

// ---- the firefly pre-pass of the guided de-noise (include/mi3pt.h: mi3pt_set_guided_despike; pt_guided.hip: k_guided_despike) ----
extern "C" int mi3pt_set_guided_despike(mi3pt_ctx *ctx, int enabled)
{
    PT_GROUP_ALL(ctx, false, mi3pt_set_guided_despike(m, enabled));
    if (int rc = require_ctx(ctx)) return rc;
    ctx->guided_despike = enabled != 0;      // (host state alone: read by the next mi3pt_denoise_guided, which allocates what it needs)
    return MI3PT_OK;
}

extern "C" int mi3pt_read_guided_despiked(mi3pt_ctx *ctx, uint32_t *texels)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_read_guided_despiked: mi3pt_denoise_guided is not built for a device group"));
    if (int rc = require_ctx(ctx)) return rc;
    if (!texels) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = guided_image(ctx, "mi3pt_read_guided_despiked")) return rc;
    if (!ctx->guided_despiked || !ctx->d_guided_despike_count)
        return pt_set_error(MI3PT_ERR_STATE, "mi3pt_read_guided_despiked: the last filter ran without the pre-pass (mi3pt_set_guided_despike)");
    std::vector<uint32_t> slots((size_t)pt::DESPIKE_SLOTS * pt::DESPIKE_SLOT_WORDS);
    HIP_TRY(read_plane(ctx, ctx->d_guided_despike_count, slots.size() * 4, slots.data()));
    uint32_t sum = 0;
    for (uint32_t k = 0; k < pt::DESPIKE_SLOTS; k++) sum += slots[(size_t)k * pt::DESPIKE_SLOT_WORDS];
    *texels = sum;
    return MI3PT_OK;
}

// ---- the moments image (include/mi3pt.h: mi3pt_set_moments; pt_kernels.hip: k_accumulate_frames<true>) ----
extern "C" int mi3pt_set_moments(mi3pt_ctx *ctx, int enabled)
{
    PT_GROUP(ctx, group_set_moments(ctx, enabled));
    if (int rc = require_idle(ctx)) return rc;
    const bool on = enabled != 0;
    if (on == ctx->moments) return MI3PT_OK;
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));      // (the accumulate passes in flight read and write the image this frees)
    if (!on) {
        ctx->d_moments.reset();
        for (DevBuf<float4> &p : ctx->d_hold) p.reset();      // (a held history is a mean WITH its moments)
        ctx->history_held = false;
        ctx->moments = false;
        ctx->by_count = false;      // (the count is the image's n: the mode goes with it)
        return MI3PT_OK;
    }
    if (ctx->width != 0) {
        const size_t tex_bytes = plane_bytes(ctx);
        DevBuf<float4> image;
        HIP_TRY(image.alloc(tex_bytes));
        if (tex_bytes) {
            const hipError_t e = hipMemsetAsync(image, 0, tex_bytes, ctx->stream);
            if (e != hipSuccess) {          // (nothing half enabled: the launches key on the pointer)
                (void)hipGetLastError();
                return pt_set_error(MI3PT_ERR_HIP, std::string("mi3pt_set_moments: clearing the image failed: ") + hipGetErrorString(e));
            }
        }
        ctx->d_moments = std::move(image);
        ctx->main_dirty = true;
    }
    ctx->moments = ctx->moments_opted = true;      // (before mi3pt_resize: the image comes with the textures)
    return MI3PT_OK;
}

static int moments_image(mi3pt_ctx *ctx, const char *what)
{
    if (!ctx->moments) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + ": the moments image is not enabled (mi3pt_set_moments)");
    if (ctx->width == 0 || !ctx->d_moments) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + " before resize");
    return MI3PT_OK;
}

extern "C" int mi3pt_read_moments(mi3pt_ctx *ctx, void *dst, size_t nbytes)
{
    PT_GROUP(ctx, group_read_moments(ctx, dst, nbytes));
    if (int rc = require_idle(ctx)) return rc;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = moments_image(ctx, "mi3pt_read_moments")) return rc;
    if (nbytes != plane_bytes(ctx)) return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the image (rows x width x 16 bytes)");
    HIP_TRY(read_plane(ctx, ctx->d_moments, nbytes, dst));
    return MI3PT_OK;
}

extern "C" int mi3pt_write_moments(mi3pt_ctx *ctx, const void *src, size_t nbytes)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_write_moments: a device group keeps its members' moments images (write each member's rows: mi3pt_group_member)"));
    if (int rc = require_idle(ctx)) return rc;
    if (!src) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = moments_image(ctx, "mi3pt_write_moments")) return rc;
    if (nbytes != plane_bytes(ctx)) return pt_set_error(MI3PT_ERR_INVALID, "source size does not match the image (rows x width x 16 bytes)");
    if (nbytes == 0) return MI3PT_OK;
    HIP_TRY(write_plane(ctx, ctx->d_moments, src, nbytes));
    ctx->main_dirty = true;
    return MI3PT_OK;
}

extern "C" int mi3pt_moments_device_ptr(mi3pt_ctx *ctx, void **dev_ptr, size_t *nbytes)
{
    PT_GROUP(ctx, group_moments_ptr(ctx, dev_ptr, nbytes));
    if (int rc = require_idle(ctx)) return rc;
    if (!dev_ptr) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = moments_image(ctx, "mi3pt_moments_device_ptr")) return rc;
    return hand_out_plane(ctx, ctx->d_moments, dev_ptr, nbytes);
}

// ---- the mean by count and the reprojection (include/mi3pt.h: mi3pt_set_mean_by_count, mi3pt_reproject; pt_accum.h, pt_reproject.hip) ----
extern "C" int mi3pt_set_mean_by_count(mi3pt_ctx *ctx, int enabled)
{
    PT_GROUP_ALL(ctx, false, mi3pt_set_mean_by_count(m, enabled));
    if (int rc = require_idle(ctx)) return rc;      // the frames queued so far were submitted under the old law
    if (enabled && !ctx->moments)
        return pt_set_error(MI3PT_ERR_STATE, "mi3pt_set_mean_by_count needs the moments image: the count is its n (mi3pt_set_moments(ctx, 1) first)");
    ctx->by_count = enabled != 0;
    return MI3PT_OK;
}

// what mi3pt_reproject and mi3pt_reproject_scene share: the argument checks, the state checks and steps 1 - 7 of the header.  scene: the
// kernel that follows a triangle back to the kept geometry (k_reproject_scene) takes k_reproject's place in step 5.
struct ReprojectCall {
    const char *who;
    float plane_tolerance, normal_cos_min;
    int max_history, max_history_moved;
    unsigned flags;
    bool scene;
};

static int reproject_run(mi3pt_ctx *ctx, const ReprojectCall &c)
{
    const std::string who = c.who;
    if (!(c.plane_tolerance >= 0.0f) || std::isinf(c.plane_tolerance))
        return pt_set_error(MI3PT_ERR_INVALID, who + ": plane_tolerance must be finite and >= 0");
    if (!(c.normal_cos_min >= -1.0f && c.normal_cos_min <= 1.0f))
        return pt_set_error(MI3PT_ERR_INVALID, who + ": normal_cos_min must lie in [-1, 1]");
    if (c.max_history < 1 || c.max_history > (1 << 24)) return pt_set_error(MI3PT_ERR_INVALID, who + ": max_history must be 1 .. 2^24");
    if (c.scene && (c.max_history_moved < 1 || c.max_history_moved > (1 << 24)))
        return pt_set_error(MI3PT_ERR_INVALID, who + ": max_history_moved must be 1 .. 2^24");
    if (c.flags) return pt_set_error(MI3PT_ERR_INVALID, who + ": unknown flag bits");
    if (int rc = require_ctx(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, who + " before resize");
    if (!ctx->moments || !ctx->d_moments || !ctx->by_count)
        return pt_set_error(MI3PT_ERR_STATE, who + " needs the moments image and the mean by count (mi3pt_set_moments, mi3pt_set_mean_by_count)");
    if (ctx->partial())
        return pt_set_error(MI3PT_ERR_STATE, who + ": not built for a rank of a tile split (a tap crosses the ranks' rows; no halo exchange)");
    static const int old_set[3] = { MI3PT_AOV_POSITION, MI3PT_AOV_NORMAL, MI3PT_AOV_IDS };
    const uint8_t *u0 = ctx->aov_u[MI3PT_AOV_POSITION];
    for (int k : old_set) {
        if (!ctx->aov_valid[k] || !ctx->d_aov[k])
            return pt_set_error(MI3PT_ERR_STATE, who + ": the POSITION, NORMAL and IDS images of the old view have not been rendered since the last resize (mi3pt_render_aovs)");
        // (resolution and aspect; camera position, direction and fov: what the first hit depends on)
        if (std::memcmp(ctx->aov_u[k], u0, 12) || std::memcmp(ctx->aov_u[k] + 32, u0 + 32, 32))
            return pt_set_error(MI3PT_ERR_STATE, who + ": the POSITION, NORMAL and IDS images were rendered from different views");
    }
    if (std::memcmp(ctx->u_rt, u0, 8))
        return pt_set_error(MI3PT_ERR_STATE, who + ": the new view's resolution differs from the old view's");
    if (c.scene) {
        if (!ctx->geometry_kept) return pt_set_error(MI3PT_ERR_STATE, who + ": no previous geometry is kept (mi3pt_keep_geometry)");
        if (!ctx->d_tris || ctx->ntris != ctx->ntris_kept)
            return pt_set_error(MI3PT_ERR_STATE, who + ": the kept geometry and the current one differ in their number of triangles");
        for (int k : old_set)
            if (ctx->aov_epoch[k] != ctx->kept_epoch)
                return pt_set_error(MI3PT_ERR_STATE, who + ": the POSITION, NORMAL and IDS images were not rendered from the kept geometry (an upload lies between them and mi3pt_keep_geometry)");
    }
    if (int rc = flush_pending(ctx)) return rc;      // every frame submitted so far belongs to the old view's mean
    ctx->history_held = false;                       // (what was held belongs to the view before this one)
    pt::ReprojectSceneLaunch S;
    pt::ReprojectLaunch &R = S.view;
    if (int rc = mi3pt_host_view_frame(u0, MI3PT_RAYTRACE_UNIFORMS_SIZE, R.f0)) return rc;
    R.res0_x = ldf(u0, 0); R.res0_y = ldf(u0, 4);
    const size_t tex_bytes = plane_bytes(ctx);
    for (int k : old_set)
        if (!ctx->d_aov_prev[k]) HIP_TRY(ctx->d_aov_prev[k].alloc(tex_bytes));
    for (DevBuf<float4> &p : ctx->d_reproject)
        if (!p) HIP_TRY(p.alloc(tex_bytes));
    // the old features become the previous set; the new view's are rendered into the images the set before it held
    for (int k : old_set) std::swap(ctx->d_aov[k], ctx->d_aov_prev[k]);
    if (int rc = mi3pt_render_aovs(ctx, (1u << MI3PT_AOV_COUNT) - 1u)) {
        for (int k : old_set) std::swap(ctx->d_aov[k], ctx->d_aov_prev[k]);      // (nothing was rendered: the old view's images stand)
        return rc;
    }
    const pt::AccUniforms acc = acc_uniforms(ctx);
    R.accum = ctx->d_accum; R.moments = ctx->d_moments;
    R.accum_out = ctx->d_reproject[0]; R.moments_out = ctx->d_reproject[1];
    R.pos1 = ctx->d_aov[MI3PT_AOV_POSITION]; R.nrm1 = ctx->d_aov[MI3PT_AOV_NORMAL]; R.ids1 = ctx->d_aov[MI3PT_AOV_IDS];
    R.pos0 = ctx->d_aov_prev[MI3PT_AOV_POSITION]; R.nrm0 = ctx->d_aov_prev[MI3PT_AOV_NORMAL]; R.ids0 = ctx->d_aov_prev[MI3PT_AOV_IDS];
    R.width = ctx->width; R.rows = ctx->local_rows;
    R.res_w = acc.res_w; R.res_h = acc.res_h;
    R.plane_tolerance = c.plane_tolerance; R.normal_cos_min = c.normal_cos_min; R.max_history = (float)c.max_history;
    R.store_f16 = ctx->storage == MI3PT_STORAGE_F16;
    if (ctx->timing) HIP_TRY(ctx->reproject_timer.begin(ctx->stream));
    if (c.scene) {
        // the records in upload order, which IDS indexes: the current ones, and the kept ones (the current ones until an upload handed them over)
        S.tris1 = ctx->d_tris.as<const float4>();
        S.tris0 = (ctx->d_tris_kept ? ctx->d_tris_kept : ctx->d_tris).as<const float4>();
        S.ntris = (int32_t)ctx->ntris;
        S.max_history_moved = (float)c.max_history_moved;
        pt::launch_reproject_scene(S, ctx->stream);
    } else {
        pt::launch_reproject(R, ctx->stream);
    }
    HIP_TRY(hipGetLastError());
    // the scratch pair takes the images' place: the context's own by a swap of pointers, a bound accumulation image by a copy on the stream
    std::swap(ctx->d_moments, ctx->d_reproject[1]);
    if (ctx->d_accum == ctx->d_accum_own) {
        std::swap(ctx->d_accum_own, ctx->d_reproject[0]);
        ctx->d_accum = ctx->d_accum_own;
    } else if (tex_bytes) {
        HIP_TRY(hipMemcpyAsync(ctx->d_accum, ctx->d_reproject[0], tex_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (ctx->timing) HIP_TRY(ctx->reproject_timer.end(ctx->stream));
    drop_sample_mask(ctx);          // a new view starts whole
    ctx->main_dirty = true;
    ctx->accum_version++;
    return MI3PT_OK;
}

extern "C" int mi3pt_reproject(mi3pt_ctx *ctx, const mi3pt_reproject_params *params)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_reproject: not built for a device group (a tap crosses the members' rows; no halo exchange)"));
    if (!ctx || !params) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    return reproject_run(ctx, { "mi3pt_reproject", params->plane_tolerance, params->normal_cos_min, params->max_history, 1, params->flags, false });
}

// ---- the previous geometry and the reprojection across a scene change (include/mi3pt.h: mi3pt_keep_geometry, mi3pt_reproject_scene) ----
extern "C" int mi3pt_reproject_scene(mi3pt_ctx *ctx, const mi3pt_reproject_scene_params *params)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_reproject_scene: not built for a device group (a tap crosses the members' rows; no halo exchange)"));
    if (!ctx || !params) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    return reproject_run(ctx, { "mi3pt_reproject_scene", params->plane_tolerance, params->normal_cos_min, params->max_history,
                                params->max_history_moved, params->flags, true });
}

// ---- the held history and its validated merge (include/mi3pt.h: mi3pt_hold_history, mi3pt_merge_history; pt_history.hip) ----
static int history_state(mi3pt_ctx *ctx, const std::string &who)
{
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, who + " before resize");
    if (!ctx->moments || !ctx->d_moments || !ctx->by_count)
        return pt_set_error(MI3PT_ERR_STATE, who + " needs the moments image and the mean by count (mi3pt_set_moments, mi3pt_set_mean_by_count)");
    if (ctx->partial())
        return pt_set_error(MI3PT_ERR_STATE, who + ": not built for a rank of a tile split (a window crosses the ranks' rows; no halo exchange)");
    return MI3PT_OK;
}

extern "C" int mi3pt_hold_history(mi3pt_ctx *ctx)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_hold_history: not built for a device group (a window crosses the members' rows; no halo exchange)"));
    if (int rc = require_ctx(ctx)) return rc;
    if (int rc = history_state(ctx, "mi3pt_hold_history")) return rc;
    if (int rc = flush_pending(ctx)) return rc;      // every frame submitted so far belongs to the history that is held
    const size_t tex_bytes = plane_bytes(ctx);
    for (DevBuf<float4> &p : ctx->d_hold)
        if (!p) HIP_TRY(p.alloc(tex_bytes));
    ctx->history_held = false;        // (a failure below leaves nothing half held)
    // the images become the held pair: the context's own by a swap of pointers, a bound accumulation image by a copy on the stream
    std::swap(ctx->d_moments, ctx->d_hold[1]);
    if (ctx->d_accum == ctx->d_accum_own) {
        std::swap(ctx->d_accum_own, ctx->d_hold[0]);
        ctx->d_accum = ctx->d_accum_own;
    } else if (tex_bytes) {
        HIP_TRY(hipMemcpyAsync(ctx->d_hold[0], ctx->d_accum, tex_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    ctx->main_dirty = true;
    ctx->accum_version++;
    if (tex_bytes) {                  // the live pair as mi3pt_reset leaves it
        HIP_TRY(hipMemsetAsync(ctx->d_accum, 0, tex_bytes, ctx->stream));
        HIP_TRY(hipMemsetAsync(ctx->d_moments, 0, tex_bytes, ctx->stream));
    }
    ctx->history_held = true;
    return MI3PT_OK;
}

extern "C" int mi3pt_merge_history(mi3pt_ctx *ctx, const mi3pt_history_params *params)
{
    PT_GROUP(ctx, group_unsupported("mi3pt_merge_history: not built for a device group (a window crosses the members' rows; no halo exchange)"));
    if (!ctx || !params) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (params->radius < 0 || params->radius > 3) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_merge_history: radius must be 0 .. 3");
    if (!(params->z_keep >= 0.0f) || std::isinf(params->z_keep))
        return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_merge_history: z_keep must be finite and >= 0");
    if (!(params->z_drop > params->z_keep) || std::isinf(params->z_drop))
        return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_merge_history: z_drop must be finite and above z_keep");
    if (params->flags) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_merge_history: unknown flag bits");
    if (int rc = require_ctx(ctx)) return rc;
    if (int rc = history_state(ctx, "mi3pt_merge_history")) return rc;
    if (!ctx->history_held || !ctx->d_hold[0] || !ctx->d_hold[1])
        return pt_set_error(MI3PT_ERR_STATE, "mi3pt_merge_history: no history is held (mi3pt_hold_history; a reset, a resize and a reprojection drop it)");
    if (int rc = flush_pending(ctx)) return rc;      // every frame submitted so far is a fresh sample of the test
    const size_t tex_bytes = plane_bytes(ctx);
    for (DevBuf<float4> &p : ctx->d_reproject)
        if (!p) HIP_TRY(p.alloc(tex_bytes));
    const pt::AccUniforms acc = acc_uniforms(ctx);
    pt::HistoryLaunch L;
    L.accum = ctx->d_accum; L.moments = ctx->d_moments;
    L.accum_held = ctx->d_hold[0]; L.moments_held = ctx->d_hold[1];
    L.accum_out = ctx->d_reproject[0]; L.moments_out = ctx->d_reproject[1];
    L.width = ctx->width; L.rows = ctx->local_rows;
    L.res_w = acc.res_w; L.res_h = acc.res_h;
    L.radius = params->radius; L.z_keep = params->z_keep; L.z_drop = params->z_drop;
    L.store_f16 = ctx->storage == MI3PT_STORAGE_F16;
    if (ctx->timing) HIP_TRY(ctx->history_timer.begin(ctx->stream));
    pt::launch_history(L, ctx->stream);
    HIP_TRY(hipGetLastError());
    // the scratch pair takes the images' place: the context's own by a swap of pointers, a bound accumulation image by a copy on the stream
    std::swap(ctx->d_moments, ctx->d_reproject[1]);
    if (ctx->d_accum == ctx->d_accum_own) {
        std::swap(ctx->d_accum_own, ctx->d_reproject[0]);
        ctx->d_accum = ctx->d_accum_own;
    } else if (tex_bytes) {
        HIP_TRY(hipMemcpyAsync(ctx->d_accum, ctx->d_reproject[0], tex_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (ctx->timing) HIP_TRY(ctx->history_timer.end(ctx->stream));
    ctx->history_held = false;
    ctx->main_dirty = true;
    ctx->accum_version++;
    return MI3PT_OK;
}

// ---- the per-tile error estimate of the running mean (include/mi3pt.h: mi3pt_estimate_convergence; pt_converge.hip) ----

extern "C" int mi3pt_estimate_convergence(mi3pt_ctx *ctx, float threshold, int min_frames)
{
    PT_GROUP_ALL(ctx, false, mi3pt_estimate_convergence(m, threshold, min_frames));
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    if (!(threshold >= 0.0f) || std::isinf(threshold)) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_estimate_convergence: the threshold must be finite and >= 0");
    if (min_frames < 0 || min_frames > (1 << 24)) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_estimate_convergence: min_frames must be 0 .. 2^24");
    if (int rc = require_ctx(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_estimate_convergence before resize");
    if (!ctx->moments || !ctx->d_moments)
        return pt_set_error(MI3PT_ERR_STATE, "mi3pt_estimate_convergence needs the moments image (mi3pt_set_moments(ctx, 1) before the frames are accumulated)");
    if (int rc = flush_pending(ctx)) return rc;      // every frame submitted so far: the accumulate passes run on this stream
    const size_t ntiles = conv_tiles_x(ctx) * conv_tiles_y(ctx);
    if (!ctx->d_conv_tiles) HIP_TRY(ctx->d_conv_tiles.alloc(ntiles * 16));
    if (!ctx->d_conv_parts) HIP_TRY(ctx->d_conv_parts.alloc((size_t)pt::converge_blocks(ctx->width, ctx->local_rows) * sizeof(pt::ConvergePart)));
    if (!ctx->d_conv_summary) HIP_TRY(ctx->d_conv_summary.alloc(sizeof(pt::ConvergeSummary)));
    if (!ctx->h_conv_summary) HIP_TRY(ctx->h_conv_summary.alloc(sizeof(pt::ConvergeSummary)));
    if (!ctx->conv_done) HIP_TRY(hipEventCreateWithFlags(ctx->conv_done.put(), hipEventDisableTiming));
    const float t2 = (threshold * threshold) * 3.0f;
    if (ctx->timing) HIP_TRY(ctx->conv_timer.begin(ctx->stream));
    pt::launch_converge(ctx->d_accum, ctx->d_moments, ctx->d_conv_tiles, ctx->d_conv_parts, ctx->d_conv_summary, ctx->width, ctx->local_rows, t2,
                        (float)min_frames, ctx->stream);
    HIP_TRY(hipGetLastError());
    if (ctx->timing) HIP_TRY(ctx->conv_timer.end(ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_conv_summary, ctx->d_conv_summary, sizeof(pt::ConvergeSummary), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->conv_done, ctx->stream));
    ctx->conv_valid = true;
    ctx->conv_threshold = threshold;
    ctx->conv_min_frames = min_frames;
    return MI3PT_OK;
}

// what both reads start with: the state, then the wait for the estimate's event -- not for the stream, and the queue is not launched
static int conv_wait(mi3pt_ctx *ctx, const char *what)
{
    if (int rc = require_ctx(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + " before resize");
    if (!ctx->conv_valid) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + ": nothing has been estimated since the last resize (mi3pt_estimate_convergence)");
    HIP_TRY(ctx_event_sync(ctx, ctx->conv_done, "convergence estimate"));
    return MI3PT_OK;
}

extern "C" int mi3pt_read_convergence(mi3pt_ctx *ctx, mi3pt_convergence *out)
{
    PT_GROUP(ctx, group_read_convergence(ctx, out));
    if (!ctx || !out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = conv_wait(ctx, "mi3pt_read_convergence")) return rc;
    const pt::ConvergeSummary s = *ctx->h_conv_summary;
    auto as_float = [](uint32_t bits) { float f; std::memcpy(&f, &bits, 4); return f; };
    out->tiles = s.tiles;
    out->tiles_above = s.above;
    out->tiles_young = s.young;
    out->tiles_nonfinite = s.nonfinite;
    out->texels = s.texels;
    out->worst_tile = as_float(s.worst_tile);
    out->worst_texel = as_float(s.worst_texel);
    out->n_min = out->tiles ? as_float(~s.n_min_inv) : 0.0f;
    out->threshold = ctx->conv_threshold;
    return MI3PT_OK;
}

extern "C" int mi3pt_read_convergence_tiles(mi3pt_ctx *ctx, float *dst, size_t nfloats)
{
    PT_GROUP(ctx, group_read_convergence_tiles(ctx, dst, nfloats));
    if (!ctx || !dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = require_ctx(ctx)) return rc;
    if (ctx->width != 0 && ctx->conv_valid && nfloats != conv_tiles_x(ctx) * conv_tiles_y(ctx) * 4)
        return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the tile map (ceil(rows / 8) x ceil(width / 8) x 4 floats)");
    if (int rc = conv_wait(ctx, "mi3pt_read_convergence_tiles")) return rc;
    if (nfloats == 0) return MI3PT_OK;
    // the map is the estimate's until the next estimate: copied beside the context's stream, which may be busy with later frames
    if (!ctx->conv_read_stream) HIP_TRY(hipStreamCreateWithFlags(ctx->conv_read_stream.put(), hipStreamNonBlocking));
    HIP_TRY(hipMemcpyAsync(dst, ctx->d_conv_tiles, nfloats * 4, hipMemcpyDeviceToHost, ctx->conv_read_stream));
    HIP_TRY(hipStreamSynchronize(ctx->conv_read_stream));
    return MI3PT_OK;
}

// ---- adaptive sampling: the per-tile sample mask (include/mi3pt.h: mi3pt_set_sample_mask; pt_host_adapt.cpp, pt_accumulate_tiles.hip) ----
extern "C" int mi3pt_set_sample_mask(mi3pt_ctx *ctx, const uint8_t *tiles, size_t ntiles)
{
    PT_GROUP(ctx, group_set_sample_mask(ctx, tiles, ntiles));
    if (int rc = require_ctx(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_set_sample_mask before resize");
    const bool clear = !tiles && ntiles == 0;
    if (!clear && !tiles) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (!clear && ntiles != conv_tiles_x(ctx) * conv_tiles_y(ctx))
        return pt_set_error(MI3PT_ERR_INVALID, "the mask's size does not match the tile map (ceil(rows / 8) x ceil(width / 8) bytes)");
    if (int rc = flush_pending(ctx)) return rc;      // the frames queued so far were submitted under the old mask
    if (clear || ntiles == 0) {                       // (a rank without rows has nothing to mask)
        drop_sample_mask(ctx);
        return MI3PT_OK;
    }
    ctx->mask.resize(ntiles);
    uint32_t sampled = 0;
    for (size_t t = 0; t < ntiles; t++) {
        ctx->mask[t] = tiles[t] ? 1 : 0;
        sampled += tiles[t] ? 1u : 0u;
    }
    ctx->mask_sampled = sampled;
    ctx->mask_epoch = ++ctx->mask_epochs;
    return MI3PT_OK;
}

extern "C" int mi3pt_read_sample_mask(mi3pt_ctx *ctx, uint8_t *dst, size_t ntiles, uint32_t *sampled_out)
{
    PT_GROUP(ctx, group_read_sample_mask(ctx, dst, ntiles, sampled_out));
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_read_sample_mask before resize");
    const size_t need = conv_tiles_x(ctx) * conv_tiles_y(ctx);
    if (ntiles != need) return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the tile map (ceil(rows / 8) x ceil(width / 8) bytes)");
    if (!dst && need) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (ctx->mask.empty()) {
        if (need) std::memset(dst, 1, need);
        if (sampled_out) *sampled_out = (uint32_t)need;
        return MI3PT_OK;
    }
    std::memcpy(dst, ctx->mask.data(), need);
    if (sampled_out) *sampled_out = ctx->mask_sampled;
    return MI3PT_OK;
}

extern "C" int mi3pt_freeze_converged(mi3pt_ctx *ctx, int guard, uint32_t *sampled_out)
{
    PT_GROUP(ctx, group_freeze_converged(ctx, guard, sampled_out));
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    if (guard != 0 && guard != 1) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_freeze_converged: guard must be 0 or 1");
    if (int rc = conv_wait(ctx, "mi3pt_freeze_converged")) return rc;
    const size_t tiles_x = conv_tiles_x(ctx), tiles_y = conv_tiles_y(ctx), n = tiles_x * tiles_y;
    std::vector<float> records(n * 4);
    if (n)
        if (int rc = mi3pt_read_convergence_tiles(ctx, records.data(), records.size())) return rc;
    std::vector<uint8_t> mask(n, 1);
    if (!ctx->mask.empty()) mask = ctx->mask;
    uint32_t sampled = 0;
    if (int rc = mi3pt_host_freeze_tiles(records.data(), (int)tiles_x, (int)tiles_y, ctx->conv_threshold, ctx->conv_min_frames, guard, mask.data(), &sampled)) return rc;
    if (n)
        if (int rc = mi3pt_set_sample_mask(ctx, mask.data(), n)) return rc;
    if (sampled_out) *sampled_out = sampled;
    return MI3PT_OK;
}
