// pt_ctx_calls.h -- what crosses the translation units of the context (pt_context.hip and pt_ctx_*.hip): every function that more than one
// of them uses, declared once under the unit that defines it, with its contract.  The rule: a call from one unit into another is declared
// here, or the function is static.  What the context OWNS is pt_ctx.h.  Host code only.
#pragma once
#include "pt_ctx.h"

// ================================================ pt_context.hip: the core ================================================
// (the last error: pt_set_error / pt_last_error, pt_internal.h)

// A context, and its device current: MI3PT_ERR_INVALID for a null handle, MI3PT_ERR_HIP where hipSetDevice fails.
int require_ctx(mi3pt_ctx *ctx);
// Every wait of a blocking entry point: for the event, or (ev == nullptr) for the stream; bounded while the launch gate is armed (a held
// launch is released from the host after gate_timeout_ms without progress).  `why` goes into the warning.
hipError_t ctx_wait(mi3pt_ctx *ctx, hipStream_t s, hipEvent_t ev, const char *why);
static inline hipError_t ctx_stream_sync(mi3pt_ctx *ctx, hipStream_t s, const char *why = "stream wait") { return ctx_wait(ctx, s, nullptr, why); }
static inline hipError_t ctx_event_sync(mi3pt_ctx *ctx, hipEvent_t ev, const char *why = "event wait") { return ctx_wait(ctx, nullptr, ev, why); }
// ctx->batch_cap from the options and the tile split, capped by a quarter of the memory that is free now: after mi3pt_resize and after a
// batch option changed.  Nothing to do before the first resize.
void recompute_batch_cap(mi3pt_ctx *ctx);

// Blocks of launch-invariant scalars for the raytrace kernel's service step (pt::RtService), one per batched launch.  Launches
// alternate between two streams and at most two are in flight; a slot is rewritten (in stream order, by the setup kernel of
// launch k + SERVICE_SLOTS) on the stream launch k ran on, i.e. after it.
static const int SERVICE_SLOTS = 8;
static inline size_t service_slot_bytes() { return (pt::service_block_bytes() + 255) / 256 * 256; }

// ---- image planes: the local_rows x width images of a context (radiance, mean, feature images, filter images, moments) ----
static inline size_t plane_texels(const mi3pt_ctx *ctx) { return (size_t)ctx->local_rows * ctx->width; }
static inline size_t plane_bytes(const mi3pt_ctx *ctx) { return plane_texels(ctx) * 16; }
// Blocking copy from device memory on the context's stream to (pageable) host memory; the bounded wait comes first.  Nothing to copy: the
// stream is not touched.
hipError_t read_plane(mi3pt_ctx *ctx, const void *src, size_t nbytes, void *dst);
// the 8 x 8 tiles of the error estimate and the sample mask, over the rows this context holds
static inline size_t conv_tiles_x(const mi3pt_ctx *ctx) { return ((size_t)ctx->width + 7) / 8; }
static inline size_t conv_tiles_y(const mi3pt_ctx *ctx) { return ((size_t)ctx->local_rows + 7) / 8; }

// ================================================ pt_ctx_scene.hip: the scene and its lazy analyses ================================================
// The device's scene as the kernels take it: the buffers of the active layout, counts, flags.  After prepare_layout and prepare_cull.
pt::SceneRefs scene_refs(const mi3pt_ctx *ctx);
// The scene is complete when the three buffers agree with each other (MI3PT_ERR_STATE otherwise); an empty scene is legal.
int check_scene(const mi3pt_ctx *ctx);
// The lazy debug relabelling of mi3pt_debug_set_packet_layout; nothing to do unless the layout is dirty.  Flushes the frame queue first.
int prepare_layout(mi3pt_ctx *ctx);
// The lazy scene analysis behind the culling walks (kernel variants 9 .. 14); runs when the triangles, the tree or an option that shapes
// the packets changed.
int prepare_cull(mi3pt_ctx *ctx);

// ================================================ pt_ctx_launch.hip: the launch path ================================================
// require_ctx + flush of the deferred frame queue: every entry point that observes or changes device state goes through this.
int require_idle(mi3pt_ctx *ctx);
// Launches everything that is queued, batch_cap frames at a time; the queue is emptied even on failure.  The device is current already
// (require_ctx): the lazy scene analyses and the features that work on the mean call this.
int flush_pending(mi3pt_ctx *ctx);
// The accumulate pass's uniforms as mi3pt_set_uniforms left them, and the tile of the image this context holds.
pt::AccUniforms acc_uniforms(const mi3pt_ctx *ctx);
pt::Tile tile_of(const mi3pt_ctx *ctx);
// Folds parity `par`'s finished batch launch (its event pair, waited for) into the launch statistics; nothing pending: nothing done.
int collect_rt_time(mi3pt_ctx *ctx, int par);
// The fullscreen pass on the context's stream, from the mean (or the last radiance) into the canvas, with the uniforms `u_fs`.
int run_fullscreen(mi3pt_ctx *ctx, const uint8_t *u_fs);

// ================================================ pt_ctx_image.hip: the images and their features ================================================
// Whether a first-hit pass walks the shipped walk's data (walk 13) -- after prepare_layout and prepare_cull.
bool first_hit_walk_is_shipped(const mi3pt_ctx *ctx);

// ================================================ pt_ctx_group.hip: device groups ================================================
// ---- device groups (mi3pt_create_group; implementation in pt_ctx_group.hip).  A group handle is an mi3pt_ctx whose
// `group` member is set: every entry point first hands such a handle to its group_* counterpart.
struct GroupState {
    std::vector<mi3pt_ctx *> members;
    mi3pt_ctx *present = nullptr;
    int block_rows = 8;
    int width = 0, height = 0;
    bool gathered = false;        // the presenting context holds the members' current accumulation images
    bool want_present = false;    // a fullscreen pass has been submitted since the canvas was last drawn
    // The scene lives in member 0: uploads and the host-side analyses (packets, leaf ranks, the cull analysis) happen there once;
    // the other members receive device-to-device copies of the finished buffers (group_sync_scene).
    uint64_t cloned_epoch = 0;    // member 0's scene_epoch the other members' copies were made from
    // Can the presenting device's copy engines address member i's memory directly?  (same device, or peer access enabled and
    // confirmed at create).  Where not -- or after a direct gather failed -- the gather is staged through pinned host memory.
    std::vector<char> peer_direct;
    PinnedBuf<void> stage;        // pinned host buffer (allocated when first needed)
    // first-hit feature images: which the members hold (rendered since the last resize), and which of those the presenting
    // context's whole image is a current copy of
    bool aov_rendered[MI3PT_AOV_COUNT] = {}, aov_gathered[MI3PT_AOV_COUNT] = {};
};

#define PT_GROUP(ctx, call) do { if ((ctx) && (ctx)->group) return (call); } while (0)
// one call applied to every member (and, where marked, to the presenting context too)
#define PT_GROUP_ALL(ctx, with_present, ...)                                                                              \
    do {                                                                                                                  \
        if ((ctx) && (ctx)->group) {                                                                                      \
            auto fn_ = [&](mi3pt_ctx *m) -> int { return __VA_ARGS__; };                                                  \
            return group_each((ctx), (with_present), fn_);                                                                \
        }                                                                                                                 \
    } while (0)
template <class F>
static int group_each(mi3pt_ctx *g, bool with_present, F fn)
{
    for (mi3pt_ctx *m : g->group->members)
        if (int rc = fn(m)) return rc;
    if (with_present)
        if (int rc = fn(g->group->present)) return rc;
    return MI3PT_OK;
}

// what mi3pt_<name> does with a group handle; group_member0: where a group's scene lives; group_unsupported: MI3PT_ERR_STATE with `what`
mi3pt_ctx *group_member0(mi3pt_ctx *g);
int group_unsupported(const char *what);
int group_destroy(mi3pt_ctx *g);
int group_resize(mi3pt_ctx *g, int width, int height);
int group_reset(mi3pt_ctx *g);
int group_set_uniforms(mi3pt_ctx *g, int pass, const void *bytes, size_t nbytes);
int group_submit_frames(mi3pt_ctx *g, unsigned pass_mask, uint32_t count);
int group_flush(mi3pt_ctx *g);
int group_sync(mi3pt_ctx *g);
int group_read_texture(mi3pt_ctx *g, int which, float *dst, size_t nfloats);
int group_write_texture(mi3pt_ctx *g, int which, const float *src, size_t nfloats);
int group_read_canvas(mi3pt_ctx *g, uint8_t *dst, size_t nbytes);
int group_accumulation_ptr(mi3pt_ctx *g, void **dev_ptr, size_t *nbytes);
int group_pass_time(mi3pt_ctx *g, int pass, float *us);
int group_launch_stats(mi3pt_ctx *g, int reset, double *total_ms, uint64_t *launches, uint64_t *frames);
int group_launch_span(mi3pt_ctx *g, double *span_ms);
int group_counters(mi3pt_ctx *g, uint64_t *out);
int group_render_aovs(mi3pt_ctx *g, unsigned aov_mask);
int group_read_aov(mi3pt_ctx *g, int which, void *dst, size_t nbytes);
int group_aov_ptr(mi3pt_ctx *g, int which, void **dev_ptr, size_t *nbytes);
int group_set_moments(mi3pt_ctx *g, int enabled);
int group_read_moments(mi3pt_ctx *g, void *dst, size_t nbytes);
int group_moments_ptr(mi3pt_ctx *g, void **dev_ptr, size_t *nbytes);
int group_read_convergence(mi3pt_ctx *g, mi3pt_convergence *out);
int group_read_convergence_tiles(mi3pt_ctx *g, float *dst, size_t nfloats);
int group_set_sample_mask(mi3pt_ctx *g, const uint8_t *tiles, size_t ntiles);
int group_read_sample_mask(mi3pt_ctx *g, uint8_t *dst, size_t ntiles, uint32_t *sampled_out);
int group_freeze_converged(mi3pt_ctx *g, int guard, uint32_t *sampled_out);
int group_get_option(mi3pt_ctx *g, int option, int *value);
int group_set_option(mi3pt_ctx *g, int option, int value);
