// pt_ctx_probe.hip -- the context's probes (mi3pt_debug_*): wave time stamps, the walks' and the arithmetic's decisions on given inputs.
#include "../../include/mi3pt.h"
#include "pt_ctx_calls.h"

#include <hip/hip_runtime.h>
#include <string>

// the walk the probe runs: 1 = uploaded records, 2 = packets, 3 = packets + prepared-reciprocal slab test
static int pick_walk(const mi3pt_ctx *ctx) { return ctx->variant == 0 ? 3 : (ctx->variant >= 4 ? 3 : (ctx->variant == 3 ? 2 : ctx->variant)); }

// Diagnostic: per-wave begin / feed-empty / end stamps of the last persistent raytrace
// launch.  out == NULL enables (allocates) or, with capacity 0 and enable 0, disables it.
extern "C" int mi3pt_debug_wave_times(mi3pt_ctx *ctx, int enable, uint64_t *out, size_t capacity_slots,
                                      size_t *slots_out)
{
    PT_GROUP(ctx, mi3pt_debug_wave_times(group_member0(ctx), enable, out, capacity_slots, slots_out));
    if (int rc = require_idle(ctx)) return rc;
    const int slots = pt::PT_MAX_RESIDENT_WAVES;
    if (!out) {
        HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
        if (enable && !ctx->d_wave_times) {
            HIP_TRY(ctx->d_wave_times.alloc((size_t)slots * 128));
            HIP_TRY(hipMemset(ctx->d_wave_times, 0, (size_t)slots * 128));
            ctx->wave_times_slots = slots;
        } else if (!enable && ctx->d_wave_times) {
            ctx->d_wave_times.reset();
            ctx->wave_times_slots = 0;
        }
        return MI3PT_OK;
    }
    if (!ctx->d_wave_times) return pt_set_error(MI3PT_ERR_STATE, "wave times are not enabled");
    if (capacity_slots < (size_t)ctx->wave_times_slots) return pt_set_error(MI3PT_ERR_INVALID, "buffer too small");
    HIP_TRY(read_plane(ctx, ctx->d_wave_times, (size_t)ctx->wave_times_slots * 128, out));
    if (slots_out) *slots_out = (size_t)ctx->wave_times_slots;
    return MI3PT_OK;
}

extern "C" int mi3pt_debug_intersect(mi3pt_ctx *ctx, const float *rays, size_t n, float *out)
{
    PT_GROUP(ctx, mi3pt_debug_intersect(group_member0(ctx), rays, n, out));
    if (int rc = require_idle(ctx)) return rc;
    if (!rays || !out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = check_scene(ctx)) return rc;
    if (n == 0) return MI3PT_OK;
    DevBuf<float> d_rays, d_out;
    HIP_TRY(d_rays.alloc(n * 24));
    if (d_out.alloc(n * 48) != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, "hipMalloc failed");
    hipError_t e = hipMemcpyAsync(d_rays, rays, n * 24, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        pt::launch_debug_intersect(scene_refs(ctx), d_rays, n, d_out, pick_walk(ctx), ctx->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = read_plane(ctx, d_out, n * 48, out);
    if (e != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, std::string("debug_intersect: ") + hipGetErrorString(e));
    return MI3PT_OK;
}

// the shipped first-hit walk (k_aov_cull's loop) on rays from memory; never another walk in its place
extern "C" int mi3pt_debug_intersect_shipped(mi3pt_ctx *ctx, const float *rays, size_t n, float *out)
{
    PT_GROUP(ctx, mi3pt_debug_intersect_shipped(group_member0(ctx), rays, n, out));
    if (int rc = require_idle(ctx)) return rc;
    if (!rays || !out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = check_scene(ctx)) return rc;
    if (int rc = prepare_layout(ctx)) return rc;    // (what mi3pt_render_aovs does before it picks its walk)
    if (int rc = prepare_cull(ctx)) return rc;
    const pt::SceneRefs scene = scene_refs(ctx);
    if (!first_hit_walk_is_shipped(ctx) || !scene.cwide || !scene.tripk64 || !scene.leaf_rank)
        return pt_set_error(MI3PT_ERR_STATE, "debug_intersect_shipped: mi3pt_render_aovs would not run the shipped first-hit walk on this scene / these options");
    if (n == 0) return MI3PT_OK;
    DevBuf<float> d_rays, d_out;
    HIP_TRY(d_rays.alloc(n * 24));
    if (d_out.alloc(n * 48) != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, "hipMalloc failed");
    hipError_t e = hipMemcpyAsync(d_rays, rays, n * 24, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        pt::launch_debug_intersect_cull(scene, d_rays, n, d_out, ctx->wide_stack_worst, ctx->leaf_min, ctx->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = read_plane(ctx, d_out, n * 48, out);
    if (e != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, std::string("debug_intersect_shipped: ") + hipGetErrorString(e));
    return MI3PT_OK;
}

extern "C" int mi3pt_debug_pairs(mi3pt_ctx *ctx, int fn, const float *rays, const float *geom, float *out, size_t n)
{
    PT_GROUP(ctx, mi3pt_debug_pairs(group_member0(ctx), fn, rays, geom, out, n));
    if (int rc = require_idle(ctx)) return rc;
    if (!rays || !geom || !out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (fn != 0 && fn != 1) return pt_set_error(MI3PT_ERR_INVALID, "debug_pairs: fn must be 0 (box) or 1 (triangle)");
    if (n == 0) return MI3PT_OK;
    const size_t G = fn == 0 ? 7 : 9;
    DevBuf<float> d_rays, d_geom, d_out;
    hipError_t e = d_rays.alloc(n * 24);
    if (e == hipSuccess) e = d_geom.alloc(n * G * 4);
    if (e == hipSuccess) e = d_out.alloc(n * 48);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays, rays, n * 24, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_geom, geom, n * G * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        pt::launch_debug_pairs(fn, d_rays, d_geom, d_out, n, ctx->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = read_plane(ctx, d_out, n * 48, out);
    if (e != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, std::string("debug_pairs: ") + hipGetErrorString(e));
    return MI3PT_OK;
}

extern "C" int mi3pt_debug_math(mi3pt_ctx *ctx, int fn, const float *a, const float *b, float *out, size_t n)
{
    PT_GROUP(ctx, mi3pt_debug_math(group_member0(ctx), fn, a, b, out, n));
    if (int rc = require_idle(ctx)) return rc;
    if (!a || !out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (n == 0) return MI3PT_OK;
    DevBuf<float> d_a, d_b, d_o;
    hipError_t e = d_a.alloc(n * 4);
    if (e == hipSuccess) e = d_o.alloc(n * 4);
    if (e == hipSuccess && b) e = d_b.alloc(n * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(d_a, a, n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && b) e = hipMemcpyAsync(d_b, b, n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        pt::launch_debug_math(fn, d_a, d_b, d_o, n, ctx->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = read_plane(ctx, d_o, n * 4, out);
    if (e != hipSuccess) return pt_set_error(MI3PT_ERR_HIP, std::string("debug_math: ") + hipGetErrorString(e));
    return MI3PT_OK;
}
