/*
 * mi3pt.h -- C ABI of libmi3pt.so, the MI355X (gfx950) path-tracing back-end.
 *
 * This is the drop-in boundary for the reference's per-pixel ray-trace path
 * (umar-ahmed/webgpu-pathtracer: src/passes/, src/renderer.ts, src/scene.ts).  The
 * reference has no FFI: its seam is the WebGPU device/queue API as used by the three
 * Pass classes and the Renderer.  Every entry point below replaces one group of those
 * WebGPU calls and cites it (paths relative to the reference root).  Buffers cross
 * the boundary as RAW BYTES IN THE REFERENCE'S OWN LAYOUTS (what webgpu-utils
 * computes from the WGSL structs):
 *
 *   Triangle  112 B  raytrace.wgsl:40-49    BVHNode  48 B  raytrace.wgsl:51-64
 *   Material   64 B  raytrace.wgsl:31-38    Uniforms 96 B  raytrace.wgsl:66-75
 *   accumulate Uniforms 16 B accumulate.wgsl:1-5
 *   fullscreen Uniforms 24 B fullscreen.wgsl:14-20
 *   environment / CDF textures: 1024x512 rgba32float, renderer.ts:111-130
 *
 * Conventions
 *   - plain C types only; every function returns an mi3pt_status (0 = OK) unless
 *     stated otherwise; mi3pt_last_error() gives the message for the calling thread
 *     (the N-API / ctypes shims turn it into a thrown Error, like the reference's
 *     `throw new Error(...)` sites renderer.ts:65-67, 133-143, 514-516).
 *   - uploads COPY at call time (queue.writeBuffer / writeTexture semantics); the
 *     caller keeps ownership of its memory.
 *   - mi3pt_submit() is asynchronous and stream ordered, like
 *     `device.queue.submit([encoder.finish()])` (renderer.ts:389-390).  A context has ONE stream -- its own, or the
 *     caller's (mi3pt_set_stream) -- and everything that can be observed happens in that stream's order; the raytrace
 *     kernels run on internal streams tied to it by events in both directions, which no caller can see.
 *     STREAM ORDERED, returning before the device has run anything: mi3pt_submit, mi3pt_submit_frames, mi3pt_flush,
 *     mi3pt_reset, mi3pt_reset_counters, mi3pt_render_aovs, mi3pt_denoise_guided, mi3pt_estimate_convergence, mi3pt_reproject,
 *     mi3pt_reproject_scene, mi3pt_hold_history, mi3pt_merge_history, mi3pt_set_mean_by_count, mi3pt_set_sample_mask (it launches the frame queue, under the old mask, and waits for nothing).  mi3pt_set_uniforms, the setters of
 *     modes and options and the *_device_ptr getters start no device work of their own (those that observe state launch
 *     the frame queue first).  A host that has set its own stream may therefore enqueue its work in front of and behind
 *     these calls on that stream -- fill a bound accumulation tensor, copy out of a *_device_ptr image -- and wait once.
 *     BLOCKING (the host waits for the context's stream, at least): every upload and mi3pt_write_* (copy at call time),
 *     mi3pt_resize (the internal streams too), mi3pt_set_stream (the stream it leaves), mi3pt_bind_accumulation,
 *     mi3pt_set_moments when it changes the state, every mi3pt_read_*, mi3pt_sync, mi3pt_get_counters, mi3pt_pass_time_us,
 *     mi3pt_raytrace_launch_stats / _span, the mi3pt_debug_* probes, mi3pt_device_build_bvh, mi3pt_device_build_bvh_ex, mi3pt_device_refit_bvh, mi3pt_destroy.
 *     BLOCKING, but for ONE EVENT only and without launching the frame queue: mi3pt_read_convergence and
 *     mi3pt_read_convergence_tiles wait for the most recent mi3pt_estimate_convergence, not for what was enqueued behind it;
 *     mi3pt_freeze_converged waits for the same event, then acts as mi3pt_set_sample_mask.  mi3pt_read_sample_mask reads host state.
 *     Three things make a stream-ordered call wait ONCE: the first raytrace submit or mi3pt_render_aovs after a scene
 *     upload (or a change of kernel variant) compiles the scene and reads it back; the first call that needs an image
 *     allocates it, and a launch deeper than any before on this context replaces its radiance slots (freeing waits for
 *     the whole device, the caller's other streams included); with timing enabled a launch waits for the one two
 *     before it.  A job of a shape the context has run before waits for nothing (tests/test_gpu_streams.py).
 *   - one host thread per context; no callbacks.
 *   - there is NO CPU fallback: without a HIP device mi3pt_create() fails with
 *     MI3PT_ERR_NO_DEVICE.  The mi3pt_host_* functions are the reference's own
 *     CPU-side scene compile (BVH build, env CDF) and need no device.
 */
#ifndef MI3PT_H
#define MI3PT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 5): mi3pt_set_tile deals the row blocks back and forth (ABI 2 as first released dealt them one way: a host that
 * de-interleaves gathered rows must use mi3pt_tile_global_row / mi3pt_tile_owner, not its own copy of the old formula);
 * MI3PT_OPT_BATCH defaults to 256 frames per launch (was 64), MI3PT_OPT_WALK_MIN reads 0 = "by the size of the tree" (was 32);
 * new exports mi3pt_tile_global_row, mi3pt_tile_owner; new options MI3PT_OPT_GATE_TIMEOUT_MS, MI3PT_OPT_GATE_RELEASES, MI3PT_OPT_CAMERA_BASE,
 * MI3PT_OPT_PACKET_ORDER, MI3PT_OPT_SIX_WAVES (22 .. 27); MI3PT_OPT_WAVES_PER_CU reads up to 24 (six waves per SIMD). */
/* 4 (round 6): mi3pt_set_rows and mi3pt_measure_tile_cost are GONE (contiguous cost-balanced bands: measured 7 % slower than the dealt
 * 8-row blocks in round 4 and kept since as dead surface); mi3pt_set_kernel_variant accepts 14 (the eight-wide walk: an option).
 * Added since under the same number (nothing existing changed): mi3pt_host_sky_tiles, MI3PT_OPT_SKY_TILES (31); mi3pt_host_scene_compile; mi3pt_host_walk_buffer; mi3pt_host_route;
 * mi3pt_render_aovs, mi3pt_read_aov, mi3pt_aov_device_ptr, enum mi3pt_aov, MI3PT_PASS_AOV (3); mi3pt_denoise_guided, mi3pt_read_guided,
 * mi3pt_guided_device_ptr, struct mi3pt_guided_params, MI3PT_GUIDED_PRESENT, MI3PT_PASS_GUIDED (4); mi3pt_estimate_convergence,
 * mi3pt_read_convergence, mi3pt_read_convergence_tiles, struct mi3pt_convergence, MI3PT_PASS_CONVERGENCE (5); mi3pt_set_sample_mask,
 * mi3pt_read_sample_mask, mi3pt_freeze_converged, mi3pt_host_freeze_tiles; mi3pt_set_mean_by_count, mi3pt_host_view_frame, mi3pt_reproject,
 * struct mi3pt_reproject_params, MI3PT_PASS_REPROJECT (6); mi3pt_keep_geometry, mi3pt_reproject_scene, struct mi3pt_reproject_scene_params;
 * mi3pt_hold_history, mi3pt_merge_history, struct mi3pt_history_params, MI3PT_HISTORY_EPS, MI3PT_PASS_HISTORY (7);
 * MI3PT_GUIDED_YOUNG, MI3PT_GUIDED_YOUNG_COUNT; mi3pt_set_guided_despike, mi3pt_read_guided_despiked; mi3pt_device_refit_bvh, mi3pt_host_bvh_cost;
 * mi3pt_device_build_bvh_ex, struct mi3pt_bvh_build_params, struct mi3pt_bvh_build_info, MI3PT_BVH_METHOD_*, MI3PT_PLOC_SEARCH_BLOCK. */
#define MI3PT_ABI_VERSION 4

typedef enum mi3pt_status {
    MI3PT_OK = 0,
    MI3PT_ERR_INVALID = 1,    /* bad argument / wrong byte size */
    MI3PT_ERR_NO_DEVICE = 2,  /* no HIP device (renderer.ts:514-516 "WebGPU device not found.") */
    MI3PT_ERR_HIP = 3,        /* a HIP runtime call failed */
    MI3PT_ERR_STATE = 4       /* call made in the wrong state (e.g. submit before resize) */
} mi3pt_status;

/* strides of the reference layouts */
#define MI3PT_TRIANGLE_STRIDE 112
#define MI3PT_BVHNODE_STRIDE 48
#define MI3PT_MATERIAL_STRIDE 64
#define MI3PT_RAYTRACE_UNIFORMS_SIZE 96
#define MI3PT_ACCUMULATE_UNIFORMS_SIZE 16
#define MI3PT_FULLSCREEN_UNIFORMS_SIZE 24
#define MI3PT_ENV_WIDTH 1024
#define MI3PT_ENV_HEIGHT 512

/* the three passes of renderer.ts:23-27 */
typedef enum mi3pt_pass {
    MI3PT_PASS_RAYTRACE = 0,
    MI3PT_PASS_ACCUMULATE = 1,
    MI3PT_PASS_FULLSCREEN = 2,
    MI3PT_PASS_AOV = 3,          /* -- no counterpart: the first-hit feature images (mi3pt_render_aovs).  Known to
                                    mi3pt_pass_time_us only; it has no uniform block (mi3pt_set_uniforms refuses it) */
    MI3PT_PASS_GUIDED = 4,       /* -- no counterpart: the feature-guided de-noise (mi3pt_denoise_guided), pack kernel and every level.
                                    Known to mi3pt_pass_time_us only */
    MI3PT_PASS_CONVERGENCE = 5,  /* -- no counterpart: the per-tile error estimate (mi3pt_estimate_convergence), its tile kernel and the
                                    kernel that folds the summary.  Known to mi3pt_pass_time_us only */
    MI3PT_PASS_REPROJECT = 6,    /* -- no counterpart: the gather kernel of mi3pt_reproject and the copy into a bound accumulation image (the
                                    feature render inside that call is MI3PT_PASS_AOV's).  Known to mi3pt_pass_time_us only */
    MI3PT_PASS_HISTORY = 7       /* -- no counterpart: the kernel of mi3pt_merge_history and the copy into a bound accumulation image.
                                    Known to mi3pt_pass_time_us only */
} mi3pt_pass;

#define MI3PT_SUBMIT_RAYTRACE 1u
#define MI3PT_SUBMIT_ACCUMULATE 2u
#define MI3PT_SUBMIT_FULLSCREEN 4u

/* which image mi3pt_read_texture() returns */
typedef enum mi3pt_texture {
    MI3PT_TEX_OUTPUT = 0,        /* renderer.outputTexture (renderer.ts:94-109): the frame's radiance
                                    after a raytrace pass, the running mean after an accumulate pass
                                    (accumulate.ts:171-175 copies it back).  Under a sample mask
                                    (mi3pt_set_sample_mask) a queued frame's radiance is written for the
                                    SAMPLED tiles only where the launch takes a tile list: the radiance
                                    texels of frozen tiles are not written and hold whatever they held */
    MI3PT_TEX_ACCUMULATION = 1,  /* accumulate.ts:45-59 accumulationTexture == outputTexturePrev */
    MI3PT_TEX_CANVAS = 2         /* the fullscreen pass's colour attachment, as float RGBA
                                    (canvas_w x canvas_h, row 0 = top) */
} mi3pt_texture;

/* The feature images of the FIRST HIT (AOVs, a G-buffer), mi3pt_render_aovs.  The reference renders none; each is defined by
 * the reference's own functions: the un-jittered camera ray of the texel (getUv raytrace.wgsl:247-250, cameraToRay :217-245)
 * and its closest hit (raySceneIntersect :205-211; the hit record of rayTriangleIntersect :78-116).  Each image is
 * local_rows x width x 16 bytes, rows and tile compaction exactly as MI3PT_TEX_OUTPUT, fp32 / i32 whatever mi3pt_set_storage says.
 *                                   hit                                                   miss (and texels outside `resolution`)
 *   ALBEDO    4 x f32   materials[hit.material].color.rgb (raytrace.wgsl:31-38), 1.0      0, 0, 0, 0
 *   NORMAL    4 x f32   hit.normal.xyz as :105-112 forms it (interpolated, normalised,    0, 0, 0, 0
 *                       world space, NOT flipped towards the ray), 0.0
 *   POSITION  4 x f32   hit.position.xyz (origin + t * direction, :111), t                0, 0, 0, 1e20 (the miss record's t, INF, :155)
 *   IDS       4 x i32   triangle index (into the uploaded 112-byte records),              -1, -1, 0, 0
 *                       materialIndex (:49), 1, 0 */
typedef enum mi3pt_aov {
    MI3PT_AOV_ALBEDO = 0,
    MI3PT_AOV_NORMAL = 1,
    MI3PT_AOV_POSITION = 2,
    MI3PT_AOV_IDS = 3,
    MI3PT_AOV_COUNT = 4
} mi3pt_aov;

/* texel storage of output / accumulation textures */
typedef enum mi3pt_storage {
    MI3PT_STORAGE_F32 = 0,       /* keep fp32 (default; what the 1e-4 parity target needs) */
    MI3PT_STORAGE_F16 = 1        /* round every stored texel through binary16 = the reference's
                                    rgba16float textures (renderer.ts:102, accumulate.ts:52) */
} mi3pt_storage;

/* what a submit that includes MI3PT_SUBMIT_FULLSCREEN shows (mi3pt_set_present_mode) */
typedef enum mi3pt_present_mode {
    MI3PT_PRESENT_EXACT = 0,     /* the canvas is drawn from the running mean INCLUDING this submit's frame:
                                    renderer.ts:379-390 as written, one accumulate pass and one fullscreen pass
                                    per presenting frame, in frame order.  The frames' raytrace passes are
                                    launched together, up to MI3PT_OPT_PRESENT_DEPTH (16) frames at a time,
                                    when the queue is that deep or the context is observed (read-back, sync,
                                    flush): nothing that can be read differs from a launch per frame. */
    MI3PT_PRESENT_LATEST = 1     /* headless hosts: the frame is queued like any other; the canvas is drawn
                                    from the running mean of the batches launched so far, and only when that
                                    mean or the fullscreen uniforms changed since the last draw.  A submit
                                    with FULLSCREEN alone (render() after sampling has stopped,
                                    renderer.ts:369-373) launches the queue and shows every frame. */
} mi3pt_present_mode;

/* counters accumulated by every raytrace pass since the last mi3pt_reset_counters() */
typedef enum mi3pt_counter {
    MI3PT_CNT_RAYS = 0,       /* raySceneIntersect calls (raytrace.wgsl:379) */
    MI3PT_CNT_BOX_TESTS = 1,  /* rayAABBIntersect calls  (raytrace.wgsl:118) = N_box */
    MI3PT_CNT_TRI_TESTS = 2,  /* rayTriangleIntersect calls (raytrace.wgsl:78) = N_tri */
    MI3PT_CNT_HITS = 3,
    MI3PT_CNT_MISSES = 4,     /* environment lookups */
    MI3PT_CNT_STACK_OVERFLOWS = 5, /* traversals aborted at raytrace.wgsl:167-171 */
    MI3PT_CNT_PIXELS = 6,     /* (pixel, frame) jobs executed */
    MI3PT_CNT_RESERVED = 7,
    MI3PT_CNT_COUNT = 8
} mi3pt_counter;

typedef struct mi3pt_ctx mi3pt_ctx;

/* ---- library ---- */
int mi3pt_abi_version(void);
const char *mi3pt_last_error(void);

/* ---- device discovery: Renderer.diagnostic(), renderer.ts:470-489 ---- */
int mi3pt_device_count(int *count);
int mi3pt_device_name(int device, char *name, size_t capacity);

/* ---- context: Renderer.create() + constructor, renderer.ts:47-92, 491-533.
 * Creates the HIP stream, placeholder scene buffers (2 triangles / 1 material /
 * 1 node, raytrace.ts:72-77), zeroed environment textures and default uniforms.
 * destroy waits for submitted work first (renderer.ts:418-429). ---- */
int mi3pt_create(int device, mi3pt_ctx **out_ctx);
int mi3pt_destroy(mi3pt_ctx *ctx);
/* Renderer.create() over several GPUs of one node (the reference knows one adapter and one device, renderer.ts:491-533;
 * SURVEY.md 8e): the returned handle is used with the SAME entry points as a single-device context and renders the
 * same bits.  Behind it: one member context per listed device -- member i renders tile i of n (block_rows-row blocks
 * dealt round robin), every upload is replicated, nothing is exchanged per frame -- and a presenting context on
 * devices[0] that holds the whole image.  Reading the accumulation image or the canvas GATHERS: one strided
 * device-to-device copy per member (peer DMA over xGMI), de-interleaved on the way; no host staging, no collective
 * library.  Differences from a single context, all following from "the image is whole only after the gather":
 *   - mi3pt_read_texture / mi3pt_write_texture move WHOLE images (height x width), whatever the split;
 *   - the fullscreen pass runs on the gathered image, so a group always presents lazily: a FULLSCREEN submit is
 *     remembered and performed when the canvas is read (MI3PT_PRESENT_LATEST whatever mi3pt_set_present_mode says);
 *   - mi3pt_set_tile, mi3pt_set_stream and mi3pt_bind_accumulation are refused (MI3PT_ERR_STATE);
 *   - counters are the members' sums, pass times the slowest member's; the debug probes address member 0.
 * A device may be listed more than once (several members on one GPU: how the tests run it on a one-GPU box). */
int mi3pt_create_group(const int *devices, int ndevices, int block_rows, mi3pt_ctx **out_ctx);
/* Members of a group handle (1 for a plain context) and the member contexts themselves (index -1: the presenting
 * context), e.g. for per-device launch statistics.  They belong to the group: never destroy or resize them. */
int mi3pt_group_size(mi3pt_ctx *ctx, int *members);
int mi3pt_group_member(mi3pt_ctx *ctx, int index, mi3pt_ctx **member);

/* Run on a caller-owned hipStream_t instead of the context's own: from now on everything the conventions above call stream
 * ordered is enqueued on it.  Launches what is queued on the stream the context leaves and BLOCKS until that stream is idle (not
 * the new one: work already on hip_stream stays in front of whatever the context sends there).
 * Handle 0 / NULL is NOT the HIP default stream: it restores the context's internal stream, which is created hipStreamNonBlocking
 * and is ordered with nothing of the caller's -- in particular not with work on torch's default stream, whose handle
 * (torch.cuda.current_stream().cuda_stream while no other stream is current) IS 0: a host that passes it gets MI3PT_OK and no
 * ordering.  Pass a stream you created -- hipStreamCreate*; with torch a torch.cuda.Stream() s, made current for the tensor
 * operations that go with the context's work (`with torch.cuda.stream(s):`), handle s.cuda_stream, as bench.py does.
 * The stream stays the caller's: keep it alive until mi3pt_destroy or the next mi3pt_set_stream; mi3pt_destroy waits for it and
 * leaves it usable.  Refused for a device group.  Held to the oracle by tests/test_gpu_streams.py. */
int mi3pt_set_stream(mi3pt_ctx *ctx, void *hip_stream);
int mi3pt_set_storage(mi3pt_ctx *ctx, int storage /* mi3pt_storage */);

/* Tile split (multi-GPU): the image's rows are dealt to the ranks in blocks of block_rows, round after round, BACK AND
 * FORTH: with gb = y / block_rows, round = gb / nranks, pos = gb % nranks this context renders the rows whose
 * (round odd ? nranks - 1 - pos : pos) == rank -- a cost that rises or falls down the image (floor, model, sky) is shared out
 * evenly (dealt one way only, rank 0 of eight had 5 % more work than rank 6).  Its textures are compact local_rows x width images,
 * rows in image order.  Default rank 0 of 1.  Takes effect at the next mi3pt_resize(). */
int mi3pt_set_tile(mi3pt_ctx *ctx, int rank, int nranks, int block_rows);
int mi3pt_tile_local_rows(int height, int rank, int nranks, int block_rows); /* returns the count */
/* The deal itself, for hosts that gather and de-interleave on their own (multi-process jobs: bench.py, a JS host per GPU) -- so
 * that nobody re-implements the formula above: the image row that local row `local_row` of `rank`'s compact texture holds
 * (may be >= height in a ragged last round: such rows do not exist; -1 for bad arguments), and the rank that owns image row y. */
int mi3pt_tile_global_row(int local_row, int rank, int nranks, int block_rows);
int mi3pt_tile_owner(int y, int nranks, int block_rows);

/* ---- scene upload: queue.writeBuffer of the structured views ----
 * raytrace.ts:104-121 (triangles), :138-160 (materials), :177-193 (BVH nodes).
 * nbytes must be a non-zero multiple of the stride.  Buffer handles are resolved at
 * dispatch time, so a new scene is picked up by the next submit (the reference needs
 * a reset() for that: raytrace.ts:403 vs :508-522).
 * mi3pt_upload_bvh checks EVERY record of the buffer, the nodes the root never reaches included: a child index of a non-leaf
 * node that is not negative must be greater than its parent's and inside the buffer, and a leaf's triangleIndex must not be
 * negative -- MI3PT_ERR_INVALID otherwise, and the scene uploaded before stays (the reference's walk would not care about
 * records it never visits; this is what bounds every walk on the device).  Anything else is rendered as the reference's walk
 * defines it: a leaf as root, absent children, shared subtrees, triangles with several leaves, isLeaf values other than 0 and 1
 * (internal nodes), boxes that are NaN, infinite, inverted or empty. */
int mi3pt_upload_triangles(mi3pt_ctx *ctx, const void *bytes, size_t nbytes);
int mi3pt_upload_materials(mi3pt_ctx *ctx, const void *bytes, size_t nbytes);
int mi3pt_upload_bvh(mi3pt_ctx *ctx, const void *bytes, size_t nbytes);

/* renderer.ts:132-157 (environment texels) and :253-280 (CDF texels): width/height
 * must be 1024 x 512 ("Environment texture must be 1024x512 pixels"). */
int mi3pt_upload_environment(mi3pt_ctx *ctx, const float *rgba, int width, int height);
int mi3pt_upload_environment_cdf(mi3pt_ctx *ctx, const float *rgba, int width, int height);

/* ---- textures: resize() / reset(), renderer.ts:283-295, 397-416 and
 * accumulate.ts:36-59.  (Re)allocates and ZEROES the output, accumulation and canvas
 * images; width x height is the canvas / full texture size. ---- */
int mi3pt_resize(mi3pt_ctx *ctx, int width, int height);
int mi3pt_reset(mi3pt_ctx *ctx);

/* ---- uniforms: Pass.setUniforms -> queue.writeBuffer(uniformsBuffer, 0, ...)
 * raytrace.ts:359-369, accumulate.ts:178-188, fullscreen.ts:138-148.  The host keeps
 * the structured view (partial set semantics live there) and sends the whole block:
 * 96 / 16 / 24 bytes. ---- */
int mi3pt_set_uniforms(mi3pt_ctx *ctx, int pass /* mi3pt_pass */, const void *bytes, size_t nbytes);

/* ---- execution: one command buffer, renderer.ts:379-390.  pass_mask is an OR of
 * MI3PT_SUBMIT_*; passes run in the reference's order raytrace -> accumulate ->
 * fullscreen (raytrace.ts:696-708, accumulate.ts:154-176, fullscreen.ts:158-177).
 * RAYTRACE|ACCUMULATE in one submit runs as one fused kernel (bit-identical to
 * the two-pass result).
 * Non-finite and negative radiance is no special case anywhere: NaN, +-inf,
 * negative and subnormal values that the reference's arithmetic produces --
 * log(0) in randNormal when rand() returns exactly 0, emission or environment
 * texels that overflow binary32 (or binary16 under MI3PT_STORAGE_F16), inf * 0
 * in the throughput, material fields outside [0, 1] or NaN -- are carried
 * exactly as that arithmetic carries them through the radiance storage, the
 * running mean and the tone-map; the RGBA8 canvas maps NaN to 0 and clamps the
 * rest to [0, 255].  The `frame` counters of the raytrace and the accumulate
 * block are u32 and wrap modulo 2^32; an accumulate `frame` of 0 (or 1)
 * anywhere, in the middle or at the end of a batch too, has weight 1 and
 * restarts the mean.  Held to the oracle and to the executed shader on every
 * kernel variant by tests/test_gpu_shading.py. ---- */
int mi3pt_submit(mi3pt_ctx *ctx, unsigned pass_mask);
/* `count` consecutive frames with one call: frame i is submitted with the raytrace and the
 * accumulate uniform `frame` fields at (their current value + i); afterwards both hold current +
 * count.  Exactly what `count` calls of Renderer.render() submit while only the frame counter
 * moves (renderer.ts:369-377); for headless hosts that render a fixed number of samples. */
int mi3pt_submit_frames(mi3pt_ctx *ctx, unsigned pass_mask, uint32_t count);
int mi3pt_sync(mi3pt_ctx *ctx);   /* queue.onSubmittedWorkDone(), renderer.ts:420 */
/* Default MI3PT_PRESENT_EXACT.  See mi3pt_present_mode. */
int mi3pt_set_present_mode(mi3pt_ctx *ctx, int mode /* mi3pt_present_mode */);
/* RAYTRACE|ACCUMULATE submits may be queued inside the library and launched together (up to
 * 256 consecutive frames whose uniforms differ only in `frame` -- 256 x nranks for a rank of a tile
 * split, at most 512 (MI3PT_OPT_BATCH, MI3PT_OPT_BATCH_LIMIT), less when memory is short: a quarter of
 * the free memory bounds the radiance slots -- run as one kernel + one ordered accumulate).  Every call that observes or changes device state launches the queue first;
 * mi3pt_flush does only that, without waiting -- use it before synchronising the stream
 * yourself (e.g. torch.cuda.synchronize()). */
int mi3pt_flush(mi3pt_ctx *ctx);
/* Frames one launch covers at the current size and tile split (the queue is launched by itself when
 * it holds this many).  A caller that wants launches of one shape flushes at a divisor of its job. */
int mi3pt_batch_capacity(mi3pt_ctx *ctx, int *frames);

/* ---- first-hit feature images -- no counterpart in the reference (see mi3pt_aov for what each image holds).
 * mi3pt_render_aovs renders the images named in aov_mask, an OR of (1u << mi3pt_aov), from the raytrace uniform block (96 B,
 * raytrace.wgsl:66-75) and the scene AS THEY ARE AT THE CALL; asynchronous and stream ordered like mi3pt_submit.  For every texel
 * of this context's share (local row ly = image row gy of mi3pt_set_tile's deal, column x):
 *   inside the rectangle -- x < u32(resolution.x) and gy < u32(resolution.y), the bounds test of raytrace.wgsl:425-427 --
 *     uv = (x / resolution.x, gy / resolution.y), ray = cameraToRay(camera, uv), hit = raySceneIntersect(ray): the closest t, of
 *     equal t the leaf the reference's walk visits first, best-so-far after the 64-entry abort (:167-171).  No jitter, no lens, no
 *     rand(): frame, maxBounces, samplesPerFrame, focalDistance, aperture, the environment and the other passes' blocks do not enter;
 *   outside: the miss values.  Every call defines every texel of every image it was asked for.
 * It is NOT a raytrace pass: nothing is added to mi3pt_get_counters, mi3pt_debug_last_launch / MI3PT_OPT_LAST_BUILD keep naming the
 * last SAMPLE launch, and queued sample frames stay queued -- the pass runs beside them, what they render is bit-identical with or
 * without it.  Images are allocated at the first call that asks for them and freed by mi3pt_resize / mi3pt_destroy (a context that
 * never asks allocates nothing).  Images rendered earlier are not altered by later uploads or uniform changes.
 *   MI3PT_ERR_STATE before mi3pt_resize or for an inconsistent scene (as a raytrace submit); MI3PT_ERR_INVALID for a mask of 0 or
 *   with unknown bits.
 * mi3pt_read_aov (blocking) copies image `which` to dst: nbytes = rows x width x 16.  mi3pt_aov_device_ptr hands out the device
 * image itself (zero copy, e.g. for a torch tensor; valid until the next mi3pt_resize; order your reads behind the context's
 * stream or call mi3pt_sync first).  Both: MI3PT_ERR_STATE for an image not rendered since the last resize, MI3PT_ERR_INVALID for
 * a wrong nbytes / unknown image.  Tile split: rows = this rank's compact rows.  Device group: the render goes to every member,
 * and these two GATHER the whole height x width image onto devices[0] like the accumulation image (two strided copies per member;
 * staged through pinned memory under MI3PT_OPT_GATHER_STAGED or without peer access).
 * With timing enabled, mi3pt_pass_time_us(MI3PT_PASS_AOV) is the device time of the most recent call (a group: the slowest member's). ---- */
int mi3pt_render_aovs(mi3pt_ctx *ctx, unsigned aov_mask);
int mi3pt_read_aov(mi3pt_ctx *ctx, int which /* mi3pt_aov */, void *dst, size_t nbytes);
int mi3pt_aov_device_ptr(mi3pt_ctx *ctx, int which /* mi3pt_aov */, void **dev_ptr, size_t *nbytes);

/* ---- feature-guided de-noise of the running mean -- no counterpart in the reference (its only de-noiser is the colour-only bilateral of
 * the fullscreen pass, fullscreen.wgsl:22-71).  An edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010) over the accumulation
 * image, guided by the four feature images of mi3pt_render_aovs.  Pinned arithmetic: fp32, round to nearest even, nothing contracted,
 * correctly rounded division, the library's exp (mi3pt_debug_math fn 4).  Per texel p = (x, y) of the width x rows image:
 *   c = rgb of MI3PT_TEX_ACCUMULATION, n = NORMAL.xyz, P = POSITION.xyz, a = ALBEDO.rgb, hit = word 2 of IDS;
 *   inv_X = 1 / (sigma_X * sigma_X) in fp32, and 0 for sigma_X == 0 (the term is off).
 * Level i = 0 .. levels - 1, step s = 1 << i, inv_c(i) = inv_color * 4^i (sigma_color halves per level); level i reads the output of level
 * i - 1, level 0 reads c.  Taps q = p + s * (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner, h = [1/16, 1/4, 3/8, 1/4, 1/16].  A tap COUNTS
 * iff q lies inside [0, width) x [0, rows) and hit(q) == hit(p); for each that counts, in that order:
 *   dc = c_q - c_p     ec = ((dc.x*dc.x + dc.y*dc.y) + dc.z*dc.z) * inv_c(i)
 *   dn = n_q - n_p     en = ((dn.x*dn.x + dn.y*dn.y) + dn.z*dn.z) * inv_normal
 *   da = a_q - a_p     ea = ((da.x*da.x + da.y*da.y) + da.z*da.z) * inv_albedo
 *   dP = P_q - P_p     pd = (n_p.x*dP.x + n_p.y*dP.y) + n_p.z*dP.z;   ep = (pd * pd) * inv_plane
 *   w  = exp(-(((ec + en) + ea) + ep)) * (h[dx] * h[dy])
 *   den = den + w;   num.k = num.k + w * c_q.k      (k = r, g, b; both start at 0)
 * Output: (num.r / den, num.g / den, num.b / den, c_p.w).  The centre tap always counts with w = 9/64, so den > 0 for finite inputs.
 * NON-FINITE inputs (texels, features, or a sigma so small that 1 / (sigma * sigma) overflows) give unspecified values; they neither hang
 * nor fault.
 * mi3pt_denoise_guided filters the running mean as mi3pt_read_texture(MI3PT_TEX_ACCUMULATION) would return it at the call -- frames still
 * queued are launched first, as for a read-back -- and the four feature images as they stand; asynchronous and stream ordered after that:
 * one small pack kernel and one launch per level on the context's stream, between two images the context allocates at the first call and
 * frees at mi3pt_resize / mi3pt_destroy.  It changes neither the accumulation image, nor the feature images, nor any counter; sample frames
 * submitted afterwards accumulate as if it had not been called.  With MI3PT_GUIDED_PRESENT the canvas is then drawn from the FILTERED image
 * by the fullscreen pass with its current uniforms, `denoise` taken as 0 (tone-map, scaling, RGBA8 as they are).
 *   MI3PT_ERR_STATE before mi3pt_resize; unless all four feature images have been rendered since the last resize; for a context whose tile
 *   is not the whole image (mi3pt_set_tile with more than one rank) and for a device group: five levels reach 32 rows up and down, the halo
 *   exchange is NOT BUILT -- gather into a 1-rank context (mi3pt_write_texture) and filter there.
 *   MI3PT_ERR_INVALID for levels outside 1 .. 5, a negative or non-finite sigma, unknown flag bits, a null pointer.
 * mi3pt_read_guided (blocking) copies the filtered image to dst: nbytes = rows x width x 16.  mi3pt_guided_device_ptr hands out the device
 * image (zero copy; valid until the next mi3pt_denoise_guided or mi3pt_resize; order your reads behind the context's stream or call
 * mi3pt_sync first).  Both: MI3PT_ERR_STATE before the first filter since the last resize, MI3PT_ERR_INVALID for a null pointer / a wrong
 * nbytes.  With timing enabled, mi3pt_pass_time_us(MI3PT_PASS_GUIDED) is the device time of the most recent filter (without the draw). ---- */
typedef struct mi3pt_guided_params {
    int levels;                  /* 1 .. 5 */
    float sigma_color, sigma_normal, sigma_albedo, sigma_plane;   /* finite, >= 0; 0 = term off */
    unsigned flags;              /* MI3PT_GUIDED_* */
} mi3pt_guided_params;
#define MI3PT_GUIDED_PRESENT 1u
int mi3pt_denoise_guided(mi3pt_ctx *ctx, const mi3pt_guided_params *params);
int mi3pt_read_guided(mi3pt_ctx *ctx, void *dst, size_t nbytes);
int mi3pt_guided_device_ptr(mi3pt_ctx *ctx, void **dev_ptr, size_t *nbytes);

/* ---- the moments image: the spread of the frames around the running mean -- no counterpart in the reference (accumulate.wgsl keeps
 * the mean alone).  Off by default.  While enabled every accumulate step also updates a second image beside the accumulation image:
 * local_rows x width x 4 fp32 = (M2.r, M2.g, M2.b, n), ALWAYS fp32 whatever mi3pt_set_storage says, rows and tile compaction exactly
 * those of the accumulation image.  Welford's update written around the reference's own mean -- for every accumulate step of a texel
 * inside the accumulate block's rectangle (x < resolution.x and gy < resolution.y, accumulate.wgsl:14-16), with c = this frame's
 * radiance rgb as the step reads it, p = the mean before the step, p' = the mean after it AS STORED (rounded to binary16 under
 * MI3PT_STORAGE_F16), fp32, nothing contracted, k = r, g, b:
 *   restart = (frame <= 1) || (enabled != 1)            exactly the steps whose weight is 1 (see mi3pt_submit)
 *   restart:   M2.k = 0;   n = 1
 *   otherwise: M2.k = M2.k + (c.k - p.k) * (c.k - p'.k);   n = n + 1
 * Texels outside the rectangle are not touched.  n is an fp32 count: it stops growing at 2^24 = 16 777 216 steps.  Non-finite radiance
 * is carried as this arithmetic carries it.  M2.k / (n - 1) is the sample variance of channel k, M2.k / (n (n - 1)) the variance of
 * its mean -- what MI3PT_GUIDED_VARIANCE steers its colour weight by, and what a headless host needs to decide when to stop sampling.
 * The mean, every counter and mi3pt_debug_last_launch are bit-identical with moments on and off: the image is kept by moments-keeping
 * twins of the two accumulate kernels, in the same pass; the per-pixel kernel variants (1 / 2), which otherwise fold the accumulate
 * pass into the raytrace kernel, run the two passes separately while moments are on (same bits).
 * mi3pt_set_moments(1) allocates and zeroes the image (a context that never enables it allocates nothing and launches exactly what it
 * launched before); mi3pt_resize re-allocates and zeroes it while enabled; mi3pt_reset zeroes it; mi3pt_write_texture and
 * mi3pt_bind_accumulation (binding and un-binding) zero it (a mean that comes from outside has unknown spread -- mi3pt_write_moments
 * afterwards restores a checkpoint); mi3pt_set_moments(0) and
 * mi3pt_destroy free it.  Enable, disable and write launch the frame queue first.
 * mi3pt_read_moments (blocking) copies the image to dst, mi3pt_write_moments loads it from src (checkpoint / resume, like
 * mi3pt_write_texture): nbytes = rows x width x 16.  mi3pt_moments_device_ptr hands out the device image (zero copy; valid until the
 * next mi3pt_resize or mi3pt_set_moments; order your reads behind the context's stream or call mi3pt_sync first).
 *   MI3PT_ERR_STATE for read / write / ptr while disabled or before mi3pt_resize; MI3PT_ERR_INVALID for a wrong nbytes or a null pointer.
 * Tile split: this rank's compact rows (the update is pointwise).  Device group: mi3pt_set_moments goes to every member; read and ptr
 * GATHER the whole height x width image onto devices[0] like a feature image (the presenting context allocates its copy at the first
 * read, not before); mi3pt_write_moments is refused (MI3PT_ERR_STATE). ---- */
int mi3pt_set_moments(mi3pt_ctx *ctx, int enabled);                       /* default 0 */
int mi3pt_read_moments(mi3pt_ctx *ctx, void *dst, size_t nbytes);
int mi3pt_write_moments(mi3pt_ctx *ctx, const void *src, size_t nbytes);
int mi3pt_moments_device_ptr(mi3pt_ctx *ctx, void **dev_ptr, size_t *nbytes);

/* ---- MI3PT_GUIDED_VARIANCE: mi3pt_denoise_guided with the colour weight steered by the per-pixel variance of the mean -- the spatial
 * filter of SVGF (Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017), variance carried from level to level.  Needs
 * the moments image: MI3PT_ERR_STATE while mi3pt_set_moments is off -- on a context that has enabled it before; a context that has never
 * called mi3pt_set_moments(ctx, 1) answers as it did before the flag existed, MI3PT_ERR_INVALID for an unknown flag bit (the flag is
 * opt-in like the image; the message names mi3pt_set_moments).  Everything of mi3pt_denoise_guided's definition stands -- tap
 * order, the hit rule, en / ea / ep, the h weights, the division, the exp -- except the colour term and what follows.
 * One variance kernel per call, before the levels.  Per texel q of the moments image: s = (M2.r + M2.g) + M2.b;
 *   v(q) = fmax(s / (n * (n - 1)), 0) for n >= 2 (fp32, the division correctly rounded once, fmax drops a NaN), 0 for n < 2
 *   var_0(p) = (sum of g[dx] * g[dy] * v(q)) / (sum of g[dx] * g[dy])   over q = p + (dx, dy), dy = -1 .. 1 outer, dx = -1 .. 1 inner,
 *   g = [1/4, 1/2, 1/4], counting the q inside the image with hit(q) == hit(p) (the centre always counts)
 * -- the variance of the mean summed over rgb: |dc|^2 in expectation, up to a factor of 2.
 * Level i, with k_c = sigma_color * sigma_color in fp32 and denom = k_c * var_i(p) + MI3PT_GUIDED_VARIANCE_EPS for the centre p:
 *   ec = ((dc.x*dc.x + dc.y*dc.y) + dc.z*dc.z) / denom      (0 when sigma_color == 0; NO 4^i factor: the variance shrinks by itself)
 *   w as before;   nv = nv + (w * w) * var_i(q)   beside den and num;   var_(i+1)(p) = nv / (den * den)
 * Colour output as before, alpha included.  denom >= EPS > 0, so the exp's argument stays non-positive for finite inputs.
 * mi3pt_read_guided returns the colour image as before; mi3pt_read_guided_variance (blocking) the last level's variance var_levels:
 * nfloats = rows x width.  MI3PT_ERR_STATE unless the last filter since the last resize ran with the flag; MI3PT_ERR_INVALID for a null
 * pointer / a wrong nfloats.  A rank of a tile split and a device group stay refused as above.  MI3PT_PASS_GUIDED's time includes the
 * variance kernel. ---- */
#define MI3PT_GUIDED_VARIANCE 2u
#define MI3PT_GUIDED_VARIANCE_EPS 1e-8f
int mi3pt_read_guided_variance(mi3pt_ctx *ctx, float *dst, size_t nfloats);

/* ---- MI3PT_GUIDED_YOUNG: MI3PT_GUIDED_VARIANCE for an image whose texels differ in age -- after mi3pt_reproject, mi3pt_reproject_scene or
 * mi3pt_hold_history most texels carry a long history and the disoccluded ones restart at n = 1, where v = 0 and the filter leaves them
 * raw.  A texel with a short history takes its variance from a 7 x 7 neighbourhood, boosted for the short history (SVGF, section 4.2) --
 * here not from luminance moments but from the neighbours' own (M2, n), pooled exactly by Chan's pairwise rule.  Valid only together with
 * MI3PT_GUIDED_VARIANCE (alone: MI3PT_ERR_INVALID; on a context that never opted into moments it is an unknown bit like that one).
 * Everything of the variance mode stands except var_0; pinned arithmetic as there.  With (M2, n) = the moments texel, c = the colour
 * level 0 reads:   young(q) <=> n_q < MI3PT_GUIDED_YOUNG_COUNT (a NaN count is not young);   s_q = (M2.r + M2.g) + M2.b.
 * Centre p NOT young: var_0(p) as above, but a tap q of the 3 x 3 counts only if it is not young either (the centre always counts).  With
 *   no young texel in the image the bits are those of the variance mode without this flag.
 * Centre p young with n_p < 1 (never sampled): var_0(p) = 0.
 * Centre p young with n_p >= 1: taps q = p + (dx, dy), dy = -3 .. 3 outer, dx = -3 .. 3 inner.  A tap COUNTS iff q lies inside the image,
 *   hit(q) == hit(p) and n_q >= 1.  For each that counts, in that order, en / ea / ep exactly as in the level law (the centre's normal
 *   for pd), N, A, SS starting at 0:
 *     w  = exp(-((en + ea) + ep))              (the centre: 1; no h weights, no colour term)
 *     a  = w * n_q
 *     pass 1:  N = N + a;   A.k = A.k + a * c_q.k            then mu.k = A.k / N
 *     pass 2:  d = c_q - mu;   d2 = (d.x*d.x + d.y*d.y) + d.z*d.z;   SS = SS + w * (s_q + n_q * d2)
 *     v = N >= 2 ? fmax(SS / (N - 1), 0) : 0                 (fmax drops a NaN)
 *     var_0(p) = (v / n_p) * (MI3PT_GUIDED_YOUNG_COUNT / n_p)
 *   -- the per-sample variance of all the samples the counted neighbours hold, over the texel's own count, times SVGF's boost for a
 *   short history.  The var_0 of a young texel is not blurred.
 * Non-finite inputs give unspecified values; they neither hang nor fault.  Nothing is allocated beyond what the variance mode has; a rank of
 * a tile split and a device group stay refused; MI3PT_PASS_GUIDED's time includes the kernel. ---- */
#define MI3PT_GUIDED_YOUNG 4u
#define MI3PT_GUIDED_YOUNG_COUNT 4.0f

/* ---- the firefly pre-pass of mi3pt_denoise_guided: context state, not a flag bit (bit 8 and every higher bit stay MI3PT_ERR_INVALID).  A
 * few paths find a small bright light and leave single texels far above their neighbours; the colour weight isolates exactly those
 * texels and the filter keeps them.  While mi3pt_set_guided_despike(ctx, 1) holds, every mi3pt_denoise_guided -- any mode -- runs one
 * more kernel after the pack kernel and before the variance kernel and the levels, which scales such a texel down to the brightest
 * neighbour of its own class.  The accumulation image stays as it is: only the image handed to the filter changes.  Pinned arithmetic:
 * fp32, nothing contracted, correctly rounded division; a NaN is carried by the comparisons as written.  With c = the colour level 0 would
 * read, cls(q) = words 1 and 2 of IDS (material and hit flag):
 *   L(q) = ((c.r + c.g) + c.b) * (1.0f / 3.0f)
 *   taps q = p + (dx, dy), dy = -1 .. 1 outer, dx = -1 .. 1 inner, the centre left out.  A tap COUNTS iff q lies inside the image and
 *   cls(q) == cls(p) (both words);   m = the number of counting taps
 *   cap = 0;   for each counting tap, in that order: cap = fmaxf(cap, L(q))          (fmaxf drops a NaN; fmaxf(+0, -0) = +0: cap is never -0)
 *   p is CLAMPED iff m >= 1 && L(p) > cap:   s = cap / L(p);   c'(p).k = c(p).k * s  (k = r, g, b; the alpha channel keeps its bits)
 *   otherwise:                               s = 1;            c'(p) = c(p), bit for bit
 * Level 0 reads c' in c's place; so do MI3PT_GUIDED_YOUNG's c and the output's alpha rule.  Under MI3PT_GUIDED_VARIANCE, with or without
 * MI3PT_GUIDED_YOUNG, var_0 is taken exactly as there and then var_0(p) = var_0(p) * (s * s) for the clamped texels: the variance of a
 * scaled variable.  Nothing else of any mode's definition changes; an image in which no texel is clamped gives the bits of the same call
 * with the state off.  (A texel of a class of its own among its neighbours, m == 0, is left alone: a small emitter is not clamped against
 * the wall behind it.  L(p) = +inf over a finite cap gives s = 0: c'.k = NaN for an infinite channel k and 0 for a finite one -- finite channels
 * whose sum overflows give c' = 0.  Two texels with L = +inf beside each other are not clamped; a NaN L(p) is never clamped.)
 * The clamped texels are counted on the device, one vector atomic add per wave; mi3pt_read_guided_despiked (blocking) returns the count
 * of the last filter: MI3PT_ERR_STATE unless the last filter since the last resize ran with the state on, MI3PT_ERR_INVALID for a null
 * pointer.  One more rows x width x 16 B image (and 8 KiB of counter words) is allocated by the first filter that runs with the state on and
 * freed at mi3pt_resize / mi3pt_destroy; a context that never enables the state allocates and launches exactly what it did before.  The
 * pre-pass changes neither the accumulation, the moments, the feature images nor any counter; MI3PT_GUIDED_PRESENT draws from the filtered
 * image as before; a rank of a tile split and a device group stay refused by mi3pt_denoise_guided (the setter itself goes to every
 * member of a group); MI3PT_PASS_GUIDED's time includes the kernel.  MI3PT_ERR_INVALID for a null context. ---- */
int mi3pt_set_guided_despike(mi3pt_ctx *ctx, int enabled);           /* default 0 */
int mi3pt_read_guided_despiked(mi3pt_ctx *ctx, uint32_t *texels);    /* blocking: texels the last filter clamped */

/* ---- the per-tile error estimate of the running mean: when to stop sampling -- no counterpart in the reference, which renders a fixed
 * number of frames.  mi3pt_estimate_convergence reduces (accumulation image, moments image) on the device to one record per 8 x 8 tile
 * and a 40-byte summary; a host reads those instead of two whole images.  Pinned arithmetic as everywhere: fp32, round to nearest even,
 * nothing contracted, correctly rounded division.
 * Tile grid: 8 x 8 texels over the context's compact image, as mi3pt_host_sky_tiles lays them out: tiles_x = ceil(width / 8),
 * tiles_y = ceil(rows / 8), row-major; rows = this rank's local rows.
 * Per texel q, with c = the accumulation image as mi3pt_read_texture(MI3PT_TEX_ACCUMULATION) would return it (a bound image included)
 * and (M2, n) = its moments texel:
 *   counts(q) = q lies inside [0, width) x [0, rows) and n >= 1 (a NaN n does not count: texels the accumulate rectangle never touched)
 *   v(q) = the v of MI3PT_GUIDED_VARIANCE: fmax(((M2.r + M2.g) + M2.b) / (n * (n - 1)), 0) for n >= 2, else 0
 *   s = ((c.r + c.g) + c.b) * (1.0f / 3.0f);   m = s < 0 ? 0 : s   (fmax(s, 0) for every number s; a NaN s STAYS a NaN: a mean that is
 *   not a number must show in the verdict, not pass for black);   d = 1 + m;   d2 = d * d;   d4 = d2 * d2;   r(q) = v(q) / d4
 * -- the variance of the tone-mapped mean x / (1 + x) summed over rgb, to first order: the derivative of x / (1 + x) is 1 / (1 + x)^2,
 * taken at the texel's mean brightness.
 * Per tile: the 64 lanes are j = 8 * (row in tile) + (column in tile); a lane that counts holds sum r, count 1, n_min n, a lane that does
 * not holds sum 0, count 0, n_min +inf.
 *   sum_r: six halving rounds, a[j] = a[j] + a[j + s] for j < s, s = 32, 16, 8, 4, 2, 1 (a fixed tree: the sum is reproducible)
 *   max_r: fmaxf over 0 and the counting lanes' r (fmaxf drops a NaN: never a NaN, never below 0)
 *   n_min: fminf over the lanes;   count: an integer
 *   record: 4 x fp32 = (sum_r, max_r, (float)count, n_min); a tile with count 0 is (0, 0, 0, 0)
 * Verdict, for threshold (a target RMSE of the tone-mapped mean; finite, >= 0) and min_frames (0 .. 2^24), t2 = (threshold * threshold)
 * * 3.0f.  A tile with count > 0 is
 *   young      iff n_min < (float)min_frames  (a texel that has only seen black has zero variance: min_frames is the guard against that)
 *   above      iff young or !(sum_r <= t2 * (float)count)     (a NaN sum is above)
 *   nonfinite  iff sum_r is NaN or +-inf
 * Summary: every field is independent of the order in which the tiles are combined (integer sums, maxima of the bit patterns of
 * non-negative floats), so it is bitwise reproducible.  "Converged" is tiles > 0 && tiles_above == 0.  The image-wide RMSE estimate,
 * sqrt(sum over tiles of sum_r / (3 * texels)), is left to hosts, in double, from the tile map.
 * mi3pt_estimate_convergence launches the frame queue first, as mi3pt_denoise_guided does -- the estimate is of every frame submitted so
 * far -- and is asynchronous and stream ordered after that: two kernels, the summary's copy into pinned host memory, one event.  It
 * changes no image, no counter and nothing mi3pt_debug_last_launch / MI3PT_OPT_LAST_BUILD report; frames submitted afterwards accumulate
 * as if it had not been called.  The tile map and the summary are allocated by the first call and freed by mi3pt_resize / mi3pt_destroy
 * (a context that never calls it allocates nothing and launches exactly what it launched before).
 *   MI3PT_ERR_INVALID for a negative or non-finite threshold or min_frames outside 0 .. 2^24; MI3PT_ERR_STATE before mi3pt_resize or
 *   while mi3pt_set_moments is off.
 * mi3pt_read_convergence and mi3pt_read_convergence_tiles (nfloats = tiles_y x tiles_x x 4) block, but for THAT ESTIMATE'S EVENT only:
 * they do not launch the queue and do not wait for the stream, so frames submitted and flushed after the estimate keep running while
 * the host reads, and the values are those as of the estimate.
 *   MI3PT_ERR_STATE before the first estimate since the last resize; MI3PT_ERR_INVALID for a null pointer or a wrong nfloats.
 * With timing enabled, mi3pt_pass_time_us(MI3PT_PASS_CONVERGENCE) is the device time of the most recent estimate.
 * Tile split: the tiles of this rank's compact rows.  Device group: the estimate goes to every member; mi3pt_read_convergence combines the
 * members' summaries (counts add, max of max, min of min).  mi3pt_read_convergence_tiles returns the whole image's map, ceil(height / 8)
 * x tiles_x, when the group's block_rows is a multiple of 8 -- assembled on the host, member `rank`'s local tile row t at tile row
 * mi3pt_tile_global_row(t, rank, n, block_rows / 8) -- and is MI3PT_ERR_STATE otherwise. ---- */
typedef struct mi3pt_convergence {
    uint32_t tiles, tiles_above, tiles_young, tiles_nonfinite;  /* tiles: those with count > 0 */
    uint64_t texels;                                            /* sum of counts */
    float worst_tile;    /* fmaxf over counted tiles of sum_r / (float)count; 0 when none */
    float worst_texel;   /* fmaxf over tiles of max_r */
    float n_min;         /* fminf over counted tiles; 0 when none */
    float threshold;     /* as given */
} mi3pt_convergence;     /* 40 bytes */
int mi3pt_estimate_convergence(mi3pt_ctx *ctx, float threshold, int min_frames);
int mi3pt_read_convergence(mi3pt_ctx *ctx, mi3pt_convergence *out);
int mi3pt_read_convergence_tiles(mi3pt_ctx *ctx, float *dst, size_t nfloats);  /* tiles_y x tiles_x x 4 */

/* ---- adaptive sampling: stop sampling the tiles that have converged -- no counterpart in the reference.  The error estimate above says
 * which tiles are done; the sample mask stops them from being traced and accumulated.
 * The sample mask: one byte per 8 x 8 tile of the context's compact image, on the grid of mi3pt_estimate_convergence (tiles_x =
 * ceil(width / 8), tiles_y = ceil(rows / 8), row-major, rows = local rows).  Non-zero = sampled, zero = frozen.  Default: no mask,
 * every tile sampled; a context that never sets one allocates nothing new and launches exactly what it launched before (same kernels,
 * grids, counters, mi3pt_debug_last_launch, MI3PT_OPT_LAST_BUILD).
 * What the mask changes: while one is set, an accumulate step touches the texels of sampled tiles only -- queued sample frames, the
 * immediate path of mi3pt_submit and an ACCUMULATE-only submit alike.  A frozen tile's accumulation texels and moments texels keep
 * their bits.  The arithmetic of a sampled texel is unchanged: the same operations in frame order, the weight taken from the accumulate
 * block's `frame` as always.  Hence, if tiles are only ever frozen between resets, every texel equals, bit for bit, the unmasked run's
 * texel after the last frame its tile was sampled in -- mean and moments, F32 and F16 storage, a bound image.  A tile that is thawed
 * again continues with the uniform's weight 1 / frame although it has seen fewer samples: the result is then the law's weighted mean,
 * NOT the sample mean (under mi3pt_set_mean_by_count it continues as a sample mean).  The hosts only ever freeze.
 * What the mask saves: queued RAYTRACE | ACCUMULATE frames trace only the sampled tiles wherever the launch can take a tile list (the
 * state-machine kernel's lean build of variants 9 - 14, without a cost order); the view's empty tiles among them are shaded by the
 * streaming sky kernel as without a mask.  There MI3PT_CNT pixels, rays and misses count the sampled tiles' in-bounds pixels only and
 * the radiance slots of frozen tiles are not written.  On every other route (variants 1 - 8, the per-pixel kernels, RAYTRACE without
 * ACCUMULATE) every tile is traced as before and the accumulate step alone applies the mask; the per-pixel variants 1 / 2 run their two
 * passes unfused while a mask is set, as they do for moments.  The image is the same on every route.  With no tile sampled a queued
 * launch enqueues no raytrace, sky or accumulate kernel.  The ordered mean's work falls with the sampled tiles on every route.
 * Life time: mi3pt_resize and mi3pt_reset drop the mask -- a new accumulation starts whole.  mi3pt_write_texture,
 * mi3pt_bind_accumulation and mi3pt_set_moments leave it.  Setting or changing the mask launches the frame queue first, under the old
 * mask, and does not wait for the stream.
 *   mi3pt_set_sample_mask(tiles, ntiles): ntiles = tiles_y x tiles_x; (NULL, 0) removes the mask.
 *   mi3pt_read_sample_mask: the mask as 0 / 1 bytes (no mask: all 1) and the number of sampled tiles.  Host state: no wait.
 *   mi3pt_freeze_converged(guard): waits for the last estimate's event only, exactly as mi3pt_read_convergence_tiles does; applies
 *     mi3pt_host_freeze_tiles to that estimate's tile records, with that estimate's threshold and min_frames, and to the current mask
 *     (all ones if none); installs the result as by mi3pt_set_sample_mask; *sampled_out = the tiles still sampled.
 *   mi3pt_host_freeze_tiles: the rule, plain host code, no device.  records = tiles_y x tiles_x x (sum_r, max_r, count, n_min).  With
 *     above(t) exactly the verdict above (young or !(sum_r <= t2 * (float)count), t2 = (threshold * threshold) * 3.0f):
 *       under(t) = count(t) > 0 && !above(t)
 *       a tile with count == 0 is frozen at once: it has nothing to sample
 *       a sampled tile with count > 0 is frozen iff under(t) and, for guard == 1, under(u) || count(u) == 0 for each of its up to eight
 *       neighbours u inside the map -- the ring keeps a converged tile sampling while a neighbour is still noisy, which hides tile borders
 *       an already frozen tile stays frozen: the function never thaws.  guard is 0 or 1.
 *     The ring reads the verdicts of ALL neighbours, frozen ones included: a tile that was frozen on an older estimate and reads above in this
 *     one (a host that applies a decision one chunk late, renderUntil's lookahead) keeps its neighbours sampling for as long as it does.
 *   MI3PT_ERR_INVALID for a wrong ntiles, a null pointer where one is needed, or guard outside 0 / 1; MI3PT_ERR_STATE before
 *   mi3pt_resize, and for mi3pt_freeze_converged before the first estimate since the last resize.
 * Tile split: the mask is over this rank's compact rows, and the guard ring is taken over that compact map: across a block boundary
 * these are NOT the image's neighbours.  A host that wants the image's ring gathers the ranks' maps, applies mi3pt_host_freeze_tiles
 * to the whole map and hands each rank its rows with mi3pt_set_sample_mask.
 * Device group: the three context calls take and return the WHOLE image's map, ceil(height / 8) x tiles_x, when the group's block_rows
 * is a multiple of 8 -- assembled and scattered on the host by the row rule of mi3pt_read_convergence_tiles -- and are MI3PT_ERR_STATE
 * otherwise; the group's mi3pt_freeze_converged applies the rule to the whole map, so its ring is the image's. ---- */
int mi3pt_set_sample_mask(mi3pt_ctx *ctx, const uint8_t *tiles, size_t ntiles);   /* NULL, 0: no mask */
int mi3pt_read_sample_mask(mi3pt_ctx *ctx, uint8_t *dst, size_t ntiles, uint32_t *sampled_out);  /* no mask: all 1 */
int mi3pt_freeze_converged(mi3pt_ctx *ctx, int guard, uint32_t *sampled_out);
int mi3pt_host_freeze_tiles(const float *records, int tiles_x, int tiles_y, float threshold, int min_frames,
                            int guard, uint8_t *mask_inout, uint32_t *sampled_out);   /* plain host C++, no device */

/* ---- the mean by count: a running mean whose weight comes from the texel's OWN sample count -- no counterpart in the reference, whose
 * weight is 1 / frame for every texel (accumulate.wgsl:18-28).  Off by default; a context that never enables it launches exactly what it
 * launched before (the two existing instantiations of each accumulate kernel are untouched; the mode runs a third).  Needs the moments
 * image, whose n IS the count: MI3PT_ERR_STATE while mi3pt_set_moments is off, and mi3pt_set_moments(ctx, 0) switches the mode off too.
 * Both calls launch the frame queue first (queued frames accumulate under the law they were submitted under).
 * While the mode is on, EVERY accumulate step of a texel inside the accumulate block's rectangle -- queued frames, the immediate path of
 * mi3pt_submit, an ACCUMULATE-only submit, with and without a sample mask -- is, with p the mean, (M2, n) the moments texel, c the
 * radiance, fp32, nothing contracted, the division correctly rounded:
 *   restart = (enabled != 1) || !(n >= 1.0f)              a NaN, zero or negative n restarts
 *   weight  = restart ? 1.0f : 1.0f / (n + 1.0f)
 *   p'      = the stored mix(p, c, weight) = p * (1 - weight) + c * weight, rounded to binary16 under MI3PT_STORAGE_F16 -- as always
 *   restart:   M2.k = 0;   n = 1
 *   otherwise: M2.k = M2.k + (c.k - p.k) * (c.k - p'.k);   n = n + 1
 * The accumulate block's `frame` does not enter the step (the raytrace block's `frame` still seeds the samples).  Hence:
 *   - after mi3pt_reset (n = 0 everywhere) N steps give the SAMPLE MEAN, bit-identical -- mean and moments, F32 and F16 storage -- to
 *     the default law run with the accumulate `frame` = 1, 2, ..., N;
 *   - a tile that is frozen by a sample mask and thawed again continues as a sample mean (the default law does not, see above);
 *   - mi3pt_write_texture and mi3pt_bind_accumulation zero the moments, so the next step RESTARTS every texel from the frame's radiance:
 *     follow them with mi3pt_write_moments to resume a checkpoint;
 *   - both hosts start their accumulate `frame` at 2 (renderer.ts:369-377), so their default mean after N frames is N / (N + 1) of the
 *     sample mean (the first step mixes with the zeroed image at weight 1 / 2); a by-count image is BRIGHTER by (N + 1) / N.
 * The per-pixel kernel variants (1 / 2) run their two passes unfused, as they do whenever moments are on.  Tile split: the step is
 * pointwise.  Device group: the call goes to every member. ---- */
int mi3pt_set_mean_by_count(mi3pt_ctx *ctx, int enabled);                  /* default 0 */

/* ---- reprojection: carry the running mean and its moments across a camera move -- no counterpart in the reference, whose hosts reset
 * on every camera change (renderer.ts:397-416).  The temporal half of SVGF (Schied et al. 2017): every texel of the NEW view looks its
 * first hit's world point up in the OLD view's images and takes over mean, variance and sample count where the old view saw the same
 * surface.  The scene is taken as STATIC between the two views; uploads in between are not detected (taps are then rejected or carry
 * stale radiance; nothing faults); mi3pt_reproject_scene below follows triangles that moved.
 * mi3pt_host_view_frame (plain host C++, no device): the camera frame the reprojection projects with, from a 96-byte raytrace block,
 * computed in double from the block's fp32 fields, each output rounded to fp32 once:
 *   w = normalize(-direction);  up = (0,1,0), or (0,0,1) when |w.y| > 0.99999;  u = normalize(cross(up, w));  v = cross(w, u)
 *   t = tan(fov * pi / 360);  r = aspect * t;  fwd = -w
 *   out = position.xyz, aspect,  fwd.xyz, t,  u.xyz, r,  v.xyz, 0
 * (cameraToRay's frame, raytrace.wgsl:217-236; it need not equal the ray generator's fp32 frame bit for bit -- an ulp of t moves a
 * reprojected coordinate by 1e-6 texels -- it is an INPUT of the pinned arithmetic below.)  MI3PT_ERR_INVALID for a wrong nbytes, a
 * null pointer, a zero or non-finite direction, a fov outside (0, 180), a non-finite position.
 * State: the context remembers the raytrace block each feature image was rendered from.  The OLD view U0 is the block of POSITION,
 * NORMAL and IDS as they stand -- the caller rendered them in the view the mean was sampled in; the NEW view U1 is the raytrace block
 * at the call.  mi3pt_reproject, in order:
 *   1 launches the frame queue;  2 F0 = mi3pt_host_view_frame(U0);  3 makes the three old feature images the "previous set" (a swap of
 *   pointers with a second set of three images, allocated by the first call and freed by mi3pt_resize / mi3pt_destroy);  4 renders all
 *   four feature images from U1 exactly as mi3pt_render_aovs(ctx, 15) -- the de-noiser finds them current;  5 runs the kernel below from
 *   (A, M) = (accumulation image, moments image) into a scratch pair;  6 makes the scratch pair the accumulation and moments images: a
 *   swap of pointers where the image is the context's own, a copy on the stream into memory bound by mi3pt_bind_accumulation;  7 drops
 *   the sample mask, as mi3pt_reset does.
 * Asynchronous and stream ordered.  It changes no counter and nothing mi3pt_debug_last_launch / MI3PT_OPT_LAST_BUILD report.  Because
 * of the swaps, pointers handed out earlier by mi3pt_accumulation_device_ptr (of the context's own image), mi3pt_moments_device_ptr and
 * mi3pt_aov_device_ptr name other images afterwards: ask again.
 * The kernel.  Pinned fp32: dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, correctly rounded division, nothing contracted.  Index 1: the new
 * features, index 0: the previous set; hit = word 2 of IDS, mat = word 1.  For every texel p = (x, y) of the image inside the
 * accumulate block's rectangle:
 *   carry needs hit1(p) == 1;   P = POSITION1(p).xyz;  t1 = POSITION1(p).w;  N = NORMAL1(p).xyz
 *   d = P - F0.position;  a = dot(d, F0.u);  b = dot(d, F0.v);  cz = dot(d, F0.fwd);      needs cz > 0
 *   k = F0.aspect / cz;   uvx = (a * k + F0.r) / (F0.r + F0.r);   uvy = (b * k + F0.t) / (F0.t + F0.t)
 *   fx = uvx * U0.resolution.x;  fy = uvy * U0.resolution.y;   needs fx > -1 && fx < width && fy > -1 && fy < rows   (a NaN fails)
 *   x0 = floorf(fx);  tx = fx - x0;  wx = [1 - tx, tx];   y0, ty, wy likewise
 *   taps q = (x0 + i, y0 + j), j = 0, 1 outer, i = 0, 1 inner, bw = wx[i] * wy[j].  A tap COUNTS iff
 *       q lies inside the rectangle and the image,  bw > 0,  hit0(q) == 1,  mat0(q) == mat1(p),
 *       n0 = M(q).w >= 1                       (a NaN does not count)
 *       dot(N, NORMAL0(q).xyz) >= normal_cos_min
 *       fabsf(dot(N, POSITION0(q).xyz - P)) <= plane_tolerance * t1
 *     for each that counts, in that order:
 *       ws = ws + bw;   col.k = col.k + bw * A(q).k;   nmin = fminf(nmin, n0)       (ws, col, var start at 0, nmin at +inf)
 *       var.k = var.k + bw * (n0 >= 2 ? fmaxf(M2(q).k / (n0 - 1), 0) : 0)
 *   carried (ws > 0):   n' = fminf(nmin, (float)max_history)
 *                       A'(p) = (stored col.k / ws, 1)                 (rounded to binary16 under MI3PT_STORAGE_F16)
 *                       M'(p) = ((var.k / ws) * (n' - 1), n')
 *   restarted (a "needs" failed, or no tap counted):   A'(p) = (0, 0, 0, 1);   M'(p) = (0, 0, 0, 0)
 * Texels outside the rectangle keep their bits.  The cap by max_history keeps the per-sample variance and shortens the history: new
 * samples then take over from reprojected ones, which are exact for diffuse surfaces and biased for glossy ones (their radiance
 * depends on the direction they are seen from).  Misses restart: a texel that sees the environment directly has next to no variance.
 * Non-finite inputs give unspecified values; every index is range-checked before it is used, so they neither hang nor fault.  The
 * un-jittered pinhole ray defines the features: with aperture > 0 the carried mean is that of the in-focus surface.
 * Afterwards everything works in the new view unchanged: under mi3pt_set_mean_by_count sampling continues per texel -- a restarted texel
 * (n = 0) takes its first frame at weight 1 --, mi3pt_estimate_convergence sees disoccluded tiles as young, MI3PT_GUIDED_VARIANCE filters
 * with the carried variance.
 *   MI3PT_ERR_STATE before mi3pt_resize; while moments or the mean by count are off; unless POSITION, NORMAL and IDS have all been
 *   rendered since the last resize, from blocks whose resolution, aspect and camera fields are bitwise equal; unless U1's resolution
 *   equals U0's bitwise; for a rank of a tile split with more than one rank and for a device group (taps cross rows; the halo exchange
 *   is NOT BUILT).  MI3PT_ERR_INVALID for a null pointer, a plane_tolerance that is negative or not finite, normal_cos_min outside
 *   [-1, 1], max_history outside 1 .. 2^24, non-zero flags.
 * With timing enabled, mi3pt_pass_time_us(MI3PT_PASS_REPROJECT) is the device time of the kernel and the copy of the most recent call;
 * the feature render inside it is timed as MI3PT_PASS_AOV. ---- */
typedef struct mi3pt_reproject_params {
    float plane_tolerance;   /* finite, >= 0; relative to the new texel's hit distance */
    float normal_cos_min;    /* in [-1, 1] */
    int   max_history;       /* 1 .. 2^24 */
    unsigned flags;          /* 0 */
} mi3pt_reproject_params;
int mi3pt_host_view_frame(const void *raytrace_uniforms, size_t nbytes, float out[16]);   /* plain host C++, no device */
int mi3pt_reproject(mi3pt_ctx *ctx, const mi3pt_reproject_params *params);

/* ---- reprojection across a scene change: the mean follows triangles that moved -- no counterpart in the reference.  mi3pt_reproject
 * takes the scene as static; a host that nudges one object or plays an animation would lose every sample of every texel, the large
 * majority whose surface did not move included.  The motion-vector half of SVGF: word 0 of IDS names the hit triangle, the context
 * keeps the records in upload order, so a texel of the new view can find the point of the PREVIOUS geometry it shows now.
 * Topology is the caller's contract: index i names the same surface element before and after the upload (both hosts flatten their
 * scene in a fixed order: rigid motion and skinning satisfy this).
 * mi3pt_keep_geometry(ctx, 1): the triangle records as they are uploaded NOW are the "previous geometry" from here on.  No second
 * upload and no copy: until the next mi3pt_upload_triangles "previous" aliases "current"; that upload hands the current buffer over
 * as the previous geometry instead of freeing it; later uploads replace the current records only.  The context records its upload
 * count (every mi3pt_upload_triangles / _bvh / _materials counts) at the call and at every mi3pt_render_aovs, per image.  A later
 * keep = 1 replaces what is kept; keep = 0, mi3pt_destroy or a second keep free a handed-over buffer, after a wait for the context's
 * stream.  COST: 112 B per triangle of device memory from the hand-over until the release.  MI3PT_ERR_STATE without uploaded
 * triangles (keep = 1) and for a device group.
 * mi3pt_reproject_scene: steps 1 - 7 of mi3pt_reproject unchanged, with the kernel below in step 5; the feature images of step 4 are
 * rendered from U1 and the CURRENT scene.  U1 may equal U0: a moved object under a fixed camera.  Asynchronous and stream ordered; it
 * changes no counter and nothing mi3pt_debug_last_launch reports; timed as MI3PT_PASS_REPROJECT, its feature render as MI3PT_PASS_AOV.
 * The kernel.  Pinned fp32: dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, correctly rounded division and sqrtf, nothing contracted.  For a
 * texel p inside the rectangle with hit1(p) == 1:
 *   T = word 0 of IDS1(p);   needs 0 <= T < ntris;   R1 = the current record T, R0 = the kept record T
 *   P, t1, N as in mi3pt_reproject
 *   static: the nine position floats of R0 and R1 are equal as 32-bit words.  Then  Q = P;  NQ = N;  len = 1;  tq = t1
 *   moved, with a1, b1, c1 the positions of R1 and a0, b0, c0, na0, nb0, nc0 the positions and normals of R0:
 *     e1 = b1 - a1;  e2 = c1 - a1;  w = P - a1
 *     d11 = dot(e1,e1);  d12 = dot(e1,e2);  d22 = dot(e2,e2);  w1 = dot(w,e1);  w2 = dot(w,e2)
 *     den = d11*d22 - d12*d12                                                                needs den > 0   (a NaN fails)
 *     u = (d22*w1 - d12*w2) / den;   v = (d11*w2 - d12*w1) / den;   g = (1 - u) - v
 *     f1 = b0 - a0;  f2 = c0 - a0;   Q.k = a0.k + (u*f1.k + v*f2.k)
 *     NQ.k = (g*na0.k + u*nb0.k) + v*nc0.k;   len = sqrtf(dot(NQ,NQ))                          needs len > 0   (a NaN fails)
 *     d = Q - F0.position;   tq = sqrtf(dot(d,d))
 *   From there the law is mi3pt_reproject's with Q in P's place in d, a, b, cz, k, uvx, uvy, fx, fy and the taps, and the two surface
 *   tests of a tap read
 *       dot(NQ, NORMAL0(q).xyz) >= normal_cos_min * len
 *       fabsf(dot(NQ, POSITION0(q).xyz - Q)) <= (plane_tolerance * tq) * len
 *   hit0(q) == 1, mat0(q) == mat1(p), n0 >= 1, the tap order and the sums are unchanged.
 *   carried:   n' = fminf(nmin, (float)(static ? max_history : max_history_moved));   A', M' as in mi3pt_reproject
 *   restarted texels and texels outside the rectangle: as in mi3pt_reproject.
 * With len = 1 both products are exact: a static texel is mi3pt_reproject's texel bit for bit, by construction.
 * Known limits.  A needle triangle loses precision in den: its taps then fail the plane test or land a fraction of a texel off.
 * Radiance that changed because a shadow or a reflection moved is carried stale: max_history and max_history_moved bound for how long.
 *   MI3PT_ERR_STATE wherever mi3pt_reproject returns it (a rank of a tile split and a device group included); while no geometry is
 *   kept; when the kept triangle count differs from the current one; unless POSITION, NORMAL and IDS were all rendered at exactly the
 *   kept upload count -- any upload between rendering them and mi3pt_keep_geometry (in either order) refuses the call; "keep, then
 *   render them, no upload in between" is accepted.  MI3PT_ERR_INVALID for mi3pt_reproject's argument faults and max_history_moved
 *   outside 1 .. 2^24. ---- */
int mi3pt_keep_geometry(mi3pt_ctx *ctx, int keep);          /* 1: remember the triangle records as they are uploaded NOW as the
                                                               "previous geometry"; 0: release it */
typedef struct mi3pt_reproject_scene_params {
    float plane_tolerance;     /* finite, >= 0 */
    float normal_cos_min;      /* [-1, 1] */
    int   max_history;         /* 1 .. 2^24: cap for texels whose triangle did not move */
    int   max_history_moved;   /* 1 .. 2^24: cap for texels whose triangle moved */
    unsigned flags;            /* 0 */
} mi3pt_reproject_scene_params;
int mi3pt_reproject_scene(mi3pt_ctx *ctx, const mi3pt_reproject_scene_params *params);

/* ---- a held history, validated against fresh samples before it is merged -- no counterpart in the reference.  Both reprojections merge
 * what they carry into the live mean at once; radiance that changed although the surface did not (a repainted material, a dimmed
 * environment, a shadow that moved) then stays in the picture until new samples outweigh the carried ones.  The temporal validation of
 * an SVGF-style loop: set the carried mean ASIDE, sample a few frames of the scene as it is now, and merge per texel only as much of
 * the carried history as a two-sample test of "fresh mean against carried mean" supports.  The moments image holds the per-sample
 * variance of both sides, so the test needs no new input.
 * mi3pt_hold_history, in order:  1 launches the frame queue;  2 makes the accumulation and moments images the HELD pair (a second pair
 * of images, allocated by the first call and freed by mi3pt_resize / mi3pt_destroy): a swap of pointers where the image is the
 * context's own, a copy on the stream out of memory bound by mi3pt_bind_accumulation;  3 leaves the live accumulation and moments
 * images zero-filled, as mi3pt_reset leaves them.  Output, canvas, feature images, sample mask and counters are untouched; under the
 * mean by count every texel restarts with its next frame.  Called after mi3pt_reproject / mi3pt_reproject_scene, or at any time; a
 * second hold replaces the first.  mi3pt_reset, mi3pt_resize, mi3pt_reproject, mi3pt_reproject_scene, mi3pt_set_moments(ctx, 0) and
 * mi3pt_destroy DROP a held history (the reprojections: when they pass their checks); nothing else about them changes.
 * mi3pt_merge_history, in order:  1 launches the frame queue;  2 runs the kernel below from the live pair (A, M) and the held pair
 * (Ah, Mh) into mi3pt_reproject's scratch pair;  3 makes the scratch pair the accumulation and moments images as step 6 of
 * mi3pt_reproject does;  4 marks the history as no longer held.
 * Both are asynchronous and stream ordered, change no counter and nothing mi3pt_debug_last_launch / MI3PT_OPT_LAST_BUILD report.
 * Because of the swaps, pointers handed out earlier by mi3pt_accumulation_device_ptr (of the context's own image) and
 * mi3pt_moments_device_ptr name other images after either call: ask again.
 * The kernel.  Pinned fp32: correctly rounded division, nothing contracted, fmaxf / fminf return the other operand for a NaN;
 * r = radius.  Live texel (a, .) = A(q), (m2, n) = M(q); held texel (ah, .) = Ah(q), (m2h, nh) = Mh(q).
 *   pair(q) iff q lies inside the image and the accumulate block's rectangle, and n >= 1 && nh >= 1        (a NaN fails)
 *   var(m2, n).k = n >= 2 ? fmaxf(m2.k / (n - 1), 0) : 0
 * For every texel p = (x, y) inside the rectangle, D = V = 0, then for dy = -r .. r outer, dx = -r .. r inner, q = (x + dx, y + dy), the
 * taps with pair(q) in that order:
 *       sf = var(m2, n);   sh = var(m2h, nh);   w = 1 / n + 1 / nh
 *       D.k = D.k + (a.k - ah.k);   V.k = V.k + fmaxf(sf.k, sh.k) * w
 *   z.k = (D.k * D.k) / (V.k + MI3PT_HISTORY_EPS);   z2 = fmaxf(fmaxf(z.x, z.y), z.z)
 *   drop2 = z_drop * z_drop;   keep2 = z_keep * z_keep;   lam = fminf(fmaxf((drop2 - z2) / (drop2 - keep2), 0), 1)
 *   nk = floorf(nh(p) * lam)
 *   dropped   (n(p) >= 1 and: !(nh(p) >= 1), or !(nk >= 1)):    A'(p) = A(p);   M'(p) = M(p)
 *   only held (!(n(p) >= 1) and nh(p) >= 1):                     A'(p) = Ah(p);  M'(p) = Mh(p)
 *   neither   (!(n(p) >= 1) and !(nh(p) >= 1)):                  A'(p) = A(p);   M'(p) = M(p)
 *   merged, with d.k = ah.k - a.k and sh = var(m2h, nh) at p:
 *       N = n + nk;   f = nk / N
 *       A'(p) = (stored a.k + d.k * f, 1)                          (rounded to binary16 under MI3PT_STORAGE_F16)
 *       M'(p) = ((m2.k + sh.k * (nk - 1)) + (d.k * d.k) * (n * f), N)
 * Texels outside the rectangle keep their bits.  z2 is the largest squared z-score of the pooled difference among the channels;
 * at or below z_keep the whole held history is kept, at or above z_drop none of it, a share linear in z2 in between.  The merge is
 * Chan's pairwise combine of the live samples with nk samples of the held mean and the held per-sample variance: a shortened history
 * keeps its variance, as max_history does, and counts stay whole numbers.  A z_drop whose square overflows gives lam = 0 (everything
 * dropped); so do squares that round to the same number, except that a texel whose pooled difference is exactly 0 (z2 = 0, the quotient
 * +inf) gets lam = 1 unless both squares are 0.  Non-finite inputs give unspecified values; every index is range-checked before it is
 * used, so they neither hang nor fault.
 *   MI3PT_ERR_STATE before mi3pt_resize; while moments or the mean by count are off; for a rank of a tile split with more than one
 *   rank and for a device group (a window crosses rows; the halo exchange is NOT BUILT); mi3pt_merge_history also while nothing is
 *   held.  MI3PT_ERR_INVALID for a null pointer, a radius outside 0 .. 3, a z_keep that is negative or not finite, a z_drop that is
 *   not finite or not above z_keep, non-zero flags.
 * With timing enabled, mi3pt_pass_time_us(MI3PT_PASS_HISTORY) is the device time of the kernel and the copy of the most recent
 * mi3pt_merge_history.  NOT BUILT: a host that reads the test's verdict without merging. ---- */
#define MI3PT_HISTORY_EPS 1e-8f
typedef struct mi3pt_history_params {
    int   radius;     /* 0 .. 3: the test pools (2*radius+1)^2 texels */
    float z_keep;     /* finite, >= 0: at or below it the whole carried history is kept */
    float z_drop;     /* finite, > z_keep: at or above it none of it is */
    unsigned flags;   /* 0 */
} mi3pt_history_params;
int mi3pt_hold_history(mi3pt_ctx *ctx);
int mi3pt_merge_history(mi3pt_ctx *ctx, const mi3pt_history_params *params);

/* ---- read-back (the capability a headless drop-in needs; the reference only has
 * canvas.toDataURL, main.ts:351-356).  Blocking.  dst holds rows x width x 4 floats
 * (rows = local rows for OUTPUT / ACCUMULATION, canvas height for CANVAS). ---- */
int mi3pt_read_texture(mi3pt_ctx *ctx, int which /* mi3pt_texture */, float *dst, size_t nfloats);
int mi3pt_read_canvas_rgba8(mi3pt_ctx *ctx, uint8_t *dst, size_t nbytes);
/* Host -> device: load a running mean into the accumulation image (which = ACCUMULATION or
 * OUTPUT; both name the same image after an accumulate pass, accumulate.ts:171-175).  For
 * checkpoint / resume and for presenting a gathered multi-GPU image from a 1-rank context. */
int mi3pt_write_texture(mi3pt_ctx *ctx, int which /* mi3pt_texture */, const float *src, size_t nfloats);

/* Device pointer of the accumulation image (local_rows x width x 4 fp32), for
 * zero-copy hand-off to a collective (RCCL gather of the HDR buffer). */
int mi3pt_accumulation_device_ptr(mi3pt_ctx *ctx, void **dev_ptr, size_t *nbytes);
/* Use caller-owned device memory (e.g. a torch tensor) as the accumulation image;
 * nbytes must equal local_rows*width*16.  NULL returns to the internal buffer. */
int mi3pt_bind_accumulation(mi3pt_ctx *ctx, void *dev_ptr, size_t nbytes);

/* ---- timing: TimingHelper / RollingAverage, timing.ts:28-146, pass.ts:22-26.
 * GPU time of the pass in the most recent completed submit, microseconds
 * (hipEvent pair on the context's stream).  Off by default; enabling costs one
 * event pair per pass per submit. ---- */
int mi3pt_enable_timing(mi3pt_ctx *ctx, int enabled);
int mi3pt_pass_time_us(mi3pt_ctx *ctx, int pass, float *microseconds);
/* With timing enabled: GPU time summed over the batched raytrace launches since the last
 * reset (HIP event pairs on the stream each kernel ran on), their number, and the frames
 * they covered.  Waits for the launches in flight. */
int mi3pt_raytrace_launch_stats(mi3pt_ctx *ctx, int reset, double *total_ms, uint64_t *launches, uint64_t *frames);
/* GPU-clock span from the start of the first to the end of the last of those launches.  Launches
 * overlap at their tails, so span / launches (not total_ms / launches) is what a launch costs. */
int mi3pt_raytrace_launch_span(mi3pt_ctx *ctx, double *span_ms);

/* ---- counters (roofline inputs) ---- */
int mi3pt_get_counters(mi3pt_ctx *ctx, uint64_t out[MI3PT_CNT_COUNT]);
int mi3pt_reset_counters(mi3pt_ctx *ctx);

/* Kernel variant (0 .. 14): 0 = auto, 1 = per-pixel kernel walking the uploaded records,
 * 2 = per-pixel kernel walking node packets, 3 = persistent waves with lane refill,
 * 4 = persistent per-lane state machine (the default), 5 = 4 with a walk threshold of 48,
 * 6 = 4 with the top 32 node packets staged in LDS (measured: no gain),
 * 7 = 4 with leaf tests deferred into triangle steps of their own; needs a proper tree whose
 * worst-case stack stays below 29 entries (checked at upload), otherwise 4 runs; 8 = 7 with the
 * LDS-staged top of the tree of 6 (measured: no gain); 9 = 7 with exact-image distance culling: a
 * child box that starts farther away than the closest hit so far, by a margin PROVEN to cover the
 * rounding of the reference's fp32 Moller-Trumbore code, is skipped, children are
 * visited near first -- the image is bit-identical, the box / triangle-test COUNTERS are lower than
 * the reference walk's (which has no such bound, raytrace.wgsl:118-203); 10 = 9 on 4-ary "wide" packets
 * (internal children absorbed into their parent where boxes nest: the same leaves are reached -- the
 * fp32 slab test is monotone under nesting -- in half the node steps).  9 and 10 need a proper tree whose
 * order-independent worst-case stack fits 56 entries.
 * 11 = 10 with the FILTERED slab test in the shipped batched launch: each box is decided from approximate quotients
 * (one multiplication instead of an exact division each) whenever the two ends of the approximate interval lie more
 * than 2^-21 (relative) apart, which PROVES the reference's decision (csrc/pt_kernels.hip slab_q0; tests/test_slab_filter.py);
 * any other box runs the exact test.  12 = 11 with the culling condition evaluated on one axis only (cheaper, skips
 * less).  11 and 12 exist in the experiment build only (superseded by 13; a release library runs 10 for them).
 * 13 = THE SHIPPED WALK (round 4): 10 on COMPRESSED wide packets -- 64 bytes per 4-ary node: a grid origin, three cell exponents
 * and the four child boxes as 8-bit cell indices rounded OUTWARD by at least one cell -- and 64-byte triangle records that carry
 * the leaf's own box as uploaded.  Above the leaves a box test only has to never reject what the reference's exact test passes
 * (boxes nest: a leaf that passes has every ancestor pass), so the node step runs a conservative test on the decoded planes
 * (one v_cvt_f32_ubyte + one fma per quotient); the leaf's own box is tested EXACTLY in the triangle step, and only leaves that
 * pass it count as triangle tests.  Half the bytes and half the loads of 10 per node step.  Instantiations: culling condition
 * (one axis / three axes, chosen per scene like 12 / 11) x walk threshold (32 lanes; 44 for very large trees) x waves per SIMD (six:
 * 80 registers, for launches of >= 1.5 M jobs; five: 96 registers; MI3PT_OPT_SIX_WAVES).
 * Needs every box of the tree nested in its parent's and finite (any tree of the reference's builder); otherwise 10 runs.
 * 14 = the EIGHT-wide walk (round 6; measured, NOT the default -- profiles/r06_a_ab_eight_wide.log): 13's conservative test on 80-byte packets
 * of up to eight children whose slots are chosen by position, so that `slot ^ octant of the ray's direction signs` is a front-to-back
 * order: a node step leaves two 8-bit hit masks, pushes at most ONE 64-bit node entry (first child packet, hits in visiting order,
 * internal-slot mask) and ONE 32-bit leaf entry (record base, hit slots) and pops the nearest child by a find-first-bit -- no sort,
 * no per-child references, a stack of one entry per tree level.  26 % fewer dependent node steps per ray, 47 % more box tests,
 * 1.4 x the instructions per step: -2 .. -5 % on the 870 k-triangle scene, -25 % on the 10 M-triangle forest.  Same bits (the
 * grouping of the reference tree's nodes into packets is free: only the leaves' own boxes decide what is tested).  Falls back to 13
 * where its packets could not be built (a tree more than 30 packet levels deep, more than 2^24 packets or records).
 * Every reference-legal setting (samplesPerFrame 1 .. 2^24, maxBounces 0 .. 65535, F16 storage, pipelining off) runs this
 * kernel; launches beyond those packing limits run the per-pixel kernel (2), frame by frame.
 * auto = 13 when the scene allows the wide walk and its compressed packets could be built -- else 10 (an experiment build: 10,
 * 11 or 12 by the tree's statistics), else 9, else 7, else 4; MI3PT_OPT_WIDE / MI3PT_OPT_CULL = 0 make auto stop at 9 / 7.
 * Variants 1-8 execute exactly the reference's tests (counters equal the oracle's); all variants produce the same bits.
 * mi3pt_debug_active_variant says what a submit would run now, mi3pt_debug_last_launch what the last one ran. */
int mi3pt_set_kernel_variant(mi3pt_ctx *ctx, int variant);
/* Scheduling options: how the same work is cut into launches, steps and jobs.  NONE of them changes a bit of any image
 * or a path counter (tests/test_gpu_parity.py holds each to the defaults' output); they exist for the sweeps under
 * profiles/ and for the tests.  The library reads NO environment variable for them: a build with -DMI3PT_EXPERIMENTS
 * (make -C webgpu-pathtracer_amd/csrc experiments -> libmi3pt_exp.so) maps MI3PT_<NAME> variables onto this call at
 * mi3pt_create and adds two switches that DO change what is computed (plain-division slab tests; a scaled culling margin,
 * which voids its proof) -- those exist in no release object. */
typedef enum mi3pt_option {
    MI3PT_OPT_WALK_MIN = 0,    /* walk while at least this many lanes are walking (32) */
    MI3PT_OPT_LEAF_MIN = 1,    /* run a triangle step once this many lanes have a leaf parked (24); also the vote of mi3pt_render_aovs' culled walk */
    MI3PT_OPT_SHADE_SPLIT = 2, /* service step: serve the larger of the hit / miss groups, the other only with >= n lanes (64) */
    MI3PT_OPT_TAIL_POLICY = 3, /* drain-phase scheduling bits (7) */
    MI3PT_OPT_TOP_PACKETS = 4, /* kernel variants 6 / 8: node packets staged in LDS per wave */
    MI3PT_OPT_TRI_PAIR = 5,    /* a triangle step tests two parked triangles of a lane that has two (1) */
    MI3PT_OPT_JOB_REVERSE = 6, /* the launch's jobs bottom band first (1) */
    MI3PT_OPT_JOB_GROUP = 7,   /* tiles per job group; 0 frame-major, -1 the library's choice (-1) */
    MI3PT_OPT_JOB_CHUNK = 8,   /* job tickets per draw while the queue is long (4) */
    MI3PT_OPT_BATCH_LIMIT = 9, /* upper bound of frames per launch, of this context -- or of every member of this group (512) */
    MI3PT_OPT_BATCH = 10,      /* frames per launch on one GPU; x nranks for a rank of a tile split (256; the product is capped by MI3PT_OPT_BATCH_LIMIT); 1 = no batching */
    MI3PT_OPT_WAVES_PER_CU = 11, /* resident one-wave workgroups per compute unit (0 = what the kernel build is compiled for: 24 / 20 for the shipped walk's six- / five-wave builds, 16 otherwise) */
    MI3PT_OPT_CULL = 12,       /* 0: `auto` stops at variant 7 */
    MI3PT_OPT_WIDE = 13,       /* 0: `auto` stops at variant 9 */
    MI3PT_OPT_GATE = 14,       /* launches wait for their predecessor's drain mark (1; 0 when a profiler is attached) */
    MI3PT_OPT_GATE_TIMEOUT_MS = 22, /* the wait above has no bound of its own: a blocking entry point (mi3pt_sync, reads, pass times) that has
                                   * waited this long with a launch still held publishes the mark from the host (2000; 0 = never).  An early
                                   * release only lets two launches overlap more -- same bits.  The gate switches itself off, with a
                                   * "warning: ..." text in mi3pt_last_error() and MI3PT_OK returned, once a predecessor is seen to have
                                   * finished without publishing or after the third release */
    MI3PT_OPT_GATE_RELEASES = 23,   /* READ-ONLY: host-side releases so far */
    MI3PT_OPT_CAMERA_BASE = 25,     /* batched launches load the pixel-only part of a camera ray (uv, cameraToRay's direction, cam_pos + dir0 x
                                   * focalDistance) from an image formed once per camera, size and tile instead of forming it in every frame of
                                   * every pixel (1); costs 2 x 16 bytes per pixel of this context's share; 0 = formed in the kernel */
    MI3PT_OPT_PACKET_ORDER = 26,    /* numbering of the 4-ary packets in device memory: 0 breadth-first (the reference's flattenBVH order carried
                                   * over), 1 depth-first, 2 treelets of three levels; the walk follows references, any numbering renders the
                                   * same bits.  Applied at the next scene analysis (0) */
    MI3PT_OPT_SIX_WAVES = 27,       /* the shipped walk's build: 1 = six waves per SIMD (80 registers, a 19-entry LDS stack -- 25 for very large trees,
                                   * whose parked path state then lives in memory), 0 = five (96 registers, 24 entries), -1 = by the size of
                                   * the launch: six from 1.5 M jobs (tiles x frames) on -- long launches gain 2 .. 5 % from the extra wave, a
                                   * rank of an 8-way split's 10 ms launches lose 2 .. 3 % to the longer drain (-1) */
    MI3PT_OPT_LAST_BUILD = 29,      /* READ-ONLY: which instantiation of the state-machine kernel the most recent raytrace launch ran, beside
                                   * mi3pt_debug_last_launch: waves per SIMD it is compiled for (bits 0-7), the one-axis culling condition (bit 8),
                                   * the walk threshold (bits 16-23) -- the template arguments rocprofv3 prints */
    MI3PT_OPT_WALK_ADAPT = 30,      /* the walk threshold by the VIEW (round 6): a launch of the shipped walk reports what it cost -- box tests per ray --
                                   * through host-visible memory, and later launches run the deep-walk build (made for very large trees: walk_min 44,
                                   * a longer leaf list) while that is above 40, the ordinary one again below 30: the 870 k-triangle scene from close
                                   * up +4.4 %, its stated view (17 boxes per ray) unchanged.  No wait, no effect on any bit; MI3PT_OPT_WALK_MIN != 0
                                   * overrides it (1) */
    MI3PT_OPT_COLLAPSE = 28,        /* how the reference tree's nodes are grouped into the walks' wide packets: 1 = the SAH-optimal collapse (round 6:
                                   * fewest expected packet visits; 5.9 instead of 4.0 children per 8-ary packet), 0 = rounds 2 - 5's greedy one (open
                                   * the child with the largest area until the packet is full: packets of two at the bottom of the tree), -1 = greedy
                                   * for the 4-ary packets, optimal for the 8-ary ones: measured, the fuller packets change the boxes a ray tests by
                                   * < 1 % -- the half-empty packets are the ones rays seldom reach (profiles/r06_g_collapse.log).  Same bits (-1) */
    MI3PT_OPT_DEBUG_SUPPRESS_DRAIN = 24, /* tests: arm the gate but let no kernel publish its mark (forces the situation the time-out exists for) */
    MI3PT_OPT_SLOT_SETS = 15,  /* sets of per-frame radiance slots, 2 or 3; before mi3pt_resize (2) */
    MI3PT_OPT_PIPELINE = 16,   /* = mi3pt_set_pipelining */
    MI3PT_OPT_PRESENT_DEPTH = 18, /* MI3PT_PRESENT_EXACT: presenting frames that share one raytrace launch, >= 1 (16); each still
                                   * gets its own accumulate and fullscreen pass, in order -- 1 = also its own launch */
    MI3PT_OPT_HOST_ANALYSES = 19, /* READ-ONLY: host-side scene compiles this context has done (uploads that build packets, relabellings, cull
                                   * analyses); for a device group the sum over its members -- one per scene change whatever the group's
                                   * size: the scene is compiled by member 0 and copied device to device (tests/test_gpu_group.py) */
    MI3PT_OPT_DIAG_LITE = 21,     /* experiment build: with mi3pt_debug_wave_times enabled, run the LEAN kernel with lane counts per kind of step
                                   * (five waves per SIMD, like the shipped one) instead of the four-wave diagnostic twin (profiles/wave_timeline.py) */
    MI3PT_OPT_GATHER_STAGED = 20, /* device group: 1 = every member's rows reach the presenting context through pinned host memory -- the
                                   * path the gather takes where peer access is unavailable or a direct copy failed (forced: tests) */
    MI3PT_OPT_SKY_TILES = 31,       /* 8x8 tiles whose camera rays provably reach no geometry (mi3pt_host_sky_tiles) are shaded by a streaming kernel
                                   * at full wave width instead of being given to the persistent kernel as jobs; batched launches of the lean
                                   * culling walks, pinhole camera, one sample per frame.  Same bits, same rays / hits / misses / pixels; 0 = every
                                   * tile is traced; 1 = the streaming kernel is enqueued in front of the persistent one, 2 = behind it (1) */
    MI3PT_OPT_COST_ORDER = 17  /* a launch's jobs in the order of the tiles' measured cost, costliest first: one launch adds up the path
                                * segments per 8x8 tile, later launches with the same uniforms run the
                                * cheapest quarter of the tiles last (1), or every tile costliest first (2).  Default 0: measured +0.3 % on
                                * one GPU and -1.6 ... -4 % for a rank of a tile split in batched launches; 2 is for hosts that launch
                                * and wait frame by frame: 1.29 -> 1.205 ms per 1080p frame of the 870 k-triangle scene, the demo
                                * scene +-0 (profiles/r04_r_interactive_cost_order.log) */
} mi3pt_option;
int mi3pt_debug_set_option(mi3pt_ctx *ctx, int option /* mi3pt_option */, int value);
int mi3pt_debug_get_option(mi3pt_ctx *ctx, int option /* mi3pt_option */, int *value);
/* The variant a raytrace submit would run right now: the selected one, or its fall-back when the
 * uploaded scene does not admit it (tests use it to make sure nothing fell back silently). */
int mi3pt_debug_active_variant(mi3pt_ctx *ctx, int *variant);
/* The kernel the most recent raytrace launch actually ran: kind 0 = per-pixel kernel (one 8x8 tile per wave, the WGSL control
 * flow: variants 1 / 2, and the fall-back for launches beyond the state-machine kernel's packing limits), 1 = the persistent
 * state-machine kernel; its variant after the scene / launch fall-backs; lean = 1: the build without diagnostics that every
 * ordinary launch runs (96 vector registers, five waves per SIMD) -- whatever samplesPerFrame, maxBounces, storage format,
 * pipelining and presentation mode are (tests/test_gpu_parity.py::test_every_reference_setting_runs_the_lean_kernel); 0: the
 * diagnostic twin (a diagnostic buffer is bound or a step-voting option was changed through mi3pt_debug_set_option);
 * workgroups = the launch's grid.  Any pointer may be NULL. */
int mi3pt_debug_last_launch(mi3pt_ctx *ctx, int *kind, int *variant, int *lean, int *workgroups);
/* The reference's environment importance sampling (raytrace.wgsl:315-367: getEnvironmentMapUV /
 * ...MarginalCDF / ...ConditionalCDF / ...PDF over the CDF texture of renderer.ts:159-266) is dead
 * code as shipped -- its call sites raytrace.wgsl:398 and :402-404 are commented out.  enabled = 1
 * runs the frame as if those three lines were live (a miss takes its uv from the CDF and divides
 * the path's light by the pdf); it needs the CDF texture and uses the per-pixel kernel (no
 * batching).  Default 0 = the shipped behaviour. */
int mi3pt_set_env_sampling(mi3pt_ctx *ctx, int enabled);
/* Frame pipelining (default on): RAYTRACE|ACCUMULATE submits are queued; up to 256 consecutive
 * frames (mi3pt_batch_capacity) whose uniforms differ only in `frame` run as one raytrace launch plus one ordered
 * multi-frame running mean, and launches alternate between two internal streams so the next
 * one fills the CUs while the last paths of this one drain.  Any call that observes or
 * changes device state flushes the queue first; results are bit-identical.  Off: one fused
 * kernel per frame on the context's stream, launched inside mi3pt_submit. */
int mi3pt_set_pipelining(mi3pt_ctx *ctx, int enabled);

/* ---- component probes on the device (parity tests of the pieces) ----
 * rays: n x 6 floats (origin, direction); out: n x 12 floats
 * (hit, t, position xyz, normal xyz, materialIndex, box tests, triangle tests,
 * stack overflows) = raySceneIntersect, raytrace.wgsl:205-211. */
int mi3pt_debug_intersect(mi3pt_ctx *ctx, const float *rays, size_t n, float *out);
/* The same 12 floats per ray from the SHIPPED first-hit walk (what mi3pt_render_aovs runs where `auto` means kernel variant 13: compressed
 * wide packets, distance culling, wave-voted node / leaf steps).  Slots 0-8 as above; 9: node steps of the ray's lane, 10: leaves whose own
 * box passed the reference's test (each is a triangle test of the reference's walk), 11: 0.  Runs exactly when mi3pt_render_aovs would
 * run that walk; otherwise MI3PT_ERR_STATE (never another walk in its place). */
int mi3pt_debug_intersect_shipped(mi3pt_ctx *ctx, const float *rays, size_t n, float *out);
/* The walks' primitive decisions on n independent pairs, by the kernels' own device functions.  rays: n x 6; out: n x 12; a slot that is
 * not reported holds -1.
 *   fn 0 (box), geom n x 7 = min xyz, max xyz, box_unsafe (0 / 1, the flag the upload sets per box):
 *        0 ray_aabb, 1 ray_prepare().flags, 2 ray_aabb_pre, 3 leaf_box_hit; only when flags == 0 and box_unsafe == 0:
 *        4 slab_margin > 0, 5 slab_hit, 6 cwide_hit (5 and 6 on slab_q0's own max3(tnear), tfar), 7 ray_aabb_fast, 8-10 tnear xyz, 11 tfar
 *   fn 1 (triangle), geom n x 9 = a, b, c:  hit, t, u, v of ray_triangle (0-3), ray_triangle_e (4-7), ray_triangle_flat_e (8-11); the
 *        edges of the last two are formed on the device as the upload forms them, fl(b - a), fl(c - a); t, u, v are meaningful where hit. */
int mi3pt_debug_pairs(mi3pt_ctx *ctx, int fn, const float *rays, const float *geom, float *out, size_t n);
/* An ALTERNATIVE tree, built on the device from the uploaded triangles: a linear
 * BVH (Morton codes, radix sort, Karras' parallel hierarchy, bottom-up fit) in the same 48-byte
 * records, pre-order numbered so that a child follows its parent; nodes_out (host) receives
 * (2*ntris - 1) x 48 B for mi3pt_upload_bvh.  It is NOT the reference's SAH tree
 * (mi3pt_host_build_bvh_f64 is): box / triangle test counts differ, the image does not, except
 * where two triangles are hit at exactly the same t.  build_ms (optional): device time. */
int mi3pt_device_build_bvh(mi3pt_ctx *ctx, void *nodes_out, size_t nodes_capacity_bytes, size_t *nnodes_out, float *build_ms);
/* The device builders by name.  method 0 is the linear BVH above: the records of mi3pt_device_build_bvh word for word.  method 1 is a
 * tree of the SAH class built bottom-up by parallel locally-ordered clustering (Meister and Bittner 2018; csrc/pt_ploc.hip), under THE
 * LAW below, which tests/ploc_reference.py restates in numpy; the output is a function of the triangle records and the two parameters alone.
 *
 * Arithmetic.  fp32, round to nearest even, nothing contracted.  fminf / fmaxf as in csrc/pt_lbvh.hip: a NaN operand is dropped, -0
 *   orders below +0.
 * Leaves and order.  Exactly the linear builder's first half: per triangle, the NaN-ignoring box and centroid; the 63-bit keys; a stable
 *   sort.  The result is order[p], the triangle at sorted position p, for p = 0 .. n - 1.
 * Clusters.  A list of C entries, each a box plus a subtree.  At the start C = n, and cluster p is the leaf of triangle order[p] with
 *   that triangle's box.
 * Distance of two clusters.  U = the union of the boxes, per component fminf of the minima and fmaxf of the maxima.  e = U.max - U.min.
 *   a = (e.x * e.y + e.y * e.z) + e.z * e.x.  d = a if a == a, else +inf.  d is symmetric bit for bit.
 * Key of a pair of positions a < b.  K(a, b) = (d, b - a, a & 1, a), compared lexicographically, with d compared as fp32 values.
 *   Distinct pairs have distinct keys.  The two middle terms decide exact ties: b - a prefers the closer position; among the closest,
 *   a & 1 prefers an even lower position.  A run of identical boxes therefore pairs as (0,1), (2,3), ... and halves per iteration,
 *   instead of merging one pair per iteration into a chain.
 * A search iteration.  It runs while C > 1 and fewer than max_search_iterations of them have run.  For every position i, nn(i) is the
 *   position j != i that satisfies both of: |i - j| <= radius and 0 <= j < C; it has the least K(min(i, j), max(i, j)).
 * A forced iteration.  It runs while C > 1 after the search budget is used up.  nn(i) = i ^ 1 where that is < C, otherwise none.  This
 *   bounds the number of iterations for adversarial inputs, where a search iteration may merge a single pair.
 * Merge, in both kinds of iteration.  Every pair a < b with nn(a) = b and nn(b) = a merges.  The cluster at a becomes an internal node
 *   with left = a's subtree, right = b's subtree, box = U.  The cluster at b is removed.  All others stay.  The order of the survivors
 *   is preserved.
 * Progress.  The pair with the least key among all candidate pairs is mutual, so every search iteration merges at least one pair.
 * Records.  The 48-byte records of the linear builder, numbered in pre-order.  The root is index 0.  An internal node at index x whose
 *   left subtree holds m leaves has left = x + 1 and right = x + 2m.  Floats 0-2 are the min, 4-6 the max.  Word 7 is isLeaf, 8 is
 *   left, 9 is right, 10 is triangleIndex.  A leaf has left = right = -1 and triangleIndex = its triangle.  An internal node has
 *   triangleIndex = -1.  Words 3 and 11 are 0.  There are 2n - 1 records.  n = 1 is a single leaf.
 *
 * The contract is mi3pt_device_build_bvh's: BLOCKING; nodes_out (host) receives (2*ntris - 1) x 48 B, ready for mi3pt_upload_bvh.  Like
 * mi3pt_device_refit_bvh the call moves no state of the context: queued frames are launched first; no counter, epoch or
 * mi3pt_debug_last_launch field moves; rendering after the call without uploading the result is bit-identical to rendering before it;
 * temporaries are allocated and freed inside the call, on every path; a context that never calls it allocates and launches what it did
 * before.  A device group runs it on member 0.  info (optional): build_ms is the device time from the first kernel to the last, the
 * host's turn-arounds between the iterations included (the cluster count comes back once per iteration, 4 bytes through pinned memory;
 * no thread waits for another); the two counts are the iterations of each kind that ran (method 0: both 0).
 *   MI3PT_ERR_INVALID for a null ctx, params, nodes_out or nnodes_out, an unknown method, non-zero flags, under method 1 a radius outside
 *   1 .. 64 or max_search_iterations outside 0 .. 65535 (method 0 ignores both), a capacity below (2*ntris - 1) x 48.
 *   MI3PT_ERR_STATE before triangles are uploaded. */
#define MI3PT_BVH_METHOD_LBVH 0
#define MI3PT_BVH_METHOD_PLOC 1
#define MI3PT_PLOC_SEARCH_BLOCK 256     /* positions per workgroup of the neighbour search: the sizes its tests cross */
typedef struct mi3pt_bvh_build_params {
    int method;                 /* MI3PT_BVH_METHOD_* */
    int radius;                 /* method 1: 1 .. 64 */
    int max_search_iterations;  /* method 1: 0 .. 65535 */
    unsigned flags;             /* 0 */
} mi3pt_bvh_build_params;
typedef struct mi3pt_bvh_build_info {
    float build_ms;
    uint32_t search_iterations, forced_iterations;
} mi3pt_bvh_build_info;
int mi3pt_device_build_bvh_ex(mi3pt_ctx *ctx, const mi3pt_bvh_build_params *params, void *nodes_out, size_t nodes_capacity_bytes,
                              size_t *nnodes_out, mi3pt_bvh_build_info *info);
/* REFIT: the boxes of the tree last uploaded with mi3pt_upload_bvh, re-fitted on the device to the triangle records as they stand now --
 * after a later mi3pt_upload_triangles: rigid motion, skinning, anything that keeps the triangle count and index i naming the same surface
 * element (the contract of mi3pt_reproject_scene).  The topology stays: nodes_out (host) receives nnodes x 48 B, ready for
 * mi3pt_upload_bvh; *nnodes_out = nnodes, the record count of the uploaded tree; refit_ms (optional): device time.
 * Not an approximation of the boxes: the reference's are exact (a leaf box is Box3.setFromPoints(a, b, c), an internal box the union of
 * its inputs, raytrace.ts:546-550, 581-584) and rounding to fp32 is monotone, so this gives the boxes the reference's build would give the
 * old topology, bit for bit -- on unchanged triangles the uploaded bytes of a tree from mi3pt_host_build_bvh_f64 or mi3pt_device_build_bvh.
 * What is lost is tree quality: it is no longer the SAH tree of the new positions (mi3pt_host_bvh_cost before and after says by how much).
 * Pinned arithmetic, per 48-byte record (raytrace.wgsl:51-64: floats 0 - 2 min, 4 - 6 max, word 7 isLeaf, 8 left, 9 right, 10 triangleIndex):
 *   lo(x, y) = (y < x || (y == x && signbit(y))) ? y : x        hi(x, y) = (y > x || (y == x && !signbit(y))) ? y : x
 *   -- Math.min / Math.max on zeros; a NaN y is dropped, a NaN x is kept.  Per component:
 *   leaf (word 7 == 1), a, b, c = the three positions of triangle record `triangleIndex`:  min = lo(lo(a, b), c), max = hi(hi(a, b), c)
 *   internal:  min = lo(min(left), min(right)), max = hi(max(left), max(right)) -- always left then right, whichever child finished first
 *   words 3 and 7 .. 11 are copied bit for bit from the uploaded record.
 * What "the uploaded bytes come back" covers: ANY finite or infinite coordinates, zeros of either sign and subnormals included -- there lo / hi
 * are Math.min / Math.max, mi3pt_host_build_bvh[_f64] forms its boxes with the same two functions and mi3pt_device_build_bvh with fminf /
 * fmaxf, which order -0 below +0 on the device, so all three write the same words for the same vertices (-0 wins a minimum, +0 a maximum,
 * whatever the order of the operands; a subnormal is compared as what it is, never as a zero).  It does NOT cover a NaN coordinate: there
 * the three follow different rules, each documented where it lives -- this call the law above (it only selects: a NaN bound arrives with
 * its sign, payload and signalling bit as it stood in the triangle record; one on the left of a union is kept, one on the right dropped),
 * the host builder std::min / std::max's treatment of a NaN inside the reference's sort and sweep (csrc/pt_host_scene.cpp), the device
 * builder fminf / fmaxf, which drop a NaN on either side (csrc/pt_lbvh.hip) -- and the reference itself a fourth, Math.min / Math.max,
 * which return the NaN.  Non-finite vertices neither hang nor fault.
 * It changes NO state of the context: nothing the context renders with is touched, no counter, epoch or mi3pt_debug_last_launch field
 * moves, and rendering after the call without uploading the result is bit-identical to rendering before it.  Queued frames are launched
 * first, as for a read-back; the call BLOCKS until the records are on the host.  A device group runs it on member 0, where the scene lives.
 * On the context's stream: a device copy of the records, a parent table from the left / right words (one thread per node), zeroed arrival
 * counters, the fit (every leaf writes its box and climbs; at a parent the first child to arrive leaves, the second forms the union and
 * climbs on; no thread waits for another), a copy to the host.  Temporaries: nnodes x (48 + 4 + 4) bytes, allocated per call and freed before
 * it returns; a context that never calls this allocates and launches exactly what it did before.
 *   MI3PT_ERR_STATE before both uploads; unless the uploaded tree is proper (word 4 of mi3pt_host_scene_compile: every node reached once,
 *   one leaf per triangle, depth under 64) and the root, node 0, reaches EVERY record of the buffer (a record out of its reach has no place
 *   in a bottom-up pass; the message says which of the two it was); unless it names only triangles that exist (max_tri_ref < ntris).
 *   MI3PT_ERR_INVALID for a null context, a null nodes_out or nnodes_out, a capacity below nnodes x 48. */
int mi3pt_device_refit_bvh(mi3pt_ctx *ctx, void *nodes_out, size_t nodes_capacity_bytes, size_t *nnodes_out, float *refit_ms);

/* Debug: node-packet / triangle numbering used on the device.  0 (default, shipped) = packets
 * breadth-first like the uploaded nodes, triangles as uploaded.  1 = packets in the reference's
 * visiting order (node, right subtree, left subtree) and triangles in leaf-visiting order -- a
 * pure relabelling, bit-identical by construction, kept as a test of exactly that.  Call before
 * the uploads it should apply to; after switching back, the next upload of the BVH or of the
 * triangles restores the shipped numbering. */
int mi3pt_debug_set_packet_layout(mi3pt_ctx *ctx, int layout);

/* fn: 0 sin, 1 cos, 2 tan, 3 log, 4 exp, 5 atan2(a,b), 6 asin, 7 pow(a,b),
 * 8 fp16 round trip, 9 sqrt, 10 a/b; the kernels' reduced-instruction forms: 11 sqrt, 12 1/a,
 * 13..15 x/y/z of normalize(a, b, a - b), 16 log for a = 0 or a in [2^-32, 1] (rand()'s values: what randNormal
 * calls).  b may be NULL for unary functions. */
int mi3pt_debug_math(mi3pt_ctx *ctx, int fn, const float *a, const float *b, float *out, size_t n);

/* Diagnostic record of the last persistent raytrace launch: 16 x uint64 per resident wave
 * (begin, work-queue-empty, end on the 100 MHz wall clock; shader cycles begin->end; then
 * packed step statistics: walk steps | walking lanes, service steps | leaf lanes,
 * shaded lanes | hit lanes, path starts | segment starts; [8] triangle steps of the
 * deferred-leaf walk; [9..11] shader cycles spent in node / triangle / service steps; [12..15] reserved).
 * out == NULL: enable != 0 allocates the buffer, enable == 0 frees it. */
int mi3pt_debug_wave_times(mi3pt_ctx *ctx, int enable, uint64_t *out, size_t capacity_slots, size_t *slots_out);

/* ---- host-side scene compile (CPU, no device needed) ----
 * mi3pt_host_build_bvh: buildBVH + buildBVHRecursive + flattenBVH,
 * raytrace.ts:540-694, producing the identical tree (same axis rule, stable sort,
 * first strict SAH minimum, breadth-first flatten).  `triangles` is ntris x 112 B;
 * `nodes_out` receives (2*ntris - 1) x 48 B.  Returns the node count through
 * *nnodes_out.  nthreads <= 0 picks the hardware concurrency. */
int mi3pt_host_build_bvh(const void *triangles, size_t ntris, void *nodes_out,
                         size_t nodes_capacity_bytes, size_t *nnodes_out, int nthreads);
/* Same builder on the JavaScript host's double-precision world-space positions
 * (9 doubles per triangle: a.xyz b.xyz c.xyz), i.e. before the structured view
 * rounds them to fp32 -- this is what raytrace.ts:546-550 feeds Box3.setFromPoints,
 * so near-tie splits come out exactly as in the reference. */
int mi3pt_host_build_bvh_f64(const double *positions, size_t ntris, void *nodes_out,
                             size_t nodes_capacity_bytes, size_t *nnodes_out, int nthreads);
/* The SAH figure of a tree (48-byte records) as it stands, what a host compares before and after mi3pt_device_refit_bvh: with
 * (x, y, z) = max - min of a record's box, each difference taken in double from the fp32 fields, area = 2 * ((x*y + x*z) + y*z);
 * *cost = (the areas of ALL nnodes records, added in index order) / (the area of node 0, the root); 0 for a root area of 0.  Leaves count
 * like internal nodes: one figure for "boxes a ray has to be tested against", relative to the root.  MI3PT_ERR_INVALID for a null
 * pointer or nnodes == 0. */
int mi3pt_host_bvh_cost(const void *nodes, size_t nnodes, double *cost);
/* updateEnvironmentTexture's CDF texture, renderer.ts:159-266: R marginal CDF,
 * G conditional CDF, B sin-weighted luminance, A 1. */
int mi3pt_host_env_cdf(const float *rgba, int width, int height, float *cdf_rgba_out);
/* Host-only self-check of the eight-wide packets of kernel variant 14 (no device; what the CPU tests call): builds them for a tree
 * (48-byte records) + triangles (112-byte records) as the scene analysis does (greedy = 0: the SAH-optimal grouping, what a context uses by
 * default for these packets; 1: the greedy one, MI3PT_OPT_COLLAPSE = 0), then walks the result independently of the builder --
 * every leaf triangle reachable exactly once, every packet referenced once, records carrying their leaf's box and triangle, every
 * decoded child box containing everything below it.  out[0..5] = packets, records, packet levels, children per packet x 1000,
 * leaves reached, 1 if a context would offer variant 14 for this tree (levels within the walk's stack).  MI3PT_ERR_STATE with the
 * reason in mi3pt_last_error when the tree does not admit the packets or a check fails. */
int mi3pt_host_eight_wide_check(const void *nodes, size_t nodes_bytes, const void *triangles, size_t triangles_bytes, int greedy, uint64_t out[6]);
/* Host-only scene compile (no device, no context): everything mi3pt_upload_bvh, mi3pt_upload_triangles and a context's lazy scene analysis
 * compute for a tree (48-byte records) + triangles (112-byte records), by the same code, with every device buffer reduced to a 64-bit
 * FNV-1a digest of its bytes.  collapse / packet_order: as MI3PT_OPT_COLLAPSE / MI3PT_OPT_PACKET_ORDER; want_eight_wide: also the packets
 * of kernel variant 14.  out[0 .. MI3PT_SCENE_COMPILE_WORDS - 1]: 0 nodes, 1 triangles, 2 node packets, 3 leaf_cap, 4 tree_proper,
 * 5 walk_stack_worst, 6 cull_stack_ok, 7 root_ref, 8 scene_flags, 9 max_tri_ref, 10 max_mat_ref, 11 analysed (1: the tree admits the
 * culling walks and every leaf names an uploaded triangle -- 12 .. 23 and 27 .. 31 are 0 otherwise), 12 / 13 the bits of cull_ka /
 * cull_kb, 14 wide_ok, 15 cwide_ok, 16 cw8_ok, 17 wide_root_nested, 18 wide_stack_worst, 19 auto_wide_variant, 20 wide packets, 21 8-wide
 * packets, 22 8-wide records, 23 8-wide levels; digests (0: not built): 24 node packets with their final cull words, 25 leaf ranks, 26 48-byte
 * triangle packets, 27 wide packets, 28 compressed packets, 29 64-byte records, 30 8-wide packets, 31 8-wide records.  MI3PT_ERR_INVALID with
 * the upload's own message for a tree or triangles an upload would refuse. */
#define MI3PT_SCENE_COMPILE_WORDS 32
int mi3pt_host_scene_compile(const void *nodes, size_t nodes_bytes, const void *triangles, size_t triangles_bytes, int collapse, int packet_order,
                             int want_eight_wide, uint64_t *out, size_t out_capacity);
/* Host-only: the BYTES of one buffer of that compile's walk stage, for the same arguments and by the same code -- they hash (64-bit FNV-1a)
 * to the digest mi3pt_host_scene_compile reports for it.  kind: 0 the cull words (one uint32 per node packet), 1 wide packets (128 bytes
 * each, digest word 27), 2 compressed 4-ary packets (64 bytes, word 28), 3 64-byte triangle records (word 29), 4 8-wide packets (80 bytes,
 * word 30), 5 8-wide records (64 bytes, word 31); 4 and 5 build the packets of kernel variant 14 (want_eight_wide = 1).  *bytes_out = the
 * buffer's size, 0 when the compile does not build it for this tree; `out` may be NULL to ask for the size only, otherwise `capacity` bytes
 * must hold it.  The layouts are the kernels' own (csrc/pt_kernels.h) and no part of the ABI: for tests that decode what a context uploads. */
int mi3pt_host_walk_buffer(const void *nodes, size_t nodes_bytes, const void *triangles, size_t triangles_bytes, int collapse, int packet_order,
                           int kind, void *out, size_t capacity, size_t *bytes_out);
/* The EMPTY TILES of a view (no device): the 8x8 tiles of rank `rank`'s share of a width x height image (tiles_x = ceil(width / 8), rows of
 * tiles over the rank's LOCAL rows, row-major) in which no pixel's camera ray, for any frame's jitter, can pass the reference's slab
 * test on any box of a cut of the tree `nodes` (48-byte records) -- such a ray reaches no leaf, the path is one miss.  A context
 * shades these tiles with a streaming kernel instead of tracing them (MI3PT_OPT_SKY_TILES; PROOFS.md section 5).  `raytrace_uniforms`: the
 * 96-byte block.  empty_out[tile] = 1 / 0, `capacity` bytes; *ntiles_out = tiles (empty_out may be NULL to ask for the size only).
 * All zero unless aperture == 0, no camera coordinate is -0, samplesPerFrame == 1, maxBounces >= 1, the camera lies in front of
 * every cut box and every box of the tree contains its children's. */
int mi3pt_host_sky_tiles(const void *nodes, size_t nodes_bytes, const void *raytrace_uniforms, int width, int height,
                         int rank, int nranks, int block_rows, uint8_t *empty_out, size_t capacity, size_t *ntiles_out);
/* Host-only (no device, no context): WHICH KERNEL a raytrace launch runs and on how many workgroups, by the function a context's launches
 * go through, for `rows` launches described by MI3PT_HOST_ROUTE_INPUTS int64 each: 0 the requested variant (what
 * mi3pt_debug_active_variant names); 1 / 2 the rank's tile, width and local rows; 3 frames of the launch, 4 compute units, 5
 * MI3PT_OPT_WAVES_PER_CU, 6 tiles on the launch's active list (0: all), 7 MI3PT_OPT_SIX_WAVES; 8 walk_min, 9 leaf_min, 10 shade_split,
 * 11 tail_policy, 12 job_chunk, 13 tri_pair; 14 / 15 / 16 whether the wave-times buffer, the tile-cost buffer and the service block are bound,
 * 17 diag_lite; 18 maxBounces, 19 samplesPerFrame, 20 / 21 the bits of the resolution's two floats; 22 nodes, 23 scene flags, 24 root
 * reference, 25 leaf_cap; 26 / 27 whether the compressed 4-ary / the 8-wide packets and their records are built.  Per row
 * MI3PT_HOST_ROUTE_OUTPUTS int64: 0 kind, 1 variant, 2 lean, 3 workgroups (as mi3pt_debug_last_launch), 4 waves per SIMD, 5 one-axis
 * culling condition, 6 walk threshold (as MI3PT_OPT_LAST_BUILD); 7 .. 18 the state-machine kernel's twelve template arguments (kind 1;
 * 0 otherwise); 19 the library carries that instantiation; 20 the service-setup kernel runs in front.  For tests; no part of the ABI. */
#define MI3PT_HOST_ROUTE_INPUTS 28
#define MI3PT_HOST_ROUTE_OUTPUTS 21
int mi3pt_host_route(const int64_t *in, size_t rows, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* MI3PT_H */
