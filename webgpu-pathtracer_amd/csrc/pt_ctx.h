// pt_ctx.h -- the context behind the C ABI of include/mi3pt.h (pt_context.hip and pt_ctx_*.hip; what those call of each other:
// pt_ctx_calls.h): what it owns, by lifetime.  Host code only: no file that defines a kernel includes this.
#pragma once
#include "../../include/mi3pt.h"
#include "pt_internal.h"
#include "pt_kernels.h"

#include <hip/hip_runtime.h>
#include <array>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return pt_set_error(MI3PT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---- owners.  Each holds one resource of the HIP runtime, lets go of it when it is destroyed or assigned to, moves and does not copy,
// and reads as the plain pointer / handle wherever one is wanted.  Whoever destroys one has made the resource's device current
// (require_ctx, mi3pt_destroy).

// Device memory (Pinned: page-locked host memory) with its size in bytes.
template <class T, bool Pinned = false> struct DevBuf {
    T *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DevBuf() { reset(); }
    // (a request for no bytes -- an image of a rank without rows -- still owns a pointer: 16 bytes)
    hipError_t alloc(size_t nbytes, unsigned pinned_flags = hipHostMallocDefault)
    {
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void **)&p, nbytes ? nbytes : 16, pinned_flags) : hipMalloc((void **)&p, nbytes ? nbytes : 16);
        if (e != hipSuccess) p = nullptr;
        else bytes = nbytes;
        return e;
    }
    void adopt(T *q, size_t nbytes) { reset(); p = q; bytes = nbytes; }      // (memory of another allocator that hipFree releases)
    void reset() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
    T *release() { T *q = p; p = nullptr; bytes = 0; return q; }
    operator T *() const { return p; }
    template <class U> U *as() const { return static_cast<U *>(p); }
};
template <class T> using PinnedBuf = DevBuf<T, true>;

// An event or a stream.
template <class H, hipError_t (*Destroy)(H)> struct HipOwned {
    H h = nullptr;
    HipOwned() = default;
    HipOwned(HipOwned &&o) noexcept : h(o.h) { o.h = nullptr; }
    HipOwned &operator=(HipOwned &&o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
    ~HipOwned() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    H *put() { reset(); return &h; }          // for hipEventCreate* / hipStreamCreate*
    operator H() const { return h; }
};
using Event = HipOwned<hipEvent_t, hipEventDestroy>;
using Stream = HipOwned<hipStream_t, hipStreamDestroy>;

// GPU time of one pass: an event pair around it on the pass's stream, created by the first timed call (a context that never times a
// pass creates none).  The batched raytrace launches keep their own events (ev_rt: per parity, folded into running totals).
struct PassTimer {
    Event ev[2];
    bool recorded = false;
    hipError_t begin(hipStream_t s)
    {
        for (Event &e : ev)
            if (!e)
                if (hipError_t r = hipEventCreate(e.put())) return r;
        return hipEventRecord(ev[0], s);
    }
    hipError_t end(hipStream_t s)
    {
        const hipError_t r = hipEventRecord(ev[1], s);
        recorded = r == hipSuccess;
        return r;
    }
    int elapsed_us(mi3pt_ctx *ctx, float *us, const char *not_timed);      // (MI3PT_ERR_STATE with that text while nothing is recorded)
    void forget() { recorded = false; }
};

// ---- the scene: from upload to upload.  The device buffers every member of a device group holds a copy of (clone_scene) ...
struct SceneBuffers {
    using Buf = DevBuf<void>;
    Buf d_tris, d_nodes, d_mats;
    Buf d_packets, d_tripk;
    Buf d_leaf_rank;                // per triangle: position of its leaf in the reference's visiting order
    Buf d_tris_perm;                // 112-B records in the relabelled order (the uploaded order stays in d_tris)
    Buf d_wide;                     // wide (4-ary) packets for kernel variant 10, built with the cull analysis
    Buf d_cwide, d_tripk64;         // compressed wide packets + 64-byte triangle records (kernel variant 13)
    Buf d_cw8, d_tripk8;            // 8-wide compressed packets + their triangle records (kernel variant 14)
    // every buffer above, of a const or a mutable scene alike (a member that is not listed here fails the static_assert below)
    template <class S> static auto all(S &s) -> std::array<decltype(&s.d_tris), 12>
    {
        return { &s.d_tris, &s.d_tris_perm, &s.d_nodes, &s.d_mats, &s.d_packets, &s.d_tripk, &s.d_leaf_rank, &s.d_wide, &s.d_cwide, &s.d_tripk64, &s.d_cw8, &s.d_tripk8 };
    }
};
static_assert(sizeof(SceneBuffers) == 12 * sizeof(SceneBuffers::Buf), "SceneBuffers::all lists every buffer");

// ... and everything the uploads (pt::compile_tree, pt::compile_triangles), prepare_layout and prepare_cull (pt::compile_walk) derive from
// them: plain values, copied to a group's other members by one assignment.  A fact that is added here reaches every member.
struct SceneFacts {
    int leaf_cap = 0;                     // LDS slots left for deferred leaves (0 = scene must be walked in order)
    bool cull_stack_ok = false;           // proper tree, the 64-entry abort cannot fire, and the near-first walks'
                                          // order-independent worst-case stack fits (upload_bvh)
    size_t ntris = 0, nnodes = 0, nmats = 0, npackets = 0;
    uint32_t root_ref = 0;
    uint32_t scene_flags = 0;
    bool wide_root_nested = false;  // prepare_cull: the root's box contains its children's boxes (the wide walk may skip the root test)
    int64_t max_tri_ref = -1;       // largest triangleIndex referenced by a leaf
    int64_t max_mat_ref = -1;       // largest materialIndex referenced by a triangle
    size_t nodes_reached = 0;       // mi3pt_upload_bvh: records the root reaches (mi3pt_device_refit_bvh needs every one reached)
    bool tree_proper = false;       // mi3pt_upload_bvh: every node reached once, one leaf per triangle, the 64-entry abort cannot fire
    int walk_stack_worst = 64;      // mi3pt_upload_bvh: entries the reference walk's stack can hold at most on this tree (64: unknown, or the abort can fire)
    // distance-culling walk (kernel variant 9): per-child |e1||e2| bounds in the packets' `cull` field
    bool cull_dirty = true;         // triangles or tree changed since the last analysis
    bool cull_ok = false;           // analysis done and the tree admits the walk
    float cull_ka = 0.0f, cull_kb = 0.0f;   // scene constants of the distance bound
    int auto_wide_variant = 10;     // which of the wide walks (10 exact slab test, 11 filtered, 12 filtered + one-axis culling
                                    // condition) `auto` resolves to for this scene: prepare_cull's walk statistics
    bool wide_ok = false;
    bool cwide_ok = false;          // compressed wide packets + 64-byte triangle records built (kernel variant 13): needs wide_ok, every box nested and finite
    bool cw8_tried = false;         // the last scene analysis ran with variant 14 selected: the 8-wide packets were built, or found impossible for this tree
    bool cw8_ok = false;            // 8-wide compressed packets + their triangle records built (kernel variant 14): needs cwide_ok
    size_t ncw8 = 0, cw8_records = 0;
    int cw8_height = 0;
    size_t nwide = 0;
    int wide_leaf_cap = 0;
    uint32_t wide_root = 0;
    int wide_stack_worst = 64;      // prepare_cull: the wide walks' node stack, order-independent worst case (internal packets only; <= SM_CULL_STACK_MAX where wide_ok)
    // Debug: packet / triangle numbering (mi3pt_debug_set_packet_layout).  0 = breadth-first packets,
    // triangles as uploaded (shipped).  1 = packets in the reference's visiting order (node, right
    // subtree, left subtree) and triangles in leaf-visiting order: a pure relabelling.
    int layout = 0;
    bool layout_dirty = false;      // the relabelling still has to be applied to what was uploaded
    bool layout_active = false;     // the device holds relabelled packets / triangles
    // the boxes of a cut of the uploaded tree (mi3pt_upload_bvh), behind the empty tiles of a view (sky_prepare)
    std::vector<float> sky_cut;
    bool sky_cut_ok = false;
};

// ---- the images: from resize to resize.  Everything mi3pt_resize lets go of: a fresh value of this struct is a context without textures.
// What a resize keeps -- options, `moments` / `by_count`, the convergence threshold, aov_u / aov_epoch -- lives in the context itself.
struct ImageState {
    int width = 0, height = 0, local_rows = 0;
    DevBuf<float4> d_radiance, d_accum_own, d_canvas;
    float4 *d_accum = nullptr;           // d_accum_own, or the caller's memory (mi3pt_bind_accumulation)
    DevBuf<uint32_t> d_canvas8;
    DevBuf<uint64_t> d_block_counters;
    int nblocks = 0;
    // Batched frames write per-frame radiance slots, one set per launch parity.  Allocated on
    // demand (an interactive host that presents every frame only ever needs one slot per
    // parity; up to 8 frames: 8 slots; more: the full batch_cap once), see ensure_slots().
    // Two sets, one per launch parity.  (MI3PT_SLOT_SETS=3, experiment: launch k+2 then reuses launch k's stream and
    // counters but not its slots, so it need not wait for the ordered mean of batch k -- which only finds room on the
    // GPU when launch k+1 drains.  Measured twice: dragon-class -1.8 %, demo +1.3 %: not the critical path.)
    DevBuf<float4> d_slots[3];
    int slots_alloc[3] = { 0, 0, 0 };    // frames each set can hold
    float4 *last_radiance = nullptr;     // the radiance image the most recent raytrace pass wrote
    // RtLaunch::cam_base: the pixel-only part of the camera rays, one image per launch parity (a launch only ever reads the image
    // of its own stream, so a moving camera needs no wait: the refill is enqueued on that stream in front of the launch), valid for
    // the camera / size / tile in cam_base_key
    DevBuf<float4> d_cam_base[2];
    uint8_t cam_base_key[2][80] = {};
    bool cam_base_valid[2] = { false, false };
    // First-hit feature images (mi3pt_render_aovs): each local_rows x width x 16 B, allocated by the first call that asks for it and
    // freed with the textures; aov_valid: rendered (a group's presenting context: gathered) since the last resize.  The pass runs on
    // the context's stream BESIDE the sample path: it reads the scene, writes these images and touches nothing a sample launch reads
    // or writes, so the frame queue is neither flushed nor ordered against it.
    DevBuf<float4> d_aov[MI3PT_AOV_COUNT];
    bool aov_valid[MI3PT_AOV_COUNT] = {};
    PassTimer aov_timer;
    // The feature-guided de-noise (mi3pt_denoise_guided): two ping-pong images and the packed normal + hit records, each local_rows x width
    // x 16 B, allocated by the first call and freed with the textures; guided_result: the image the last level wrote (null: no filter since
    // the last resize).
    DevBuf<float4> d_guided[2], d_guided_nh;
    const float4 *guided_result = nullptr;
    PassTimer guided_timer;
    // MI3PT_GUIDED_VARIANCE: two ping-pong variance images, local_rows x width floats, allocated by the first call with the flag and freed
    // with the textures; guided_var_result: the one the last level wrote (null: the last filter ran without the flag)
    DevBuf<float> d_guided_var[2];
    const float *guided_var_result = nullptr;
    // mi3pt_set_guided_despike: the image the pre-pass writes and the filter reads in the accumulation image's place (local_rows x width x
    // 16 B) with the words that count the clamped texels (pt::DESPIKE_SLOTS of them, summed at the read), both allocated by the first filter
    // that runs with the state on and freed with the textures; guided_despiked: the last filter since the last resize ran with the state on
    // (the count is that filter's)
    bool guided_despiked = false;
    DevBuf<float4> d_guided_despike;
    DevBuf<uint32_t> d_guided_despike_count;
    // The moments image (mi3pt_set_moments): local_rows x width x (M2.rgb, n) fp32 beside the accumulation image, kept by the
    // moments-keeping accumulate kernels; allocated while `moments` is on and the context has textures.
    DevBuf<float4> d_moments;
    // The reprojection (mi3pt_reproject; pt_reproject.hip).  d_aov_prev: the old view's NORMAL / POSITION / IDS (indexed by mi3pt_aov;
    // swapped with d_aov), d_reproject: the scratch (mean, moments) the kernel writes -- all allocated by the first call and freed with
    // the textures.
    DevBuf<float4> d_aov_prev[MI3PT_AOV_COUNT];
    DevBuf<float4> d_reproject[2];
    PassTimer reproject_timer;
    // The held history (mi3pt_hold_history, mi3pt_merge_history; pt_history.hip).  d_hold: the held (mean, moments), allocated by the first
    // hold and freed with the textures (or with the moments image); history_held: they hold a history that nothing has dropped or merged.
    DevBuf<float4> d_hold[2];
    bool history_held = false;
    PassTimer history_timer;
    // The per-tile error estimate (mi3pt_estimate_convergence; pt_converge.hip): the tile map ceil(local_rows / 8) x ceil(width / 8) x 16 B,
    // the tile kernel's per-block records and the summary on the device, the summary's copy in pinned host memory, all allocated by the
    // first call and freed with the textures
    DevBuf<float4> d_conv_tiles;
    DevBuf<pt::ConvergePart> d_conv_parts;
    DevBuf<pt::ConvergeSummary> d_conv_summary;
    PinnedBuf<pt::ConvergeSummary> h_conv_summary;
    bool conv_valid = false;             // an estimate has been enqueued since the last resize
    PassTimer conv_timer;
};

// ---- one tile list of a launch on the device (sky_prepare, tile_lists_stage): [active tiles, ascending | empty tiles], one per launch
// parity and a third for the launches mi3pt_submit runs at once on the context's stream -- written and read on that stream only
struct TileList {
    DevBuf<uint32_t> d_list;
    size_t cap = 0;                      // entries d_list can hold
    uint8_t dev_key[104] = {};           // the view + mask the list on the device was composed for
    bool dev_valid = false;
    std::vector<uint32_t> staged;        // what the last copy into d_list reads (kept until `copied`)
    Event copied;
    bool copied_valid = false;
    // behind the last ordered mean that read d_list -- the copy of a new list waits for it (the mean runs on the context's stream, the
    // copy on the launch's).  Created by the first mask.
    Event read;
    bool read_valid = false;
};

struct GroupState;

struct mi3pt_ctx : SceneBuffers, SceneFacts, ImageState {
    int device = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;         // own_stream, or the caller's (mi3pt_set_stream)

    // scene: what is not part of SceneBuffers / SceneFacts -- the environment, the options that shape the analyses, the versions
    DevBuf<void> d_env, d_cdf;
    bool cull_enabled = true;       // MI3PT_CULL=0: variant 0 resolves to the reference-counter walk (7)
    bool wide_enabled = true;       // MI3PT_WIDE=0: variant 0 stops at 9
#ifdef MI3PT_EXPERIMENTS
    bool exp_force_slow_slab = false;
    double exp_cull_scale = 1.0;
#endif
    int num_cus = 256;              // hipDeviceProp_t::multiProcessorCount
    pt::RtRoute last_route;      // the kernel the most recent raytrace launch ran (mi3pt_debug_last_launch)
    // Cost order of a launch's jobs (launch_batch): one launch adds up the path segments traced per 8x8 tile (RtLaunch::tile_cost);
    // when it has finished the tiles are sorted, costliest first, into a permutation that later launches with the same raytrace
    // uniforms (frame aside) use as their job order (RtLaunch::tile_perm) -- their last tickets are then their cheapest tiles and
    // the drain after the queue has run empty is short.  Two permutation buffers: a new order never overwrites the one that
    // launches in flight may still read.  Any order renders the same bits.
    int cost_order = 0;                   // (1: the cheapest quarter last; 2: all tiles, costliest first) MI3PT_OPT_COST_ORDER: off -- measured ± 0 on one GPU and −1.6 … −4 % for a rank of a split (profiles/r03_h_cost_order.log)
    int cost_state = 0;                   // 0: nothing measured for the current uniforms, 1: the measuring launch is in flight, 2: a permutation is in use
    DevBuf<uint32_t> d_tile_cost, d_tile_perm[2];
    size_t cost_tiles = 0;                // entries of each of the three arrays
    int perm_cur = 0;
    Event cost_event, perm_used[2];
    bool perm_used_valid[2] = { false, false };
    Stream cost_stream;
    uint8_t cost_key[MI3PT_RAYTRACE_UNIFORMS_SIZE] = {};
    GroupState *group = nullptr;          // mi3pt_create_group: this handle fans every call out to member contexts (pt_ctx_group.hip)
    uint64_t scene_epoch = 1;             // bumped whenever the device's scene data or its analysis changes (uploads, prepare_layout, prepare_cull)
    uint64_t host_analyses = 0;           // scene compiles done on the host by THIS context: uploads that build packets + cull analyses (MI3PT_OPT_HOST_ANALYSES)

    // textures: the tile the images are cut for
    int rank = 0, nranks = 1, block_rows = 8;                 // active tile
    int next_rank = 0, next_nranks = 1, next_block_rows = 8;  // applied at resize
    bool partial() const { return nranks != 1; }     // this context holds part of the image
    int slot_sets = 2;                   // (ImageState::d_slots)
    int batch_cap = 1;                   // frames per launch at this size (batch limit, tile split, free memory)
    bool cam_base_enabled = true;        // MI3PT_OPT_CAMERA_BASE
    // The empty tiles of the view (pt_host_sky.cpp; PROOFS.md section 5): 8x8 tiles whose camera rays reach no geometry are not jobs of the
    // persistent kernel -- a streaming kernel shades them (launch_batch: sky_prepare).  The classification is cached under the camera-base
    // key + what else it depends on + the scene's version, on the host (one per view) and as a device list per launch parity (TileList).
#ifndef PT_SKY_TILES_DEFAULT
#define PT_SKY_TILES_DEFAULT 1           // (A/B builds: 0 / 2)
#endif
    int sky_tiles = PT_SKY_TILES_DEFAULT; // MI3PT_OPT_SKY_TILES: 0 off, 1 on (the streaming kernel in front of the persistent one), 2 on (behind it)
    uint8_t sky_key[104] = {}, sky_seen_key[104] = {};
    bool sky_host_valid = false;
    std::vector<uint8_t> sky_empty;      // the classification for sky_key: 1 per empty tile
    std::vector<uint32_t> sky_host;      // the list for sky_list_key: [sampled and not empty | sampled and empty] (pt_host_adapt.cpp)
    uint8_t sky_list_key[104] = {};      // the view's key (zero but for the tile where the list is of the mask alone) + the mask's epoch
    bool sky_list_valid = false;
    int sky_host_active = 0, sky_host_sky = 0;
    uint64_t sky_host_pixels = 0;        // in-bounds pixels of the listed empty tiles
    TileList lists[3];
    // The sample mask (mi3pt_set_sample_mask): one byte per 8 x 8 tile of the compact image, empty = no mask.  Every mask that is set
    // gets a new epoch, which is part of the lists' keys (0: no mask), so a list a launch in flight reads is never taken for the new
    // mask's.
    std::vector<uint8_t> mask;
    uint64_t mask_epoch = 0, mask_epochs = 0;
    uint32_t mask_sampled = 0;
    int collapse = -1;                   // MI3PT_OPT_COLLAPSE: 1 = the SAH-optimal grouping of the tree's nodes into wide packets, 0 = the greedy one of rounds 2 - 5, -1 = greedy for the 4-ary packets, optimal for the 8-ary ones (what each measured best with)
    int six_waves = -1;                  // MI3PT_OPT_SIX_WAVES: the compressed-wide walk's build, -1 = by the size of the launch (pt::RtLaunch::six_waves)
    int packet_order = 0;                // MI3PT_OPT_PACKET_ORDER: numbering of the wide packets in memory (prepare_cull): 0 breadth-first, 1 depth-first, 2 treelets
    bool output_is_accum = false;
    DevBuf<uint32_t> d_tile_counter;
#ifndef PT_JOB_REVERSE_DEFAULT
#define PT_JOB_REVERSE_DEFAULT 1         // (A/B builds: 0)
#endif
    int job_reverse = PT_JOB_REVERSE_DEFAULT; // MI3PT_JOB_REVERSE, see RtLaunch::job_reverse (the top band last: +0.5 % with the sky up there)
    int job_group = -1;                  // MI3PT_JOB_GROUP, see RtLaunch::job_group; -1 = chosen per tile set in build_launch
    int tri_pair = 1;                    // MI3PT_TRI_PAIR, see RtLaunch::tri_pair
    int job_chunk = PT_DEFAULT_JOB_CHUNK;    // job tickets per draw from the queue (MI3PT_JOB_CHUNK; 1 = one atomic per job)
    DevBuf<uint32_t> d_drain_flag;        // signal memory: sequence number of the last batched launch that started draining
    bool gate_enabled = false;            // launches wait on d_drain_flag (off when the memory or the wait is unavailable)
    uint32_t launch_seq = 0;              // sequence number of the last batched launch
    int gate_timeout_ms = 2000;           // MI3PT_OPT_GATE_TIMEOUT_MS: a blocking entry point that has waited this long releases a held launch from the host (ctx_wait)
    int gate_releases = 0;                // MI3PT_OPT_GATE_RELEASES: how often that happened
    int gate_stalls_in_a_row = 0;         // ... how many of them since anything last moved by itself (ctx_wait: three switch the gate off)
    bool debug_suppress_drain = false;    // MI3PT_OPT_DEBUG_SUPPRESS_DRAIN (tests): the gate is armed but no kernel publishes its drain mark
    Stream gate_release_stream;
    volatile uint32_t *h_drain_flag = nullptr;   // the drain word as the host sees it, where signal memory is host memory (hipPointerGetAttributes at create); else null
    // The walk threshold by the VIEW (round 6): after every launch of the shipped walk a one-block kernel leaves what the launch cost -- box
    // tests and rays -- in host-visible memory; the next launch the host builds runs the deep-walk build (walk_min 44, its own leaf constants:
    // made for very large trees) when the last launch seen tested more than WALK_ADAPT_ENTER boxes per ray, the ordinary one again below
    // WALK_ADAPT_LEAVE.  The 870 k-triangle scene: its stated view 17 boxes per ray (deep build -5.6 %), its close-up 68 (+4.4 %).  Same bits.
    int walk_adapt = 1;                   // MI3PT_OPT_WALK_ADAPT
    bool deep_by_view = false;
    PinnedBuf<uint64_t> h_walk_stats;     // pinned host memory, [2 parities][4]: seq, box tests, rays of that parity's last launch
    uint64_t *d_walk_stats = nullptr;     // ... as the device addresses it
    DevBuf<uint64_t> d_walk_prev;         // [2 parities][2] the counter sets' sums at the previous call (device)
    uint64_t walk_stats_seq = 0, walk_stats_seen = 0;
    DevBuf<float> d_park;                 // [2 parities][PT_MAX_RESIDENT_WAVES][6][64] parked path state of the builds that keep it in memory (RtLaunch::park)
    DevBuf<uint32_t> d_stack_overflow;    // [2 parities][PT_MAX_RESIDENT_WAVES][SM_OVERFLOW_ENTRIES][64] overflow stack entries
    DevBuf<void> d_fs_taps;               // the de-noise pass's tap table (pt::launch_fullscreen), built for fs_taps_res
    float fs_taps_res[2] = { 0.0f, 0.0f };
    bool fs_taps_valid = false;
    DevBuf<uint8_t> d_service;            // ring of SERVICE_SLOTS pt::RtService blocks: one per batched launch in flight (launch_batch)
    DevBuf<uint64_t> d_wave_times;        // diagnostic stamps, allocated by mi3pt_debug_wave_times(enable)
    int diag_lite = 0;                    // MI3PT_OPT_DIAG_LITE (experiment builds): with the stamps enabled, the lean build + lane counts runs instead of the diagnostic twin
    int wave_times_slots = 0;

    uint8_t u_rt[MI3PT_RAYTRACE_UNIFORMS_SIZE] = {};
    uint8_t u_acc[MI3PT_ACCUMULATE_UNIFORMS_SIZE] = {};
    uint8_t u_fs[MI3PT_FULLSCREEN_UNIFORMS_SIZE] = {};

    int storage = MI3PT_STORAGE_F32;
    int variant = 0;
    bool env_sampling = false;  // mi3pt_set_env_sampling: the reference's dormant importance-sampling lines
    int tail_policy = PT_DEFAULT_TAIL_POLICY;        // MI3PT_TAIL_POLICY: see RtLaunch::tail_policy
    int shade_split = PT_DEFAULT_SHADE_SPLIT;       // MI3PT_SHADE_SPLIT: see RtLaunch::shade_split (64: while lanes walk, only the larger group is served)
    int leaf_min = PT_DEFAULT_LEAF_MIN;          // deferred-leaf walk: lanes with a parked leaf that trigger a triangle step (MI3PT_LEAF_MIN)
    int walk_min = 0;           // MI3PT_OPT_WALK_MIN: walk while at least this many lanes walk; 0 = by the size of the tree (build_launch)
    int waves_per_cu = 0;       // one-wave workgroups per compute unit; 0 = what the kernel instantiation is compiled for (pt_kernels.h: 20 / 16)
    int top_packets = 64;       // MI3PT_TOP_PACKETS

    // Frame pipelining: raytrace kernels of consecutive frames run on two alternating
    // internal streams so that frame f+1 fills the CUs while frame f's last paths drain;
    // the ordered running mean (accumulate) stays on the main stream.
    bool pipeline = true;                // MI3PT_PIPELINE=0 turns it off (one fused kernel per frame)
    Stream rt_stream[2];
    Event rt_done[2], acc_done[3], main_mark;
    bool acc_done_valid[3] = { false, false, false };
    bool main_dirty = true;              // main-stream work the next raytrace kernel must wait for
    uint64_t seq = 0;

    // Deferred batching: RAYTRACE|ACCUMULATE frames are queued and up to batch_max consecutive
    // frames (identical uniforms except `frame`) run as ONE raytrace launch + one ordered
    // multi-frame accumulate, so the persistent kernel's drain tail is paid once per batch.
    // Anything that observes or changes device state flushes the queue first.
    struct PendingFrame {
        uint8_t u_rt[MI3PT_RAYTRACE_UNIFORMS_SIZE] = {}; uint8_t u_acc[MI3PT_ACCUMULATE_UNIFORMS_SIZE] = {};
        bool present = false;                                   // EXACT: the canvas is drawn after this frame's mean ...
        uint8_t u_fs[MI3PT_FULLSCREEN_UNIFORMS_SIZE] = {};      // ... with the pass's uniforms as they were at its submit
    };
    std::vector<PendingFrame> pending;
    int batch_limit_frames = 512;        // MI3PT_OPT_BATCH_LIMIT (512: a rank of an 8-way split runs its 320-frame job as ONE launch instead of 256 + 64: 11.16 instead of 11.62 ms, profiles/r03_d_job_split.log): upper bound of frames per launch, THIS context's (round 3 kept one value per process:
                                         // contexts other than the caller's went on with a stale capacity)
    int batch_max = 256;                 // MI3PT_BATCH (1 = no batching); x nranks for a tile split, see batch_limit().  16 -> 32: +3 % (fewer drains), 32 -> 64: +2 %, 64 -> 128: +1.5 %,
                                         // 128 -> 256 / 320: +0.3 ... +1 % (profiles/r04_s_batch_depth.log); a quarter of the free memory bounds it (recompute_batch_cap)
    // per-launch GPU time of the batched raytrace kernel (HIP events on its own stream)
    Event ev_rt[2][2];
    bool ev_rt_pending[2] = { false, false };
    double rt_total_ms = 0.0, rt_last_ms = 0.0;
    uint64_t rt_launches = 0, rt_frames = 0;
    int ev_rt_frames[2] = { 0, 0 };
    int ev_rt_newest = 0;                // parity of the most recent timed launch
    Event ev_span_start;                 // start of the first timed launch since the statistics were reset
    bool span_started = false;

    // Presentation (mi3pt_set_present_mode).  EXACT: every submit that includes FULLSCREEN gets its own accumulate and
    // fullscreen pass, in order, the canvas drawn from the mean up to and including that frame (the reference's
    // renderer.ts:379-390); up to present_depth such frames share one raytrace launch (launch_batch).
    // LATEST: the frame is queued like any other and the canvas is drawn from the running mean of
    // the batches launched so far -- and only when that mean (or the fullscreen uniforms) changed
    // since the last draw; a FULLSCREEN-only submit always launches the queue and shows everything.
    int present_mode = MI3PT_PRESENT_EXACT;
    int present_depth = 16;              // EXACT: presenting frames per raytrace launch (1 = a launch per frame)
    uint64_t accum_version = 1;          // bumped whenever d_accum (or what `output` points at) changes
    uint64_t presented_version = 0;      // accum_version the canvas was last drawn from
    bool want_present = false;           // LATEST: a requested draw is still owed to the canvas (frames were queued)
    uint8_t presented_fs[MI3PT_FULLSCREEN_UNIFORMS_SIZE] = {};

    bool timing = false;
    PassTimer pass_timer[3];             // raytrace (a launch mi3pt_submit runs at once), accumulate, fullscreen: of the last submit

    // what a resize keeps of the image features (the images themselves: ImageState)
    bool guided_despike = false;         // mi3pt_set_guided_despike: the state
    bool moments = false;                // mi3pt_set_moments: the moments image is kept
    bool moments_opted = false;          // mi3pt_set_moments(1) has been called: until then MI3PT_GUIDED_VARIANCE is an unknown flag bit, as it was before the image existed
    // The mean by count (mi3pt_set_mean_by_count): the accumulate kernels' by-count twins take a step's weight from the moments texel's n
    bool by_count = false;
    uint8_t aov_u[MI3PT_AOV_COUNT][MI3PT_RAYTRACE_UNIFORMS_SIZE] = {};      // the raytrace block each feature image was rendered from (mi3pt_reproject)
    // The previous geometry (mi3pt_keep_geometry, mi3pt_reproject_scene).  upload_epoch counts the uploads of triangles, BVH and materials (scene_epoch also
    // moves with the lazy analyses, which change no record); aov_epoch: its value when each feature image was rendered.  geometry_kept:
    // d_tris as it stood at kept_epoch is the previous geometry -- d_tris itself while d_tris_kept is null (nothing uploaded since), else
    // d_tris_kept, the buffer the first mi3pt_upload_triangles after the call handed over instead of freeing it.
    uint64_t upload_epoch = 0, kept_epoch = 0;
    uint64_t aov_epoch[MI3PT_AOV_COUNT] = {};
    bool geometry_kept = false;
    DevBuf<void> d_tris_kept;
    size_t ntris_kept = 0;
    // mi3pt_estimate_convergence: conv_done is recorded behind the copy of the most recent estimate -- what the two reads wait for, and nothing else
    Event conv_done;
    Stream conv_read_stream;             // the tile map's read-back, beside the context's stream (created by the first read)
    float conv_threshold = 0.0f;         // the last estimate's threshold
    int conv_min_frames = 0;             // ... and its min_frames (mi3pt_freeze_converged applies the rule with both)

    SceneFacts &scene_facts() { return *this; }
    const SceneFacts &scene_facts() const { return *this; }
    ImageState &images() { return *this; }
};
