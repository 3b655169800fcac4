// pt_ctx_launch.hip -- from "a frame was submitted" to "its kernels are enqueued": the frame queue, the batched launch, the read-outs of both.
#include "../../include/mi3pt.h"
#include "pt_ctx_calls.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

// the exact-packet wide walk `auto` falls back to where compressed packets could not be built: 10, 11 or 12 by the scene's statistics
// in the experiment build; release builds carry 10 only (11 / 12 were superseded by 13; all of them render the same bits)
static int auto_exact_wide(const mi3pt_ctx *ctx)
{
#ifdef MI3PT_EXPERIMENTS
    return ctx->auto_wide_variant;
#else
    (void)ctx;
    return 10;
#endif
}

// 0 = auto -> the persistent kernel; the probes only know the two per-ray walks.
static int pick_variant(const mi3pt_ctx *ctx)
{
    if (ctx->env_sampling) return 2;               // the dormant path lives in the per-pixel kernel only
    const bool defer_ok = ctx->leaf_cap >= 4;      // see mi3pt_upload_bvh: leaves may be tested out of order
    const bool cull_ok = ctx->cull_stack_ok && ctx->cull_ok && !ctx->cull_dirty;     // see prepare_cull (independent of defer_ok:
                                                                                       // the culling walks have their own stack scheme)
    const bool wide_ok = cull_ok && ctx->wide_ok;
    // auto: the wide walk pays once the tree no longer sits in L1 / L2 (demo scene, 2 k nodes: binary packets 10.4, wide
    // packets 10.2 Grays/s; dragon-class 8.5 -> 8.6; 10 M-triangle forest 24 -> 21 ms per frame)
    // ... and on COMPRESSED wide packets (13) wherever they could be built (every box nested and finite: any tree of the reference's
    // builder): half the bytes and half the loads per node step -- 10 M-triangle forest +29 %, the 870 k-triangle scene from close
    // up +7 %, its stated view +0.5 %, the demo scene +-0 (profiles/r04_g_cwide_ab.log); 10 / 11 / 12 stay for the trees that do not
    // admit it and as the diagnostic twin's walk
    if (ctx->variant == 0)
        return cull_ok && ctx->cull_enabled ? (wide_ok && ctx->wide_enabled ? (ctx->cwide_ok ? 13 : auto_exact_wide(ctx)) : 9) : (defer_ok ? 7 : 4);
    if (ctx->variant == 14 && cull_ok && ctx->cw8_ok) return 14;      // (its own packets and its own stack bound: independent of the 4-ary walk's)
    if ((ctx->variant == 13 || ctx->variant == 14) && wide_ok && ctx->cwide_ok) return 13;
    if ((ctx->variant == 13 || ctx->variant == 14) && !(wide_ok && ctx->cwide_ok)) return wide_ok ? auto_exact_wide(ctx) : (cull_ok ? 9 : (defer_ok ? 7 : 4));
    if (ctx->variant >= 10 && ctx->variant <= 12 && !wide_ok) return cull_ok ? 9 : (defer_ok ? 7 : 4);
    if (ctx->variant == 9 && !cull_ok) return defer_ok ? 7 : 4;
    if ((ctx->variant == 7 || ctx->variant == 8) && !defer_ok) return ctx->variant == 8 ? 6 : 4;
    return ctx->variant;
}

pt::AccUniforms acc_uniforms(const mi3pt_ctx *ctx)
{
    pt::AccUniforms a;
    a.res_w = ldu(ctx->u_acc, 0); a.res_h = ldu(ctx->u_acc, 4);
    a.frame = ldu(ctx->u_acc, 8); a.enabled = ldu(ctx->u_acc, 12);
    return a;
}

pt::Tile tile_of(const mi3pt_ctx *ctx)
{
    pt::Tile t;
    t.tex_w = ctx->width; t.tex_h = ctx->height; t.local_rows = ctx->local_rows;
    t.rank = ctx->rank; t.nranks = ctx->nranks; t.block_rows = ctx->block_rows;
    return t;
}

static pt::RtLaunch build_launch(const mi3pt_ctx *ctx, const uint8_t *u, const pt::AccUniforms &acc)
{
    pt::RtLaunch L;
    L.scene = scene_refs(ctx);
    L.un.res_x = ldf(u, 0); L.un.res_y = ldf(u, 4); L.un.aspect = ldf(u, 8);
    L.un.frame = ldu(u, 12);
    L.un.max_bounces = ldi(u, 16); L.un.samples_per_frame = ldi(u, 20);
    for (int k = 0; k < 3; k++) { L.un.cam_pos[k] = ldf(u, 32 + 4 * k); L.un.cam_dir[k] = ldf(u, 48 + 4 * k); }
    L.un.fov = ldf(u, 60); L.un.focal_distance = ldf(u, 64); L.un.aperture = ldf(u, 68);
    L.un.env_intensity = ldf(u, 80); L.un.env_rotation = ldf(u, 84);
    L.acc = acc;
    L.tile = tile_of(ctx);
    L.radiance = ctx->d_radiance;
    L.slot_pixels = plane_texels(ctx);
    L.nframes = 1;
    L.accum = ctx->d_accum;
    L.block_counters = ctx->d_block_counters;
    L.tile_counter = ctx->d_tile_counter;
    L.job_chunk = ctx->job_chunk;
    L.job_reverse = ctx->job_reverse;
    L.tri_pair = ctx->tri_pair;
    L.job_group = ctx->job_group;
    if (ctx->job_group < 0) {
        // jobs in groups of about an eighth of a frame's tiles (whole tile rows): all frames of a launch for
        // these tiles, then the next group -- what the waves fetch for one frame of a band of the image is
        // still in the L2s when they trace the next frame of it (1 GPU +1.7 %, a rank of an 8-way split +4.5 %)
        const int tiles_x = (L.tile.tex_w + 7) / 8, ntiles = tiles_x * ((L.tile.local_rows + 7) / 8);
        const int rows = ntiles / 8 / tiles_x;
        L.job_group = (rows < 1 ? 1 : rows) * tiles_x;
    }
    L.wave_times = ctx->d_wave_times;
    L.diag_lite = ctx->diag_lite;
    L.stack_overflow = ctx->d_stack_overflow;
    L.store_f16 = ctx->storage == MI3PT_STORAGE_F16;
    // walk_min: deep walks gain from a higher threshold -- more node steps between two service steps -- short ones lose
    // (profiles/r04_o_walkmin.log, 32 / 40 / 44 / 48: forest 1 678 / 1 756 / 1 792 / 1 806 Mrays/s, the 870 k-triangle scene from
    // close up 5 484 / 5 589 / 5 600 / 5 495, its stated view 16 110 / 16 000 / 15 930 / 15 690, demo 25 500 / 25 350 / 24 270 / 23 560):
    // 44 for trees of a million wide packets and more (deep walks from every camera) on compressed packets, 32 otherwise -- both
    // compile-time constants of their lean builds (as a launch parameter the threshold cost the other scenes 0.8 .. 1.5 %)
    L.walk_min = ctx->variant == 5 ? 48 : (ctx->walk_min > 0 ? ctx->walk_min
                                           : ((pick_variant(ctx) == 13 ? (ctx->nwide >= (1u << 20) && ctx->wide_ok && ctx->cwide_ok) : (pick_variant(ctx) == 14 && ctx->ncw8 >= (1u << 19))) ? PT_DEEP_WALK_MIN : PT_DEFAULT_WALK_MIN));
    L.leaf_min = ctx->leaf_min;
    L.shade_split = ctx->shade_split;
    L.tail_policy = ctx->tail_policy;
    L.drain_flag = nullptr;
    L.drain_seq = 0;
    L.waves_per_cu = ctx->waves_per_cu;
    L.num_cus = ctx->num_cus;
    L.service = nullptr;          // (batched launches: a slot of the context's ring, see launch_batch)
    L.cam_base = nullptr;         // (batched launches: launch_batch)
    L.ntiles_active = 0;          // (batched launches: launch_batch, sky_prepare)
    L.park = ctx->d_park;
    L.six_waves = ctx->six_waves;
    L.tile_cost = nullptr;        // (batched launches: launch_batch)
    L.tile_perm = nullptr;
    L.top_packets = ctx->top_packets;
    if (pick_variant(ctx) == 13 && (size_t)L.top_packets > ctx->nwide) L.top_packets = (int)ctx->nwide;      // (A/B builds that stage compressed packets in LDS)
    if (pick_variant(ctx) == 1) L.scene.tris = ctx->d_tris.as<const float4>();    // uploaded records, uploaded indices
    return L;
}

static pt::AccUniforms acc_from(const uint8_t *u)
{
    pt::AccUniforms a;
    a.res_w = ldu(u, 0); a.res_h = ldu(u, 4); a.frame = ldu(u, 8); a.enabled = ldu(u, 12);
    return a;
}

// Folds a finished batch launch's event pair into the launch statistics.
int collect_rt_time(mi3pt_ctx *ctx, int par)
{
    if (!ctx->ev_rt_pending[par]) return MI3PT_OK;
    HIP_TRY(ctx_event_sync(ctx, ctx->ev_rt[par][1]));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_rt[par][0], ctx->ev_rt[par][1]));
    ctx->rt_total_ms += ms;
    ctx->rt_last_ms = ms;
    ctx->rt_launches++;
    ctx->rt_frames += (uint64_t)ctx->ev_rt_frames[par];
    ctx->ev_rt_pending[par] = false;
    return MI3PT_OK;
}

// Makes sure parity `par`'s slot set can hold n frames.  One frame: a single slot (the interactive
// hosts never need more).  Up to eight frames: eight.  More: the full batch_cap at once, so a batching caller allocates once.
// Growing frees the old set (hipFree waits for the device, so nothing still reads it).
static int ensure_slots(mi3pt_ctx *ctx, int par /* slot set */, int n)
{
    if (ctx->slots_alloc[par] >= n) return MI3PT_OK;
    const size_t tex_bytes = plane_bytes(ctx);
    // one frame: one slot; up to eight: eight (a host that queues a few frames at a time does not pay for -- or wait
    // seconds for the allocation of -- 2 x 64 ... 256 full images it never fills); more: the full launch depth at
    // once, so that a batching caller allocates once and not again in the middle of its job
    int want = n <= 1 ? 1 : (n <= 8 ? 8 : ctx->batch_cap);
    if (want > ctx->batch_cap) want = ctx->batch_cap;
    if (want > n && tex_bytes) {
        // the cap was computed at resize; what is free NOW decides whether the full depth (for every slot set) is taken
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const size_t fit = (free_b / 2) / ((size_t)ctx->slot_sets * tex_bytes);
            if ((size_t)want > fit) want = fit > (size_t)n ? (int)fit : n;
        } else {
            (void)hipGetLastError();
        }
    }
    if (want < n) want = n;
    DevBuf<float4> fresh;
    hipError_t e = fresh.alloc(tex_bytes * (size_t)want);
    if (e != hipSuccess && want > n) {          // not enough memory for the full depth: take what this batch needs
        (void)hipGetLastError();
        want = n;
        e = fresh.alloc(tex_bytes * (size_t)want);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return pt_set_error(MI3PT_ERR_HIP, std::string("radiance slots: ") + hipGetErrorString(e));
    }
    ctx->d_slots[par] = std::move(fresh);
    ctx->slots_alloc[par] = want;
    // a caller that batches deeply will need the other set(s) at the same depth with its very next launch: allocate them
    // now, outside its steady state (the allocation of a gigabyte took ~0.4 ms of a 12 ms job otherwise)
    if (want == ctx->batch_cap && want > 8) {
        for (int other = 0; other < ctx->slot_sets; other++) {
            if (other == par || ctx->slots_alloc[other] >= want) continue;
            DevBuf<float4> more;
            if (more.alloc(tex_bytes * (size_t)want) != hipSuccess) { (void)hipGetLastError(); break; }
            ctx->d_slots[other] = std::move(more);
            ctx->slots_alloc[other] = want;
        }
    }
    return MI3PT_OK;
}

// The measuring launch has finished (or `wait`): build this rank's job order from the segments its tiles' paths traced, into the
// permutation buffer that is not in use.
static int cost_order_collect(mi3pt_ctx *ctx, bool wait)
{
    if (ctx->cost_state != 1) return MI3PT_OK;
    if (!wait) {
        const hipError_t q = hipEventQuery(ctx->cost_event);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); return MI3PT_OK; }
        if (q != hipSuccess) { (void)hipGetLastError(); ctx->cost_state = 0; return MI3PT_OK; }
    }
    const size_t n = ctx->cost_tiles;
    const int target = ctx->perm_cur ^ 1;
    ctx->cost_state = 0;        // (whatever goes wrong below: no order, measure again)
    std::vector<uint32_t> cost(n), perm(n);
    HIP_TRY(hipStreamWaitEvent(ctx->cost_stream, ctx->cost_event, 0));
    HIP_TRY(hipMemcpyAsync(cost.data(), ctx->d_tile_cost, n * 4, hipMemcpyDeviceToHost, ctx->cost_stream));
    HIP_TRY(hipStreamSynchronize(ctx->cost_stream));
    if (ctx->perm_used_valid[target]) HIP_TRY(hipEventSynchronize(ctx->perm_used[target]));      // (long done: two orders ago)
    // The order: the image's tiles from the bottom row up, as without the feature (what neighbouring waves fetch stays
    // close together: sorting ALL tiles by cost scattered them and cost 5 % -- profiles/r03_h_cost_order.log), except that
    // the cheapest quarter of the tiles is taken out and appended: the launch's last bands are then its cheapest tiles
    // wherever they lie in the image.
    std::vector<uint32_t> sorted(cost);
    const size_t q = n / 4;
    std::nth_element(sorted.begin(), sorted.begin() + (std::ptrdiff_t)q, sorted.end());
    const uint32_t cut = sorted[q];          // tiles cheaper than this go last (ties stay in the main part)
    size_t at = 0;
    if (ctx->cost_order == 2) {
        // every tile, costliest first (ties in image order): what a launch of ONE frame wants -- its time is its work plus its
        // longest paths' dependent chains, which then start at once instead of when their tile's turn comes
        for (size_t t = 0; t < n; t++) perm[t] = (uint32_t)t;
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
        at = n;
    } else {
        for (size_t t = n; t-- > 0;) if (cost[t] >= cut) perm[at++] = (uint32_t)t;
        for (size_t t = n; t-- > 0;) if (cost[t] < cut) perm[at++] = (uint32_t)t;
    }
    HIP_TRY(hipMemcpyAsync(ctx->d_tile_perm[target], perm.data(), n * 4, hipMemcpyHostToDevice, ctx->cost_stream));
    HIP_TRY(hipStreamSynchronize(ctx->cost_stream));
    ctx->perm_cur = target;
    ctx->cost_state = 2;
    return MI3PT_OK;
}

// Sets the launch's cost-order fields; `*measuring` / `*ordered`: what to record behind the launch.
static int cost_order_prepare(mi3pt_ctx *ctx, pt::RtLaunch &L, const uint8_t *u_rt, int variant, hipStream_t rs, bool *measuring, bool *ordered)
{
    *measuring = *ordered = false;
    const size_t n = (size_t)pt::raytrace_grid_blocks(L.tile);
    if (!ctx->cost_order || variant < 9 || variant > 13 || L.un.samples_per_frame != 1 || n < 2) return MI3PT_OK;
    uint8_t key[MI3PT_RAYTRACE_UNIFORMS_SIZE];
    std::memcpy(key, u_rt, sizeof key);
    std::memset(key + 12, 0, 4);          // the frame counter
    if (ctx->cost_tiles != n) {           // (resize / tile change: new arrays)
        HIP_TRY(ctx_stream_sync(ctx, ctx->rt_stream[0]));
        HIP_TRY(ctx_stream_sync(ctx, ctx->rt_stream[1]));
        for (DevBuf<uint32_t> *q : { &ctx->d_tile_cost, &ctx->d_tile_perm[0], &ctx->d_tile_perm[1] })
            HIP_TRY(q->alloc(n * 4));
        ctx->cost_tiles = n;
        ctx->cost_state = 0;
        ctx->perm_used_valid[0] = ctx->perm_used_valid[1] = false;
    }
    if (ctx->cost_state != 0 && std::memcmp(key, ctx->cost_key, sizeof key) != 0) ctx->cost_state = 0;      // the camera moved, bounces changed ...
    if (int rc = cost_order_collect(ctx, false)) return rc;
    if (ctx->cost_state == 0) {
        std::memcpy(ctx->cost_key, key, sizeof key);
        HIP_TRY(hipMemsetAsync(ctx->d_tile_cost, 0, n * 4, rs));
        L.tile_cost = ctx->d_tile_cost;
        *measuring = true;
    } else if (ctx->cost_state == 2) {
        L.tile_perm = ctx->d_tile_perm[ctx->perm_cur];
        L.job_reverse = 0;                // the order is the permutation's: costliest first
        *ordered = true;
    }
    return MI3PT_OK;
}

// The walk threshold by the view: reads what the most recent launch that has reported cost per ray (no wait: whatever has arrived).
#define WALK_ADAPT_ENTER 40.0
#define WALK_ADAPT_LEAVE 30.0
static void adapt_walk(mi3pt_ctx *ctx)
{
    if (!ctx->walk_adapt || !ctx->h_walk_stats) { ctx->deep_by_view = false; return; }
    volatile uint64_t *h = ctx->h_walk_stats;
    uint64_t best_seq = ctx->walk_stats_seen, box = 0, rays = 0;
    for (int par = 0; par < 2; par++) {
        const uint64_t s0 = __atomic_load_n(&ctx->h_walk_stats[4 * par], __ATOMIC_ACQUIRE);
        const uint64_t b = h[4 * par + 1], r = h[4 * par + 2];
        const uint64_t s1 = __atomic_load_n(&ctx->h_walk_stats[4 * par], __ATOMIC_ACQUIRE);
        if (s0 == s1 && s0 > best_seq && s0 <= ctx->walk_stats_seq) { best_seq = s0; box = b; rays = r; }
    }
    if (best_seq == ctx->walk_stats_seen) return;
    ctx->walk_stats_seen = best_seq;
    if (rays < 65536) return;              // (too small a launch to judge a view by)
    const double per_ray = (double)box / (double)rays;
    if (per_ray >= WALK_ADAPT_ENTER) ctx->deep_by_view = true;
    else if (per_ray <= WALK_ADAPT_LEAVE) ctx->deep_by_view = false;
}

// The empty tiles of this launch's view: sets L.tile_perm / L.ntiles_active to the list of the other tiles and returns the device list
// of the empty ones through *sky_list / *sky_count / *sky_samples (0: every tile is traced, the launch is what it was).  The split is
// used by the lean builds of the culling walks only (variants 9 - 14: their box-test counter is not pinned; 1 - 8 keep the oracle's exact
// counts and so trace every tile; the diagnostic twins and the per-pixel kernels keep tracing every pixel -- they are the on-device
// check), with the camera base at hand, without a cost order.  The host's classification (a millisecond or two at 1080p) runs at
// once for a launch of SKY_MIN_FRAMES frames or more, which hides it; a shallower launch -- an interactive host -- gets it once its camera
// has stood still for a launch, so that a host that moves the camera every frame never pays for it.
// With a sample mask (mi3pt_set_sample_mask) the same list carries the mask: [A: sampled and not empty | S: sampled and empty], composed by
// pt::compose_tile_lists -- the persistent kernel gets A wherever the launch can take a list (the conditions above but for the ones the
// empty tiles alone need: the cut, the camera base, two tiles or more), k_sky_samples gets S, and the ordered mean (k_accumulate_tiles)
// gets all of it through *acc_list / *acc_count on EVERY route.  Without a classification S is empty; with A empty S is the job list.
#define SKY_MIN_FRAMES 8
static void tile_key_of(const pt::Tile &tile, uint64_t mask_epoch, uint8_t key[104])
{
    const int32_t tl[6] = { tile.tex_w, tile.tex_h, tile.local_rows, tile.rank, tile.nranks, tile.block_rows };
    std::memcpy(key + 60, tl, sizeof tl);
    std::memcpy(key + 96, &mask_epoch, 8);
}

// ctx->sky_host = the lists for `key` (the mask as it stands; the classification in ctx->sky_empty if `classified`)
static void tile_lists_compose(mi3pt_ctx *ctx, const pt::Tile &tile, const uint8_t *u_rt, const uint8_t *key, bool classified)
{
    if (ctx->sky_list_valid && std::memcmp(key, ctx->sky_list_key, sizeof ctx->sky_list_key) == 0) return;
    // the in-bounds pixels of the empty tiles (the refill's test, raytrace.wgsl:425-427): each is one ray, one miss, one pixel per frame
    const double rx = u_rt ? ldf(u_rt, 0) : 0.0, ry = u_rt ? ldf(u_rt, 4) : 0.0;
    pt::TileListInput in;
    in.tex_w = tile.tex_w; in.tex_h = tile.tex_h; in.local_rows = tile.local_rows;
    in.rank = tile.rank; in.nranks = tile.nranks; in.block_rows = tile.block_rows;
    in.res_w = rx >= 1.0 ? (long long)std::min(rx, 4294967295.0) : 0;
    in.res_h = ry >= 1.0 ? (long long)std::min(ry, 4294967295.0) : 0;
    pt::TileLists out;
    pt::compose_tile_lists(in, ctx->mask.empty() ? nullptr : ctx->mask.data(), classified ? ctx->sky_empty.data() : nullptr, out);
    ctx->sky_host.swap(out.list);
    ctx->sky_host_active = out.active;
    ctx->sky_host_sky = out.sky;
    ctx->sky_host_pixels = out.sky_pixels;
    std::memcpy(ctx->sky_list_key, key, sizeof ctx->sky_list_key);
    ctx->sky_list_valid = true;
}

// lists[slot] = ctx->sky_host (composed for `key`), copied on `s` unless the slot holds that list already.  *staged = false: no
// memory for it (an unmasked launch then stays whole; under a mask the ordered mean cannot do without: `required`)
static int tile_lists_stage(mi3pt_ctx *ctx, int slot, const uint8_t *key, size_t ntiles, hipStream_t s, bool required, bool *staged)
{
    *staged = true;
    TileList &t = ctx->lists[slot];
    if (t.dev_valid && std::memcmp(key, t.dev_key, sizeof t.dev_key) == 0) return MI3PT_OK;
    if (!t.copied) HIP_TRY(hipEventCreateWithFlags(t.copied.put(), hipEventDisableTiming));
    if (t.copied_valid) HIP_TRY(hipEventSynchronize(t.copied));      // (long done: this slot's previous list)
    if (t.cap < ntiles) {
        DevBuf<uint32_t> fresh;
        if (fresh.alloc(ntiles * 4) != hipSuccess) {
            (void)hipGetLastError();
            *staged = false;
            return required ? pt_set_error(MI3PT_ERR_HIP, "no device memory for the sample mask's tile list") : MI3PT_OK;
        }
        t.d_list = std::move(fresh);          // (hipFree waits for the device: nothing still reads the old one)
        t.cap = ntiles;
    }
    t.dev_valid = false;
    t.staged = ctx->sky_host;
    // (an ordered mean of an earlier launch may still read the slot's list from the context's stream)
    if (t.read_valid) HIP_TRY(hipStreamWaitEvent(s, t.read, 0));
    if (!t.staged.empty())
        HIP_TRY(hipMemcpyAsync(t.d_list, t.staged.data(), t.staged.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(t.copied, s));
    t.copied_valid = true;
    std::memcpy(t.dev_key, key, sizeof t.dev_key);
    t.dev_valid = true;
    return MI3PT_OK;
}

static int sky_prepare(mi3pt_ctx *ctx, pt::RtLaunch &L, const uint8_t *u_rt, int par, int n, hipStream_t rs,
                       const uint32_t **sky_list, int *sky_count, uint64_t *sky_samples, const uint32_t **acc_list, int *acc_count)
{
    *sky_list = nullptr; *sky_count = 0; *sky_samples = 0;
    *acc_list = nullptr; *acc_count = 0;
    const bool masked = !ctx->mask.empty();
    const pt::RtRoute &r = ctx->last_route;
    const int ntiles = pt::raytrace_grid_blocks(L.tile);
    const bool takes_list = !L.tile_perm && !L.tile_cost && r.kind == 1 && r.lean && r.variant >= 9 && r.variant <= 14;
    const bool sky_ok = takes_list && ctx->sky_tiles && ctx->sky_cut_ok && !ctx->env_sampling && L.cam_base && ntiles >= 2;
    if (!masked && !sky_ok) return MI3PT_OK;
    uint8_t key[104];
    std::memset(key, 0, sizeof key);
    bool classified = false;
    if (sky_ok) {
        std::memcpy(key, u_rt, 12);                       // resolution, aspect
        std::memcpy(key + 12, u_rt + 32, 40);             // camera position, direction, fov, focal distance, aperture (32 .. 72)
        std::memcpy(key + 52, u_rt + 16, 8);              // maxBounces, samplesPerFrame
        tile_key_of(L.tile, 0, key);
        std::memcpy(key + 88, &ctx->scene_epoch, 8);
        classified = true;
        if (!ctx->sky_host_valid || std::memcmp(key, ctx->sky_key, sizeof key) != 0) {
            const bool stood_still = std::memcmp(key, ctx->sky_seen_key, sizeof key) == 0;
            std::memcpy(ctx->sky_seen_key, key, sizeof key);
            if (n < SKY_MIN_FRAMES && !stood_still) {
                classified = false;
            } else {
                (void)pt::sky_classify(ctx->sky_cut, true, u_rt, L.tile.tex_w, L.tile.local_rows, L.tile.tex_h,
                                       L.tile.rank, L.tile.nranks, L.tile.block_rows, ctx->sky_empty);
                std::memcpy(ctx->sky_key, key, sizeof key);
                ctx->sky_host_valid = true;
            }
        }
        if (!classified) {
            if (!masked) return MI3PT_OK;
            std::memset(key, 0, sizeof key);              // (the list of the mask alone)
        }
    }
    tile_key_of(L.tile, ctx->mask_epoch, key);
    tile_lists_compose(ctx, L.tile, u_rt, key, classified);
    const int active = ctx->sky_host_active, nsky = ctx->sky_host_sky;
    if (!masked && (nsky <= 0 || active <= 0)) return MI3PT_OK;          // (nothing to take out -- or nothing left: such a launch stays whole)
    if (active + nsky == 0) return MI3PT_OK;                             // (no tile is sampled: launch_batch launches nothing)
    bool staged = false;
    if (int rc = tile_lists_stage(ctx, par, key, (size_t)ntiles, rs, masked, &staged)) return rc;
    if (!staged) return MI3PT_OK;                                        // no memory: no split
    if (takes_list && active == 0) {                  // only empty tiles are sampled: they are the job list, no sky kernel
        L.tile_perm = ctx->lists[par].d_list;
        L.ntiles_active = nsky;
    } else if (takes_list && (nsky > 0 || active < ntiles)) {
        L.tile_perm = ctx->lists[par].d_list;
        L.ntiles_active = active;
        if (nsky > 0) {
            *sky_list = ctx->lists[par].d_list + active;
            *sky_count = nsky;
            *sky_samples = ctx->sky_host_pixels * (uint64_t)n;
        }
    }
    if (masked) {
        *acc_list = ctx->lists[par].d_list;
        *acc_count = active + nsky;
    }
    return MI3PT_OK;
}

// The list of the sampled tiles for an ordered mean that runs at once on the context's stream (mi3pt_submit's immediate path): slot 2
static int mask_list_main(mi3pt_ctx *ctx, const pt::Tile &tile, const uint32_t **list, int *count)
{
    *list = nullptr; *count = 0;
    uint8_t key[104];
    std::memset(key, 0, sizeof key);
    tile_key_of(tile, ctx->mask_epoch, key);
    tile_lists_compose(ctx, tile, nullptr, key, false);
    if (ctx->sky_host_active == 0) return MI3PT_OK;
    bool staged = false;
    if (int rc = tile_lists_stage(ctx, 2, key, (size_t)pt::raytrace_grid_blocks(tile), ctx->stream, true, &staged)) return rc;
    *list = ctx->lists[2].d_list;
    *count = ctx->sky_host_active;
    return MI3PT_OK;
}

// behind an ordered mean that read lists[slot]
static int mask_list_used(mi3pt_ctx *ctx, int slot)
{
    TileList &t = ctx->lists[slot];
    if (!t.read) HIP_TRY(hipEventCreateWithFlags(t.read.put(), hipEventDisableTiming));
    HIP_TRY(hipEventRecord(t.read, ctx->stream));
    t.read_valid = true;
    return MI3PT_OK;
}

int run_fullscreen(mi3pt_ctx *ctx, const uint8_t *u_fs)
{
    pt::FsUniforms fs;
    fs.res_x = ldf(u_fs, 0); fs.res_y = ldf(u_fs, 4); fs.aspect = ldf(u_fs, 8);
    fs.scaling = ldf(u_fs, 12); fs.denoise = ldu(u_fs, 16); fs.tonemapping = ldu(u_fs, 20);
    const float4 *tex = ctx->output_is_accum ? ctx->d_accum : ctx->last_radiance;
    if (ctx->timing) HIP_TRY(ctx->pass_timer[2].begin(ctx->stream));
    // (bit patterns compared: a NaN uniform must not rebuild the table every frame, and -0 is not +0 for a quotient)
    const bool taps_current = ctx->fs_taps_valid && std::memcmp(ctx->fs_taps_res, &fs.res_x, 4) == 0 && std::memcmp(ctx->fs_taps_res + 1, &fs.res_y, 4) == 0;
    pt::launch_fullscreen(fs, tex, ctx->width, ctx->height, ctx->width, ctx->height, ctx->d_fs_taps, taps_current, ctx->d_canvas,
                          ctx->d_canvas8, ctx->stream);
    if (hipError_t e = hipGetLastError()) {
        ctx->fs_taps_valid = false;
        return pt_set_error(MI3PT_ERR_HIP, std::string("fullscreen launch: ") + hipGetErrorString(e));
    }
    if (fs.denoise == 1u) { ctx->fs_taps_res[0] = fs.res_x; ctx->fs_taps_res[1] = fs.res_y; ctx->fs_taps_valid = true; }
    if (ctx->timing) HIP_TRY(ctx->pass_timer[2].end(ctx->stream));
    ctx->presented_version = ctx->accum_version;
    std::memcpy(ctx->presented_fs, u_fs, sizeof ctx->presented_fs);
    return MI3PT_OK;
}

// One launch: frames [first, first + n) of the queue as one raytrace kernel over (frame slot,
// tile) jobs on this parity's side stream, then the ordered multi-frame running mean on the
// main stream.
static int launch_batch(mi3pt_ctx *ctx, const mi3pt_ctx::PendingFrame *frames, int n)
{
    adapt_walk(ctx);
    const mi3pt_ctx::PendingFrame &first = frames[0];
    const pt::AccUniforms acc = acc_from(first.u_acc);
    pt::RtLaunch L = build_launch(ctx, first.u_rt, acc);
    const int variant = pick_variant(ctx);
    const bool f16 = ctx->storage == MI3PT_STORAGE_F16;
    const int par = (int)(ctx->seq & 1u);                        // stream, counters, queue head
    const int set = (int)(ctx->seq % (uint64_t)ctx->slot_sets);   // radiance slots
    if (int rc = ensure_slots(ctx, set, n)) {
        // a single slot always fits where the textures did; fall back to it before giving up
        if (n == 1 || ensure_slots(ctx, set, 1) != MI3PT_OK) return rc;
        ctx->batch_cap = 1;
        return MI3PT_ERR_STATE;      // caller re-chunks with the smaller cap
    }
    ctx->seq++;
    hipStream_t rs = ctx->rt_stream[par];
    if (ctx->main_dirty) {      // resets / rebinds queued on the main stream come first
        HIP_TRY(hipEventRecord(ctx->main_mark, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ctx->rt_stream[0], ctx->main_mark, 0));
        HIP_TRY(hipStreamWaitEvent(ctx->rt_stream[1], ctx->main_mark, 0));
        ctx->main_dirty = false;
    }
    // the ordered mean that last read this set of radiance slots (three batches ago) must be done
    if (ctx->acc_done_valid[set]) HIP_TRY(hipStreamWaitEvent(rs, ctx->acc_done[set], 0));
    L.radiance = ctx->d_slots[set];
    L.nframes = n;
    L.block_counters = ctx->d_block_counters + (size_t)par * ctx->nblocks * pt::CNT_COUNT;
    L.tile_counter = ctx->d_tile_counter + par * 32;
    L.stack_overflow = ctx->d_stack_overflow + (size_t)par * pt::PT_MAX_RESIDENT_WAVES * pt::SM_OVERFLOW_ENTRIES * 64;
    L.park = ctx->d_park + (size_t)par * pt::PT_MAX_RESIDENT_WAVES * 6 * 64;
    L.service = reinterpret_cast<pt::RtService *>(ctx->d_service + (size_t)((ctx->seq - 1) % SERVICE_SLOTS) * service_slot_bytes());
    bool cost_measuring = false, cost_ordered = false;
    if (int rc = cost_order_prepare(ctx, L, first.u_rt, variant, rs, &cost_measuring, &cost_ordered)) return rc;
    if (ctx->timing)
        if (int rc = collect_rt_time(ctx, par)) return rc;      // the launch of two batches ago
    // Hold this launch until the previous one (on the other stream) has handed out its last job:
    // its persistent waves then start to exit, and this launch's workgroups take the slots they
    // free.  Enqueued earlier, the kernel would sit in the dispatcher for the previous launch's
    // whole run -- same throughput, but event / profiler durations twice the execution time.
    const uint32_t seq_before = ctx->launch_seq;
    // (under a sample mask with no sampled tile -- mi3pt_set_sample_mask -- nothing is launched either: no raytrace, sky or accumulate kernel,
    // and, like the empty tile, no sequence number is taken at the gate, so no later launch waits for a mark nobody publishes)
    const bool masked = !ctx->mask.empty(), none_sampled = masked && ctx->mask_sampled == 0;
    const bool launches = pt::raytrace_grid_blocks(L.tile) > 0 && !none_sampled;       // (an empty tile launches nothing)
    // Only the state-machine kernel publishes a drain mark (pt_kernels.hip, the ticket draw).  A batch routed to the per-pixel
    // kernels -- launches beyond the packing limits, maxBounces >= 65536 -- gets its mark from the host side of its stream after
    // its last frame: left to a kernel that never stores it, the NEXT batch would wait for ever (round-4 advice).
    ctx->last_route = pt::raytrace_route(L, variant);          // (does not depend on the two fields set below)
    uint32_t publish_after = 0;
    if (ctx->gate_enabled && launches) {
        if (ctx->launch_seq != 0 &&
            hipStreamWaitValue32(rs, ctx->d_drain_flag, ctx->launch_seq, hipStreamWaitValueGte, 0xffffffffu) != hipSuccess) {
            // no stream memory operations here: launches simply queue behind each other from now on
            (void)hipGetLastError();
            ctx->gate_enabled = false;
        } else if (ctx->last_route.kind == 1) {
            ++ctx->launch_seq;
            if (!ctx->debug_suppress_drain) { L.drain_flag = ctx->d_drain_flag; L.drain_seq = ctx->launch_seq; }
        } else {
            publish_after = ++ctx->launch_seq;
        }
    }
    // The pixel-only part of the camera rays (RtLaunch::cam_base), formed once per camera / size / tile for this parity's stream:
    // every frame of every later launch with the same camera loads it.  A host that moves the camera per frame pays one
    // full-width pass over the pixels per launch instead of the same arithmetic at ~30 of 64 lanes inside the launch.
    if (ctx->cam_base_enabled && ctx->last_route.kind == 1 && launches) {
        uint8_t key[80];
        std::memset(key, 0, sizeof key);
        std::memcpy(key, first.u_rt, 12);                 // resolution, aspect
        std::memcpy(key + 12, first.u_rt + 32, 36);       // camera position, direction, fov, focal distance (32 .. 68)
        const int32_t tl[6] = { L.tile.tex_w, L.tile.tex_h, L.tile.local_rows, L.tile.rank, L.tile.nranks, L.tile.block_rows };
        std::memcpy(key + 48, tl, sizeof tl);
        if (!ctx->d_cam_base[par]) {
            if (ctx->d_cam_base[par].alloc(L.slot_pixels * sizeof(float4)) != hipSuccess) {
                (void)hipGetLastError();
                ctx->cam_base_enabled = false;            // no memory for it: the kernel forms the rays itself, as before
            }
            ctx->cam_base_valid[par] = false;
        }
        if (ctx->d_cam_base[par]) {
            if (!ctx->cam_base_valid[par] || std::memcmp(key, ctx->cam_base_key[par], sizeof key) != 0) {
                pt::launch_camera_base(L, ctx->d_cam_base[par], rs);
                std::memcpy(ctx->cam_base_key[par], key, sizeof key);
                ctx->cam_base_valid[par] = true;
            }
            L.cam_base = ctx->d_cam_base[par];
        }
    }
    // the tiles whose camera rays reach no geometry leave the job list
    const uint32_t *sky_list = nullptr;
    int sky_count = 0;
    uint64_t sky_samples = 0;
    const uint32_t *acc_list = nullptr;      // under a sample mask: the sampled tiles, for the ordered mean
    int acc_count = 0;
    if (launches)
        if (int rc = sky_prepare(ctx, L, first.u_rt, par, n, rs, &sky_list, &sky_count, &sky_samples, &acc_list, &acc_count)) return rc;
    // the walk threshold by the view (adapt_walk): the deep-walk build for a launch of the shipped walk long enough to run its six-wave form
    // (>= 250 k jobs: a short launch -- an interactive host's single frames -- is all ramp and drain, and keeps the ordinary build.  Counted in
    // tiles of the FRAME, empty ones included: which of the two builds a view gets does not depend on how much sky it shows --
    // tests/test_gpu_configs.py::test_walk_threshold_follows_the_view pins the sequence; the grid and the six-wave choice count the real jobs)
    if (ctx->deep_by_view && ctx->walk_min == 0 && L.walk_min == PT_DEFAULT_WALK_MIN && variant == 13 &&
        (long long)pt::raytrace_grid_blocks(L.tile) * n >= 250000)
        L.walk_min = PT_DEEP_WALK_MIN;
    ctx->last_route = pt::raytrace_route(L, variant);          // (the grid and the build follow the number of jobs)
    if (!none_sampled) pt::launch_raytrace_setup(L, ctx->last_route, rs);
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev_rt[par][0], rs));
        if (!ctx->span_started) { HIP_TRY(hipEventRecord(ctx->ev_span_start, rs)); ctx->span_started = true; }
    }
    // (in front of the persistent kernel: it runs while the predecessor's last paths drain -- +0.4 % over behind it, where it would follow this
    // launch's own drain: profiles/sky_tiles_ab.log)
    if (sky_count && ctx->sky_tiles != 2) pt::launch_sky_samples(L, sky_list, sky_count, sky_samples, rs);
    if (!none_sampled) pt::launch_raytrace(L, ctx->last_route, false, rs);
    if (sky_count && ctx->sky_tiles == 2) pt::launch_sky_samples(L, sky_list, sky_count, sky_samples, rs);
    if (publish_after && !ctx->debug_suppress_drain && hipStreamWriteValue32(rs, ctx->d_drain_flag, publish_after, 0) != hipSuccess) {
        (void)hipGetLastError();
        ctx->gate_enabled = false;          // (the next batch enqueues no wait; a batch already held is released by ctx_wait)
    }
    if (cost_measuring && launches) { HIP_TRY(hipEventRecord(ctx->cost_event, rs)); ctx->cost_state = 1; }
    if (cost_ordered && launches) { HIP_TRY(hipEventRecord(ctx->perm_used[ctx->perm_cur], rs)); ctx->perm_used_valid[ctx->perm_cur] = true; }
    if (hipError_t e = hipGetLastError()) {
        // The kernel that would have published drain_seq never ran: publish it from the host side
        // of the stream instead, so that neither a later launch nor mi3pt_destroy waits for it.
        if (ctx->launch_seq != seq_before && hipStreamWriteValue32(rs, ctx->d_drain_flag, ctx->launch_seq, 0) != hipSuccess) {
            (void)hipGetLastError();
            ctx->launch_seq = seq_before;
            ctx->gate_enabled = false;
        }
        return pt_set_error(MI3PT_ERR_HIP, std::string("raytrace launch: ") + hipGetErrorString(e));
    }
    if (ctx->timing) {
        HIP_TRY(hipEventRecord(ctx->ev_rt[par][1], rs));
        ctx->ev_rt_pending[par] = true;
        ctx->ev_rt_frames[par] = n;
        ctx->ev_rt_newest = par;
    }
    // what this launch cost per ray, for the choice of a later launch's build (adapt_walk): behind the launch on its own stream, in front of the
    // event the ordered mean waits for -- the report is there at every sync point (the rays of the empty tiles' samples are in the same counter set)
    if (ctx->walk_adapt && ctx->h_walk_stats && launches && ctx->last_route.kind == 1 && ctx->last_route.lean && ctx->last_route.variant == 13 && ctx->walk_min == 0) {
        pt::launch_walk_stats(L.block_counters, ctx->nblocks, ctx->d_walk_prev + 2 * par, ctx->d_walk_stats + 4 * par, ++ctx->walk_stats_seq, rs);
        (void)hipGetLastError();
    }
    HIP_TRY(hipEventRecord(ctx->rt_done[par], rs));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->rt_done[par], 0));
    // The ordered mean, a run of frames at a time: a run ends with a frame whose canvas is wanted (EXACT presentation) or
    // with the launch -- all n frames in one pass unless frames present, one pass + one fullscreen pass per presenting frame.
    ctx->last_radiance = L.radiance + (size_t)(n - 1) * L.slot_pixels;
    ctx->output_is_accum = true;
    for (int k = 0; k < n;) {
        int e = k;
        while (e < n - 1 && !frames[e].present) e++;
        const bool last_run = e == n - 1;
        pt::AccUniforms a = acc;
        a.frame = acc.frame + (uint32_t)k;
        if (ctx->timing && last_run) HIP_TRY(ctx->pass_timer[1].begin(ctx->stream));
        if (masked) {        // the sampled tiles only: a frozen tile's mean and moments keep their bits
            pt::launch_accumulate_tiles(a, L.tile, acc_list, acc_count, L.radiance + (size_t)k * L.slot_pixels, L.slot_pixels, e - k + 1, ctx->d_accum,
                                        ctx->d_moments, f16, ctx->by_count, ctx->stream);
        } else {
            pt::launch_accumulate_frames(a, L.tile, L.radiance + (size_t)k * L.slot_pixels, L.slot_pixels, e - k + 1, ctx->d_accum, ctx->d_moments, f16, ctx->by_count, 4096, ctx->stream);
        }
        HIP_TRY(hipGetLastError());
        if (ctx->timing && last_run) HIP_TRY(ctx->pass_timer[1].end(ctx->stream));
        ctx->accum_version++;
        if (frames[e].present)
            if (int rc = run_fullscreen(ctx, frames[e].u_fs)) return rc;
        k = e + 1;
    }
    if (masked && acc_count)
        if (int rc = mask_list_used(ctx, par)) return rc;
    HIP_TRY(hipEventRecord(ctx->acc_done[set], ctx->stream));
    ctx->acc_done_valid[set] = true;
    return MI3PT_OK;
}

// Launches everything that is queued, batch_cap frames at a time.  The queue is emptied even on
// failure (the frames are lost with the error; the context stays usable).
int flush_pending(mi3pt_ctx *ctx)
{
    if (ctx->pending.empty()) return MI3PT_OK;
    std::vector<mi3pt_ctx::PendingFrame> q;
    q.swap(ctx->pending);
    size_t at = 0;
    while (at < q.size()) {
        int n = (int)(q.size() - at);
        if (n > ctx->batch_cap) n = ctx->batch_cap;
        const int rc = launch_batch(ctx, &q[at], n);
        if (rc == MI3PT_ERR_STATE && n > 1) continue;       // the slot memory shrank batch_cap: retry smaller
        if (rc != MI3PT_OK) return rc;
        at += (size_t)n;
    }
    return MI3PT_OK;
}

// Every entry point that observes or changes device state goes through this.
int require_idle(mi3pt_ctx *ctx)
{
    if (int rc = require_ctx(ctx)) return rc;
    return flush_pending(ctx);
}

// Can `next` join the queued frames?  Same uniforms, consecutive frame numbers.
static bool batch_compatible(const mi3pt_ctx::PendingFrame &last, const mi3pt_ctx::PendingFrame &next)
{
    if (std::memcmp(last.u_rt, next.u_rt, 12) || std::memcmp(last.u_rt + 16, next.u_rt + 16, 80)) return false;
    if (std::memcmp(last.u_acc, next.u_acc, 8) || std::memcmp(last.u_acc + 12, next.u_acc + 12, 4)) return false;
    return ldu(next.u_rt, 12) == ldu(last.u_rt, 12) + 1u && ldu(next.u_acc, 8) == ldu(last.u_acc, 8) + 1u;
}

extern "C" int mi3pt_submit(mi3pt_ctx *ctx, unsigned pass_mask)
{
    PT_GROUP(ctx, group_submit_frames(ctx, pass_mask, 1));
    if (int rc = require_ctx(ctx)) return rc;
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "submit before resize");
    if (pass_mask & ~(MI3PT_SUBMIT_RAYTRACE | MI3PT_SUBMIT_ACCUMULATE | MI3PT_SUBMIT_FULLSCREEN))
        return pt_set_error(MI3PT_ERR_INVALID, "unknown bits in pass_mask");
    const bool do_rt = pass_mask & MI3PT_SUBMIT_RAYTRACE, do_acc = pass_mask & MI3PT_SUBMIT_ACCUMULATE;
    const bool do_fs = pass_mask & MI3PT_SUBMIT_FULLSCREEN;
    if (do_fs && ctx->partial())
        return pt_set_error(MI3PT_ERR_STATE,
                            "the fullscreen pass needs the whole image: gather the tiles into a 1-rank context");
    if (do_rt) {
        if (int rc = check_scene(ctx)) return rc;
        if (int rc = prepare_layout(ctx)) return rc;    // (no-ops unless the scene changed)
        if (int rc = prepare_cull(ctx)) return rc;
    }
    const pt::Tile tile = tile_of(ctx);
    const pt::AccUniforms acc = acc_uniforms(ctx);
    const bool f16 = ctx->storage == MI3PT_STORAGE_F16;
    const int variant = pick_variant(ctx);
    const bool same_region = acc.res_w == (uint32_t)ldf(ctx->u_rt, 0) && acc.res_h == (uint32_t)ldf(ctx->u_rt, 4);
    const bool lazy_present = ctx->present_mode == MI3PT_PRESENT_LATEST;
    bool acc_done = false, drawn_with_frame = false;

    if (do_rt && do_acc && same_region && ctx->pipeline && variant >= 4) {
        // queued: runs with its neighbours as one batch (see flush_pending)
        mi3pt_ctx::PendingFrame f;
        std::memcpy(f.u_rt, ctx->u_rt, sizeof f.u_rt);
        std::memcpy(f.u_acc, ctx->u_acc, sizeof f.u_acc);
        if (!ctx->pending.empty() && !batch_compatible(ctx->pending.back(), f))
            if (int rc = flush_pending(ctx)) return rc;
        if (ctx->pending.empty()) for (PassTimer &t : ctx->pass_timer) t.forget();
        int depth = ctx->batch_cap;
        if (do_fs && !lazy_present) {          // EXACT: this frame's canvas is drawn behind its mean (launch_batch)
            f.present = true;
            std::memcpy(f.u_fs, ctx->u_fs, sizeof f.u_fs);
            if (depth > ctx->present_depth) depth = ctx->present_depth;
            drawn_with_frame = true;
        }
        ctx->pending.push_back(f);
        if ((int)ctx->pending.size() >= depth)
            if (int rc = flush_pending(ctx)) return rc;
        acc_done = true;
    } else {
        if (int rc = flush_pending(ctx)) return rc;      // anything but a queued frame runs after the queue
        for (PassTimer &t : ctx->pass_timer) t.forget();
        if (do_rt) {
            pt::RtLaunch L = build_launch(ctx, ctx->u_rt, acc);
            // Fuse when the accumulate pass covers exactly the pixels the raytrace pass writes (the per-pixel kernels; the
            // state-machine kernel writes the frame's radiance and the accumulate pass follows as a kernel of its own: same bits).
            // (not with the moments image: the per-pixel kernels do not keep it, the two passes run separately -- same bits)
            // (nor under a sample mask: the fused kernels step every texel)
            const bool fused = do_acc && same_region && pt::raytrace_variant_fuses(variant) && !ctx->d_moments && ctx->mask.empty();
            // (the service block of a launch that runs at once: its own slot -- launches on the main stream follow each other,
            // and the batches launched before it are waited for by this stream)
            L.service = reinterpret_cast<pt::RtService *>(ctx->d_service + (size_t)SERVICE_SLOTS * service_slot_bytes());
            L.block_counters = ctx->d_block_counters;
            ctx->last_route = pt::raytrace_route(L, variant);
            pt::launch_raytrace_setup(L, ctx->last_route, ctx->stream);
            if (ctx->timing) HIP_TRY(ctx->pass_timer[0].begin(ctx->stream));
            pt::launch_raytrace(L, ctx->last_route, fused, ctx->stream);
            HIP_TRY(hipGetLastError());
            if (ctx->timing) HIP_TRY(ctx->pass_timer[0].end(ctx->stream));
            ctx->last_radiance = ctx->d_radiance;
            ctx->output_is_accum = fused;
            ctx->main_dirty = true;     // a later batch must not overtake this kernel
            ctx->accum_version++;
            acc_done = fused;
        }
    }
    if (do_acc && !acc_done) {
        if (ctx->timing) HIP_TRY(ctx->pass_timer[1].begin(ctx->stream));
        if (!ctx->mask.empty()) {
            const uint32_t *list = nullptr;
            int count = 0;
            if (int rc = mask_list_main(ctx, tile, &list, &count)) return rc;
            pt::launch_accumulate_tiles(acc, tile, list, count, ctx->last_radiance, 0, 1, ctx->d_accum, ctx->d_moments, f16, ctx->by_count, ctx->stream);
            if (count)
                if (int rc = mask_list_used(ctx, 2)) return rc;
        } else {
            pt::launch_accumulate_frames(acc, tile, ctx->last_radiance, 0, 1, ctx->d_accum, ctx->d_moments, f16, ctx->by_count, 2048, ctx->stream);
        }
        HIP_TRY(hipGetLastError());
        if (ctx->timing) HIP_TRY(ctx->pass_timer[1].end(ctx->stream));
        ctx->output_is_accum = true;   // accumulate.ts:171-175 copies the mean into outputTexture
        ctx->main_dirty = true;
        ctx->accum_version++;
    }
    if (do_fs && !drawn_with_frame) {
        // LATEST: frames may still be queued; the canvas is drawn from what has been launched, and
        // only if that (or the pass's uniforms) changed since the last draw.  What is still queued
        // is owed: a canvas read-back (or a FULLSCREEN-only submit) draws it.
        const bool current = ctx->presented_version == ctx->accum_version &&
                             std::memcmp(ctx->presented_fs, ctx->u_fs, sizeof ctx->u_fs) == 0;
        if (lazy_present && current) {
            if (!ctx->pending.empty()) ctx->want_present = true;
            return MI3PT_OK;
        }
        if (int rc = run_fullscreen(ctx, ctx->u_fs)) return rc;
        ctx->want_present = lazy_present && !ctx->pending.empty();
    }
    return MI3PT_OK;
}

// `count` consecutive frames in one call: what `count` calls of Renderer.render() submit while
// nothing but the frame counter changes (renderer.ts:369-377 increments it before the uniforms
// are written) -- frame i runs with raytrace `frame` = current + i and accumulate `frame` =
// current + i, and both blocks are left at current + count, ready for the next call.
extern "C" int mi3pt_submit_frames(mi3pt_ctx *ctx, unsigned pass_mask, uint32_t count)
{
    PT_GROUP(ctx, group_submit_frames(ctx, pass_mask, count));
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    const bool queues_only = (pass_mask & ~(MI3PT_SUBMIT_RAYTRACE | MI3PT_SUBMIT_ACCUMULATE)) == 0;
    for (uint32_t i = 0; i < count; i++) {
        const size_t queued_before = ctx->pending.size();
        if (int rc = mi3pt_submit(ctx, pass_mask)) return rc;
        uint32_t f = ldu(ctx->u_rt, 12) + 1u, g = ldu(ctx->u_acc, 8) + 1u;
        std::memcpy(ctx->u_rt + 12, &f, 4);
        std::memcpy(ctx->u_acc + 8, &g, 4);
        // That submit QUEUED its frame (the ordinary case: raytrace + accumulate, pipelined): the frames behind it differ from it in
        // the frame counters alone and join the queue as copies -- what mi3pt_submit would do for each of them after checking the
        // scene, the variant and the batch compatibility again (0.3 ms of a rank's 9.6 ms job for 256 frames, before anything was
        // launched: profiles/r04_e_rank_job_host.log).  The queue is launched at the same depth as there.
        // INVARIANT this fast path rests on (round-4 advice): between two frames INSIDE this call nothing can change -- no upload, no
        // uniform other than the two frame counters, no option, no resize: single-threaded entry, and every such change is an entry
        // point of its own -- so batch_compatible, check_scene and the prepare_* steps, which that first mi3pt_submit just ran, would
        // give the same answers for every copy.  tests/test_gpu_gate.py holds it to `count` separate submits across a capacity
        // boundary and with the cost-ordered job lists (whose per-launch state flush_pending advances, as for separate submits).
        if (queues_only && ctx->pending.size() == queued_before + 1) {
            while (i + 1 < count && (int)ctx->pending.size() < ctx->batch_cap) {
                mi3pt_ctx::PendingFrame nf = ctx->pending.back();
                std::memcpy(nf.u_rt + 12, &f, 4);
                std::memcpy(nf.u_acc + 8, &g, 4);
                ctx->pending.push_back(nf);
                f++; g++; i++;
                std::memcpy(ctx->u_rt + 12, &f, 4);
                std::memcpy(ctx->u_acc + 8, &g, 4);
            }
            if ((int)ctx->pending.size() >= ctx->batch_cap)
                if (int rc = flush_pending(ctx)) return rc;
        }
    }
    return MI3PT_OK;
}

extern "C" int mi3pt_flush(mi3pt_ctx *ctx)
{
    PT_GROUP(ctx, group_flush(ctx));
    return require_idle(ctx);
}

extern "C" int mi3pt_batch_capacity(mi3pt_ctx *ctx, int *frames)
{
    PT_GROUP(ctx, mi3pt_batch_capacity(group_member0(ctx), frames));
    if (!ctx || !frames) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (ctx->width == 0) return pt_set_error(MI3PT_ERR_STATE, "no textures before resize");
    *frames = ctx->pipeline ? ctx->batch_cap : 1;
    return MI3PT_OK;
}

extern "C" int mi3pt_sync(mi3pt_ctx *ctx)
{
    PT_GROUP(ctx, group_sync(ctx));
    if (int rc = require_idle(ctx)) return rc;
    HIP_TRY(ctx_stream_sync(ctx, ctx->stream));
    return cost_order_collect(ctx, false);      // (a measuring launch has finished by now: its job order is ready for the next launch)
}

extern "C" int mi3pt_raytrace_launch_stats(mi3pt_ctx *ctx, int reset, double *total_ms, uint64_t *launches,
                                           uint64_t *frames)
{
    PT_GROUP(ctx, group_launch_stats(ctx, reset, total_ms, launches, frames));
    if (int rc = require_idle(ctx)) return rc;
    if (int rc = collect_rt_time(ctx, ctx->ev_rt_newest ^ 1)) return rc;
    if (int rc = collect_rt_time(ctx, ctx->ev_rt_newest)) return rc;
    if (total_ms) *total_ms = ctx->rt_total_ms;
    if (launches) *launches = ctx->rt_launches;
    if (frames) *frames = ctx->rt_frames;
    if (reset) { ctx->rt_total_ms = 0.0; ctx->rt_launches = 0; ctx->rt_frames = 0; ctx->span_started = false; }
    return MI3PT_OK;
}

// Wall-clock span of the batched raytrace launches since the last reset of the launch statistics:
// from the start of the first to the end of the last, on the GPU's clock.  Consecutive launches
// overlap at their tails (the next one starts while the last paths of this one drain), so the
// sum of the per-launch durations exceeds this; span / launches is the non-overlapped time a
// launch costs.
extern "C" int mi3pt_raytrace_launch_span(mi3pt_ctx *ctx, double *span_ms)
{
    PT_GROUP(ctx, group_launch_span(ctx, span_ms));
    if (int rc = require_idle(ctx)) return rc;
    if (!span_ms) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    *span_ms = 0.0;
    if (!ctx->span_started) return MI3PT_OK;
    for (int par = 0; par < 2; par++) {
        if (!ctx->ev_rt_frames[par]) continue;              // this parity never ran a timed launch
        HIP_TRY(ctx_event_sync(ctx, ctx->ev_rt[par][1]));
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ctx->ev_span_start, ctx->ev_rt[par][1]) != hipSuccess) { (void)hipGetLastError(); continue; }
        if ((double)ms > *span_ms) *span_ms = ms;
    }
    return MI3PT_OK;
}

// Which kernel variant a raytrace submit would run right now (after the lazy scene analyses): the
// selected one, or what it falls back to when the scene does not admit it.
extern "C" int mi3pt_debug_active_variant(mi3pt_ctx *ctx, int *variant)
{
    PT_GROUP(ctx, mi3pt_debug_active_variant(group_member0(ctx), variant));
    if (!ctx || !variant) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = require_idle(ctx)) return rc;
    if (int rc = check_scene(ctx)) return rc;
    if (int rc = prepare_layout(ctx)) return rc;
    if (int rc = prepare_cull(ctx)) return rc;
    *variant = pick_variant(ctx);
    return MI3PT_OK;
}

extern "C" int mi3pt_debug_last_launch(mi3pt_ctx *ctx, int *kind, int *variant, int *lean, int *workgroups)
{
    PT_GROUP(ctx, mi3pt_debug_last_launch(group_member0(ctx), kind, variant, lean, workgroups));
    if (!ctx) return pt_set_error(MI3PT_ERR_INVALID, "null context");
    if (kind) *kind = ctx->last_route.kind;
    if (variant) *variant = ctx->last_route.variant;
    if (lean) *lean = ctx->last_route.lean ? 1 : 0;
    if (workgroups) *workgroups = ctx->last_route.blocks;
    return MI3PT_OK;
}
