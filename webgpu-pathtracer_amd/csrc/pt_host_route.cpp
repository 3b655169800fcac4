// pt_host_route.cpp -- which kernel a raytrace launch runs, and on how many workgroups: decided once, here, in plain host C++
// (raytrace_route).  The context keeps the answer (last_route: what mi3pt_debug_last_launch / MI3PT_OPT_LAST_BUILD report) and hands it to
// launch_raytrace_setup / launch_raytrace (pt_kernels.hip), which map a route to a kernel and decide nothing.  mi3pt_host_route: the same
// function on flat inputs, without a context or a device (tests/test_route_table.py; recorded by profiles/route_move_record.py).
#include "../../include/mi3pt.h"
#include "pt_internal.h"

namespace pt {

int raytrace_persistent_blocks(const Tile &tile, int nframes, int waves_per_cu, int num_cus, bool tuned, int waves_per_simd, int job_tiles)
{
    const int ntiles = job_tiles > 0 ? job_tiles : raytrace_grid_blocks(tile);
    const long long jobs = (long long)ntiles * (nframes > 0 ? nframes : 1);
    if (num_cus <= 0) num_cus = 256;
    if (waves_per_simd <= 0) waves_per_simd = tuned ? SM_TUNED_WAVES_PER_SIMD : SM_OTHER_WAVES_PER_SIMD;
    if (waves_per_cu > 4 * waves_per_simd) waves_per_cu = 0;          // (more than the build can keep resident: its own width)
    if (waves_per_cu <= 0 || waves_per_cu > PT_MAX_WAVES_PER_CU) {
        waves_per_cu = 4 * waves_per_simd;
        // A small launch (an interactive host: one or two frames, or a small image) gets fewer waves: at least 8 jobs each,
        // at least 4 per CU.  With a handful of jobs per wave a launch is all ramp and drain, and a launch that fills every
        // wave slot keeps its successor out until its own waves exit; narrower launches overlap.  One 1080p frame per
        // launch: 16 waves per CU, -6 % time; 640 x 360: 4, -20 % (profiles/r03_k_small_launches.log; fewer still is
        // faster on the default scene and slower on every other one tried: MI3PT_OPT_WAVES_PER_CU)
        // Up to ~3 frames of 1080p per launch, 16 per CU beats 20 on every scene tried (-5 ... -12 %: the successor finds
        // four wave slots per CU free from the start); from 4 frames on the full width wins.
        const long long want = (jobs + (long long)num_cus * 8 - 1) / ((long long)num_cus * 8);
        if (want < 16) waves_per_cu = want < 4 ? 4 : (int)want;
        else if (want < 48 && waves_per_cu > 16) waves_per_cu = 16;
    }
    int resident = num_cus * waves_per_cu;                            // the device's own CU count (hipDeviceProp_t)
    if (resident > PT_MAX_RESIDENT_WAVES) resident = PT_MAX_RESIDENT_WAVES;
    // One wave per JOB at most -- (frame slot, tile) pairs, not tiles of one frame.  Until round 4 this read `ntiles`: a rank of an
    // 8-way split of 1080p has 17 x 240 = 4 080 tiles per frame, so its 512-frame launches ran 4 080 of the 5 120 wave slots
    // (16 instead of 20 per CU) -- the "unexplained +14 % per pixel" of a rank of eight (profiles/r04_a_rank_penalty.log:
    // fewer wave cycles per ray than the whole image, yet more time per ray).
    return jobs < (long long)resident ? (int)jobs : resident;
}

int raytrace_grid_blocks(const Tile &tile)
{
    const int tiles_x = (tile.tex_w + 7) / 8;
    const int tiles_y = (tile.local_rows + 7) / 8;
    return tiles_x * tiles_y;
}

// Tiles of a frame that the state-machine kernel is given as jobs: all of them, or the launch's active list
int raytrace_job_tiles(const RtLaunch &L)
{
    return L.ntiles_active > 0 ? L.ntiles_active : raytrace_grid_blocks(L.tile);
}

// Frame slot and bounce share a word in the state-machine kernel, and the sample count of a multi-sample frame is a float in the
// pixel's texel: launches beyond these (absurd) limits run the per-pixel kernel, frame by frame.
static bool launch_packs(const RtLaunch &L)
{
    return L.un.max_bounces < 65536 && L.nframes <= 65535 && L.un.samples_per_frame <= 16777216;
}
// The lean build (DIAG = false: no step statistics, the step-voting options as constants, the service step's scalars in
// memory) runs unless a diagnostic buffer is bound or a step-voting option was changed (mi3pt_debug_set_option).
static bool launch_is_lean(const RtLaunch &L)
{
    return (!L.wave_times || L.diag_lite) && !L.tile_cost && (L.walk_min == PT_DEFAULT_WALK_MIN || L.walk_min == PT_DEEP_WALK_MIN) && L.leaf_min == PT_DEFAULT_LEAF_MIN && L.shade_split == PT_DEFAULT_SHADE_SPLIT &&
           L.tail_policy == PT_DEFAULT_TAIL_POLICY && L.job_chunk == PT_DEFAULT_JOB_CHUNK && L.tri_pair == 1 && L.service != nullptr;
}
// What the lean builds of the culling walks have as constants (ASSUME in the kernel): a scene with nodes whose root is an
// internal node with a guard-range box, and a resolution of ordinary magnitude.  Every tree the culling walks are offered for
// has nodes and an internal root; the rest fails for scenes ~1e18 across or images ~1e12 wide.
static bool launch_assumptions_hold(const RtLaunch &L)
{
    return L.scene.nnodes != 0 && (L.scene.flags & 1u) != 0u && (L.scene.root_ref & REF_LEAF) == 0u &&
           L.un.res_x >= 9.5367431640625e-07f && L.un.res_x <= 1.099511627776e12f &&
           L.un.res_y >= 9.5367431640625e-07f && L.un.res_y <= 1.099511627776e12f;
}

bool raytrace_variant_fuses(int variant)
{
#ifdef MI3PT_EXPERIMENTS
    return variant <= 3;
#else
    return variant <= 2;
#endif
}

// Waves per SIMD of the build a route runs.  The compressed-wide walk has two lean builds per instantiation: FIVE waves (96 registers, a
// 24-entry LDS stack) and SIX (80 registers with a handful spilled around the walk loop; 19 entries -- or 25 with the parked path state in
// memory, for very large trees).  Six waves overlap more of the per-step round trips: +2 .. +5 % on launches that run for tens of
// milliseconds.  But a sixth more paths are in flight when the job queue runs empty, and that drain is paid once per launch: a rank of an
// 8-way split (a 10 ms launch) is 2 .. 3 % SLOWER with six (profiles/r05_i_six_waves_by_launch_size.log).  So the choice goes by the size of
// the launch: jobs (tiles x frames) per resident wave.  L.six_waves forces it (MI3PT_OPT_SIX_WAVES).  Other lean builds: five; twins: four.
#ifndef PT_SIX_WAVES_MIN_JOBS
#define PT_SIX_WAVES_MIN_JOBS 1500000      // (round 6, re-swept on the cheaper node step: six waves win from ~1.3 M jobs on -- profiles/r06_i_six_waves_threshold.log; was 2.5 M)
#endif

// The kernel a launch runs for a requested variant.  kind: 0 = per-pixel kernel (variant 1 / 2), 1 = state-machine kernel
// (variant 4, 7, 9 .. 14; experiment builds: 5, 6, 8), 2 = k_raytrace_persistent (variant 3, experiment builds).
RtRoute raytrace_route(const RtLaunch &L, int variant)
{
    RtRoute r;
    r.variant = variant <= 1 ? 1 : 2;
    r.blocks = raytrace_grid_blocks(L.tile);
    if (variant < 3) return r;
#ifdef MI3PT_EXPERIMENTS
    if (variant == 3) { r.kind = 2; r.variant = 3; return r; }
#else
    if (variant == 3) variant = 4;                       // (release builds: the experiment variants resolve to their nearest walk)
    if (variant == 5 || variant == 6) variant = 4;
    if (variant == 8) variant = 7;
#endif
    if (!launch_packs(L)) return r;                      // per-pixel kernel 2, frame by frame
    bool lean = launch_is_lean(L);
    if (variant == 14 && !(L.scene.cw8 && L.scene.tripk8 && (L.scene.flags & 2u))) variant = 13;      // (the 8-wide walk never tests the root's own box)
    if (variant == 13 && !(L.scene.cwide && L.scene.tripk64)) variant = 10;
    if (L.walk_min == PT_DEEP_WALK_MIN && variant != 13 && variant != 14) lean = false;        // (the deep-walk threshold is instantiated for the compressed-wide walk only)
#ifndef MI3PT_EXPERIMENTS
    if (variant == 11 || variant == 12) variant = 10;       // (release builds: superseded by 13; the exact-packet walk with the exact slab test stands in -- same bits)
#endif
    if (variant >= 9 && variant <= 14 && lean && !launch_assumptions_hold(L)) variant = L.scene.leaf_cap >= 4 ? 7 : 4;
    if (variant >= 10 && variant <= 14 && !lean) variant = 10;      // the diagnostic twin of the wide walks runs the exact slab test: same bits
#ifndef MI3PT_EXPERIMENTS
    if (variant < 9 && !lean) {
        // release builds carry diagnostic twins for the culling walks only: the lean build runs (options and the diagnostic buffer
        // are ignored) -- or, without a service block, the per-pixel kernel
        if (!L.service) return r;
        lean = true;
    }
#endif
    r.kind = 1;
    r.variant = variant;
    r.lean = lean;

    // the instantiation: k_raytrace_sm's template arguments (one row of PT_SM_BUILDS, pt_kernels.h)
    SmBuild &b = r.build;
    int walk = variant;
#ifdef MI3PT_EXPERIMENTS
    if (lean && (walk == 5 || walk == 6 || walk == 8)) walk = 4;      // (these variants differ from 4 in their diagnostic twin only)
    b.lite = lean && L.wave_times && L.diag_lite && walk >= 10;       // the lean build + lane counts
    b.toplds = !lean && (walk == 6 || walk == 8);
#endif
    b.defer = walk >= 7; b.cull = walk >= 9; b.wide = walk >= 10; b.filt = walk >= 11;
    b.cw = walk >= 13; b.w8 = walk == 14;          // compressed wide packets; eight-wide compressed packets
    b.diag = !lean;
    b.wmin = PT_DEFAULT_WALK_MIN;
    b.waves = SM_TUNED_WAVES_PER_SIMD;
    b.ymax = walk == 12;
    if (b.cw) {
        b.ymax = (L.scene.flags & 4u) != 0u;       // (SceneRefs::flags bit 2: the one-axis culling condition suits this scene)
        if (!b.lite) {                             // (the lane-count builds: walk_min 32, five waves)
            if (walk == 13) b.toplds = PT_TOP_CW;
            if (L.walk_min == PT_DEEP_WALK_MIN) b.wmin = PT_DEEP_WALK_MIN;
            const long long jobs = (long long)raytrace_job_tiles(L) * (L.nframes > 0 ? L.nframes : 1);
            // (a job of a very large tree -- the walk_min-44 builds -- is an order of magnitude longer)
            const bool six = L.six_waves >= 0 ? L.six_waves != 0 : jobs >= (b.wmin == PT_DEEP_WALK_MIN ? PT_SIX_WAVES_MIN_JOBS / 10 : PT_SIX_WAVES_MIN_JOBS);
            if (six) b.waves = SM_SIX_WAVES_PER_SIMD;
        }
    }
    r.has_kernel = false;
#define PT_SM_ROW(...) r.has_kernel |= b == SmBuild{ __VA_ARGS__ };
    PT_SM_BUILDS(PT_SM_ROW)
#undef PT_SM_ROW

    // what the build is compiled for, as reported (a diagnostic twin: four waves, the launch's own walk_min)
    r.waves = b.diag ? SM_OTHER_WAVES_PER_SIMD : b.waves;
    r.ymax = lean && b.ymax;
    r.walk_min = b.diag ? L.walk_min : b.wmin;
    r.setup = lean && r.blocks > 0;                  // (still the tiles of the frame: an empty tile launches nothing)
    r.blocks = raytrace_persistent_blocks(L.tile, L.nframes, L.waves_per_cu, L.num_cus, lean, r.waves, L.ntiles_active);
    return r;
}

}  // namespace pt

extern "C" int mi3pt_host_route(const int64_t *in, size_t rows, int64_t *out)
{
    if ((!in || !out) && rows) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_host_route: bad argument");
    static char bound;                      // what a "present" pointer points to: routing never dereferences one
    for (size_t k = 0; k < rows; k++, in += MI3PT_HOST_ROUTE_INPUTS, out += MI3PT_HOST_ROUTE_OUTPUTS) {
        pt::RtLaunch L;
        std::memset(&L, 0, sizeof L);
        auto present = [&](int i) { return in[i] ? static_cast<void *>(&bound) : nullptr; };
        auto f32 = [&](int i) { const uint32_t u = (uint32_t)in[i]; float f; std::memcpy(&f, &u, 4); return f; };
        L.tile.tex_w = (int32_t)in[1]; L.tile.local_rows = (int32_t)in[2];
        L.nframes = (int32_t)in[3]; L.num_cus = (int32_t)in[4]; L.waves_per_cu = (int32_t)in[5]; L.ntiles_active = (int32_t)in[6]; L.six_waves = (int32_t)in[7];
        L.walk_min = (int32_t)in[8]; L.leaf_min = (int32_t)in[9]; L.shade_split = (int32_t)in[10]; L.tail_policy = (int32_t)in[11];
        L.job_chunk = (int32_t)in[12]; L.tri_pair = (int32_t)in[13]; L.diag_lite = (int32_t)in[17];
        L.wave_times = static_cast<uint64_t *>(present(14)); L.tile_cost = static_cast<uint32_t *>(present(15)); L.service = static_cast<pt::RtService *>(present(16));
        L.un.max_bounces = (int32_t)in[18]; L.un.samples_per_frame = (int32_t)in[19]; L.un.res_x = f32(20); L.un.res_y = f32(21);
        L.scene.nnodes = (uint32_t)in[22]; L.scene.flags = (uint32_t)in[23]; L.scene.root_ref = (uint32_t)in[24]; L.scene.leaf_cap = (int32_t)in[25];
        L.scene.cwide = L.scene.tripk64 = static_cast<const float4 *>(present(26));
        L.scene.cw8 = L.scene.tripk8 = static_cast<const float4 *>(present(27));
        const pt::RtRoute r = pt::raytrace_route(L, (int)in[0]);
        const pt::SmBuild &b = r.build;
        const int64_t o[MI3PT_HOST_ROUTE_OUTPUTS] = { r.kind, r.variant, r.lean, r.blocks, r.waves, r.ymax, r.walk_min, b.defer, b.cull, b.wide, b.filt, b.ymax,
                                                      b.diag, b.toplds, b.lite, b.cw, b.wmin, b.waves, b.w8, r.has_kernel, r.setup };
        std::memcpy(out, o, sizeof o);
    }
    return MI3PT_OK;
}
