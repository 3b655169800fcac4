// pt_ctx_group.hip -- device groups behind the C ABI: one handle, one member context per device.  What other units call: pt_ctx_calls.h.
#include "../../include/mi3pt.h"
#include "pt_ctx_calls.h"

#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include <vector>

// =================================================================================================
// Device groups: Renderer.create() over the GPUs of one node (the reference's seam is one adapter and
// one device, renderer.ts:491-533, and one render() per frame, :366-395).
//
// A group handle behaves like a context: the same entry points, the same frame semantics, the same bits.  Behind it
// stand one member context per listed device -- member i renders tile i of n (8-row blocks dealt round robin:
// mi3pt_set_tile), the scene is replicated by every upload call, NOTHING is exchanged per frame -- and one
// presenting context on the first device that holds the whole image.  The one exchange of a job is the GATHER: when
// the accumulation image (or the canvas) is read, every member's HDR accumulation rows are copied into the presenting
// context's image, de-interleaved on the way: one strided device-to-device copy per member (hipMemcpy2DAsync: peer
// DMA over xGMI when the devices can reach each other, staged by the runtime otherwise), no host buffer, no
// torch, no collective library -- a gather to one root is n - 1 point-to-point transfers on n - 1 distinct links.  The
// fullscreen pass (the de-noise looks 6 rows up and down, so it cannot run per tile) runs on the gathered image; a
// group therefore always presents lazily -- a FULLSCREEN submit is remembered and performed when the canvas is read
// (MI3PT_PRESENT_LATEST; drawing the canvas from every frame would put a gather into every frame).
// A group may list one device several times (tests: two members on the one GPU of the box).
// =================================================================================================

mi3pt_ctx *group_member0(mi3pt_ctx *g) { return g->group->members[0]; }
int group_unsupported(const char *what) { return pt_set_error(MI3PT_ERR_STATE, what); }

extern "C" int mi3pt_create_group(const int *devices, int ndevices, int block_rows, mi3pt_ctx **out_ctx)
{
    if (!devices || !out_ctx || ndevices < 1 || ndevices > 64) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_create_group: 1..64 devices");
    if (block_rows < 1 || block_rows > 4096) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_create_group: block_rows must be in [1, 4096]");
    *out_ctx = nullptr;
    mi3pt_ctx *g = new (std::nothrow) mi3pt_ctx();
    GroupState *gs = new (std::nothrow) GroupState();
    if (!g || !gs) { delete g; delete gs; return pt_set_error(MI3PT_ERR_HIP, "out of host memory"); }
    g->group = gs;
    g->device = devices[0];
    gs->block_rows = block_rows;
    int rc = MI3PT_OK;
    for (int i = 0; i < ndevices && rc == MI3PT_OK; i++) {
        mi3pt_ctx *m = nullptr;
        rc = mi3pt_create(devices[i], &m);
        if (rc == MI3PT_OK) {
            gs->members.push_back(m);
            rc = mi3pt_set_tile(m, i, ndevices, block_rows);
        }
    }
    if (rc == MI3PT_OK) rc = mi3pt_create(devices[0], &gs->present);
    if (rc == MI3PT_OK) rc = mi3pt_set_present_mode(gs->present, MI3PT_PRESENT_EXACT);
    if (rc == MI3PT_OK) {
        // Let the first device's copy engines reach the others' memory -- and RECORD whether they can (round-3 advice: the return
        // codes were dropped, so the gather could not tell a legal device-to-device rect copy from one that fails asynchronously).
        gs->peer_direct.assign((size_t)ndevices, 0);
        const bool on0 = hipSetDevice(devices[0]) == hipSuccess;
        for (int i = 0; i < ndevices; i++) {
            if (devices[i] == devices[0]) { gs->peer_direct[(size_t)i] = 1; continue; }
            int can = 0;
            if (!on0 || hipDeviceCanAccessPeer(&can, devices[0], devices[i]) != hipSuccess || !can) { (void)hipGetLastError(); continue; }
            const hipError_t e = hipDeviceEnablePeerAccess(devices[i], 0);
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) gs->peer_direct[(size_t)i] = 1;
            (void)hipGetLastError();
        }
        *out_ctx = g;
        return MI3PT_OK;
    }
    const std::string msg = pt_last_error();
    group_destroy(g);
    return pt_set_error(rc, msg);
}

extern "C" int mi3pt_group_size(mi3pt_ctx *ctx, int *members)
{
    if (!ctx || !members) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    *members = ctx->group ? (int)ctx->group->members.size() : 1;
    return MI3PT_OK;
}

extern "C" int mi3pt_group_member(mi3pt_ctx *ctx, int index, mi3pt_ctx **member)
{
    if (!ctx || !member) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (!ctx->group) { if (index != 0) return pt_set_error(MI3PT_ERR_INVALID, "not a group: the only member is index 0"); *member = ctx; return MI3PT_OK; }
    if (index == -1) { *member = ctx->group->present; return MI3PT_OK; }
    if (index < 0 || (size_t)index >= ctx->group->members.size()) return pt_set_error(MI3PT_ERR_INVALID, "member index out of range");
    *member = ctx->group->members[(size_t)index];
    return MI3PT_OK;
}

int group_destroy(mi3pt_ctx *g)
{
    GroupState *gs = g->group;
    int rc = MI3PT_OK;
    for (mi3pt_ctx *m : gs->members)
        if (m) { const int r = mi3pt_destroy(m); if (r && !rc) rc = r; }
    if (gs->present) { const int r = mi3pt_destroy(gs->present); if (r && !rc) rc = r; }
    delete gs;
    g->group = nullptr;
    delete g;
    return rc;
}

int group_resize(mi3pt_ctx *g, int width, int height)
{
    GroupState *gs = g->group;
    gs->width = gs->height = 0;
    for (int k = 0; k < MI3PT_AOV_COUNT; k++) gs->aov_rendered[k] = gs->aov_gathered[k] = false;
    gs->present->moments = false;      // (its resize frees the gathered moments image and must not allocate one of its own: group_gather_moments)
    if (int rc = group_each(g, true, [&](mi3pt_ctx *m) { return mi3pt_resize(m, width, height); })) return rc;
    gs->width = width;
    gs->height = height;
    g->width = width; g->height = height;
    gs->gathered = true;          // every image is zero
    gs->want_present = false;
    for (int k = 0; k < MI3PT_AOV_COUNT; k++) gs->aov_rendered[k] = gs->aov_gathered[k] = false;
    return MI3PT_OK;
}

int group_reset(mi3pt_ctx *g)
{
    GroupState *gs = g->group;
    if (int rc = group_each(g, true, [&](mi3pt_ctx *m) { return mi3pt_reset(m); })) return rc;
    gs->gathered = true;
    gs->want_present = false;
    return MI3PT_OK;
}

int group_set_uniforms(mi3pt_ctx *g, int pass, const void *bytes, size_t nbytes)
{
    if (pass == MI3PT_PASS_FULLSCREEN) return mi3pt_set_uniforms(g->group->present, pass, bytes, nbytes);
    return group_each(g, false, [&](mi3pt_ctx *m) { return mi3pt_set_uniforms(m, pass, bytes, nbytes); });
}

// image row of local row `ly` of member i of n (mi3pt_set_tile's deal: rounds go back and forth)
static size_t group_global_row(int ly, int i, int n, int br)
{
    const int b = ly / br;
    return ((size_t)b * (size_t)n + (size_t)((b & 1) ? n - 1 - i : i)) * (size_t)br + (size_t)(ly % br);
}

// One scene buffer of `src` replicated into `dst` (another member, maybe another device): device to device, on dst's stream.
static int clone_buffer(mi3pt_ctx *dst, DevBuf<void> &dbuf, const mi3pt_ctx *src, const DevBuf<void> &sbuf)
{
    dbuf.reset();
    if (!sbuf) return MI3PT_OK;
    HIP_TRY(dbuf.alloc(sbuf.bytes));
    if (sbuf.bytes) HIP_TRY(hipMemcpyPeerAsync(dbuf, dst->device, sbuf, src->device, sbuf.bytes, dst->stream));
    return MI3PT_OK;
}

// Everything mi3pt_upload_* and the scene analyses leave in a context, copied from `src` (a group's member 0) to `dst`.
static int clone_scene(mi3pt_ctx *dst, const mi3pt_ctx *src)
{
    if (int rc = require_idle(dst)) return rc;
    HIP_TRY(ctx_stream_sync(dst, dst->stream));
    for (int k = 0; k < 2; k++) HIP_TRY(ctx_stream_sync(dst, dst->rt_stream[k]));
    const auto from = SceneBuffers::all(*src);
    const auto to = SceneBuffers::all(*dst);
    for (size_t k = 0; k < from.size(); k++)
        if (int rc = clone_buffer(dst, *to[k], src, *from[k])) return rc;
    const size_t env_bytes = (size_t)MI3PT_ENV_WIDTH * MI3PT_ENV_HEIGHT * 16;
    HIP_TRY(hipMemcpyPeerAsync(dst->d_env, dst->device, src->d_env, src->device, env_bytes, dst->stream));
    HIP_TRY(hipMemcpyPeerAsync(dst->d_cdf, dst->device, src->d_cdf, src->device, env_bytes, dst->stream));
    HIP_TRY(ctx_stream_sync(dst, dst->stream));
    dst->scene_facts() = src->scene_facts();
    // what does not come from `src`: the copy's own caches are of another scene, its streams have new work to order, its scene has a new version.
    // (Nor do the options -- cull_enabled, wide_enabled, collapse, packet_order: set on every member -- the kept geometry and host_analyses.)
    dst->cost_state = 0;
    dst->sky_host_valid = false;
    dst->main_dirty = true;
    dst->scene_epoch++;
    return MI3PT_OK;
}

// Before anything traces rays: member 0 compiles the scene (the host-side analyses run ONCE per scene change, whatever the
// number of members -- round-3 verdict: config 5 on eight GPUs was eight uploads, eight 1.4 GB read-backs and eight analyses),
// the other members get device copies.
static int group_sync_scene(mi3pt_ctx *g)
{
    GroupState *gs = g->group;
    mi3pt_ctx *m0 = gs->members[0];
    if (int rc = require_ctx(m0)) return rc;
    if (int rc = check_scene(m0)) return rc;
    if (int rc = prepare_layout(m0)) return rc;
    if (int rc = prepare_cull(m0)) return rc;
    if (m0->scene_epoch == gs->cloned_epoch) return MI3PT_OK;
    for (size_t i = 1; i < gs->members.size(); i++)
        if (int rc = clone_scene(gs->members[i], m0)) return rc;
    gs->cloned_epoch = m0->scene_epoch;
    return MI3PT_OK;
}

int group_submit_frames(mi3pt_ctx *g, unsigned pass_mask, uint32_t count)
{
    GroupState *gs = g->group;
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, "submit before resize");
    const unsigned sample = pass_mask & (MI3PT_SUBMIT_RAYTRACE | MI3PT_SUBMIT_ACCUMULATE);
    if (pass_mask & MI3PT_SUBMIT_RAYTRACE)
        if (int rc = group_sync_scene(g)) return rc;
    if (sample) {
        if (int rc = group_each(g, false, [&](mi3pt_ctx *m) { return count == 1 ? mi3pt_submit(m, sample) : mi3pt_submit_frames(m, sample, count); })) return rc;
        if (sample & MI3PT_SUBMIT_ACCUMULATE) gs->gathered = false;
    }
    if (pass_mask & MI3PT_SUBMIT_FULLSCREEN) gs->want_present = true;      // performed when the canvas is read (see the header of this section)
    return MI3PT_OK;
}

int group_flush(mi3pt_ctx *g) { return group_each(g, false, [&](mi3pt_ctx *m) { return mi3pt_flush(m); }); }

int group_sync(mi3pt_ctx *g)
{
    // launch everything that is queued on every member first, THEN wait: the members run side by side
    if (int rc = group_flush(g)) return rc;
    return group_each(g, true, [&](mi3pt_ctx *m) { return mi3pt_sync(m); });
}

// The one exchange: members' accumulation rows -> the presenting context's whole image.
// Member i's rows, de-interleaved into the whole image.  direct: one strided device-to-device copy (the de-interleave is the copy's
// geometry: source pitch = one block, destination pitch = n blocks) on the presenting context's stream -- peer DMA over xGMI.
// Otherwise: staged through pinned host memory (a device-to-host copy on the member's device, then the same strided copy from
// the host buffer).
// (member_plane: the member's rows of the image gathered; whole_plane: that image on the presenting context)
static int gather_member(GroupState *gs, int i, bool direct, const float4 *member_plane, float4 *whole_plane)
{
    mi3pt_ctx *p = gs->present;
    const mi3pt_ctx *m = gs->members[(size_t)i];
    const int n = (int)gs->members.size(), br = gs->block_rows, W = gs->width, H = gs->height;
    const size_t row_bytes = (size_t)W * 16, block_bytes = row_bytes * (size_t)br;
    uint8_t *dst = reinterpret_cast<uint8_t *>(whole_plane);
    const uint8_t *src = reinterpret_cast<const uint8_t *>(member_plane);
    const int rows = m->local_rows;
    if (rows == 0) return MI3PT_OK;
    const int full = rows / br, tail = rows - full * br;      // whole blocks, rows of a last partial block (the image's bottom edge)
    const size_t grow = group_global_row(full * br, i, n, br);      // global row of the partial block
    if (tail > 0 && (int)grow + tail > H) return pt_set_error(MI3PT_ERR_STATE, "gather: tile geometry mismatch");
    hipMemcpyKind kind = hipMemcpyDeviceToDevice;
    if (!direct) {
        const size_t need = (size_t)rows * row_bytes;
        if (gs->stage.bytes < need) HIP_TRY(gs->stage.alloc(need));
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(hipMemcpy(gs->stage, src, need, hipMemcpyDeviceToHost));      // (synchronous: the one staging buffer is reused member by member)
        HIP_TRY(hipSetDevice(p->device));
        src = gs->stage.as<const uint8_t>();
        kind = hipMemcpyHostToDevice;
    }
    // The deal goes back and forth: the member's even local blocks sit at image block (2 k n + i), its odd ones at
    // ((2 k + 1) n + n - 1 - i) -- two strided sets, each ONE rect copy (source pitch = two blocks, destination pitch = 2 n blocks)
    const int n_even = (full + 1) / 2, n_odd = full / 2;
    if (n_even > 0)
        HIP_TRY(hipMemcpy2DAsync(dst + (size_t)i * block_bytes, 2 * (size_t)n * block_bytes, src, 2 * block_bytes, block_bytes, (size_t)n_even, kind, p->stream));
    if (n_odd > 0)
        HIP_TRY(hipMemcpy2DAsync(dst + (size_t)(n + n - 1 - i) * block_bytes, 2 * (size_t)n * block_bytes, src + block_bytes, 2 * block_bytes, block_bytes, (size_t)n_odd, kind, p->stream));
    if (tail > 0)
        HIP_TRY(hipMemcpyAsync(dst + grow * row_bytes, src + (size_t)full * block_bytes, (size_t)tail * row_bytes, kind, p->stream));
    if (!direct) HIP_TRY(ctx_stream_sync(p, p->stream));       // the staging buffer is free again
    return MI3PT_OK;
}

// the copies of a gather (the members' work has been waited for); plane(ctx): the image gathered, as that context holds it
template <class Plane> static int gather_copies(GroupState *gs, Plane plane)
{
    mi3pt_ctx *p = gs->present;
    const int n = (int)gs->members.size();
    for (int attempt = 0; attempt < 2; attempt++) {
        // direct copies first, all in flight together on the presenting stream (n - 1 transfers on n - 1 links into one root) ...
        for (int i = 0; i < n; i++) {
            if (!gs->peer_direct[(size_t)i]) continue;
            if (gather_member(gs, i, true, plane(gs->members[(size_t)i]), plane(p)) != MI3PT_OK) { (void)hipGetLastError(); gs->peer_direct[(size_t)i] = 0; }
        }
        if (ctx_stream_sync(p, p->stream) == hipSuccess) break;
        // ... a rect copy between two devices can also fail asynchronously (round-3 advice): nothing this pass wrote is trusted;
        // every member on another device goes through the host from now on, and the gather is done again, once
        (void)hipGetLastError();
        bool any = false;
        for (int i = 0; i < n; i++)
            if (gs->members[(size_t)i]->device != p->device && gs->peer_direct[(size_t)i]) { gs->peer_direct[(size_t)i] = 0; any = true; }
        if (!any || attempt == 1) return pt_set_error(MI3PT_ERR_HIP, "group gather: the copies into the presenting context failed");
    }
    // ... then whatever cannot be addressed directly, staged through pinned host memory
    for (int i = 0; i < n; i++)
        if (!gs->peer_direct[(size_t)i])
            if (int rc = gather_member(gs, i, false, plane(gs->members[(size_t)i]), plane(p))) return rc;
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(ctx_stream_sync(p, p->stream));
    return MI3PT_OK;
}

// A whole image the presenting context allocates when it is first gathered (a feature image, the moments image) and frees with its
// textures.  wait_for_members: the members' work that writes the image, then the presenting context ready for the copies.
template <class Plane, class Wait> static int gather_lazy_image(GroupState *gs, Plane plane, Wait wait_for_members)
{
    if (int rc = wait_for_members()) return rc;
    mi3pt_ctx *p = gs->present;
    if (!plane(p)) HIP_TRY(plane(p).alloc(plane_bytes(p)));
    return gather_copies(gs, plane);
}

static int group_gather(mi3pt_ctx *g)
{
    GroupState *gs = g->group;
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, "read before resize");
    if (gs->gathered) return MI3PT_OK;
    if (int rc = group_sync(g)) return rc;
    mi3pt_ctx *p = gs->present;
    if (int rc = require_idle(p)) return rc;
    if (int rc = gather_copies(gs, [](mi3pt_ctx *c) -> float4 *& { return c->d_accum; })) return rc;
    p->output_is_accum = true;      // like the copy-back of accumulate.ts:171-175
    p->main_dirty = true;
    p->accum_version++;
    gs->gathered = true;
    return MI3PT_OK;
}

// ---- first-hit feature images of a group: rendered by every member for its rows, gathered when read ----
int group_render_aovs(mi3pt_ctx *g, unsigned aov_mask)
{
    GroupState *gs = g->group;
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_render_aovs before resize");
    if (aov_mask == 0 || (aov_mask >> MI3PT_AOV_COUNT)) return pt_set_error(MI3PT_ERR_INVALID, "aov_mask must be a non-empty OR of (1u << mi3pt_aov)");
    if (int rc = group_sync_scene(g)) return rc;
    if (int rc = group_each(g, false, [&](mi3pt_ctx *m) { return mi3pt_render_aovs(m, aov_mask); })) return rc;
    for (int k = 0; k < MI3PT_AOV_COUNT; k++)
        if ((aov_mask >> k) & 1u) { gs->aov_rendered[k] = true; gs->aov_gathered[k] = false; }
    return MI3PT_OK;
}

static int group_gather_aov(mi3pt_ctx *g, int which, const char *what)
{
    GroupState *gs = g->group;
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + " before resize");
    if (which < 0 || which >= MI3PT_AOV_COUNT) return pt_set_error(MI3PT_ERR_INVALID, "unknown feature image");
    if (!gs->aov_rendered[which])
        return pt_set_error(MI3PT_ERR_STATE, std::string(what) + ": this image has not been rendered since the last resize (mi3pt_render_aovs)");
    if (gs->aov_gathered[which]) return MI3PT_OK;
    // the members' passes (their own streams; their frame queues stay as they are), then the copies
    auto members_streams = [&]() -> int {
        for (mi3pt_ctx *m : gs->members) {
            if (int rc = require_ctx(m)) return rc;
            HIP_TRY(ctx_stream_sync(m, m->stream));
        }
        return require_ctx(gs->present);
    };
    if (int rc = gather_lazy_image(gs, [which](mi3pt_ctx *c) -> DevBuf<float4> & { return c->d_aov[which]; }, members_streams)) return rc;
    gs->present->aov_valid[which] = true;
    gs->aov_gathered[which] = true;
    return MI3PT_OK;
}

int group_read_aov(mi3pt_ctx *g, int which, void *dst, size_t nbytes)
{
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (g->group->width && which >= 0 && which < MI3PT_AOV_COUNT && g->group->aov_rendered[which] &&
        nbytes != (size_t)g->group->width * g->group->height * 16)
        return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the image (a group reads whole images: height x width x 16 bytes)");
    if (int rc = group_gather_aov(g, which, "mi3pt_read_aov")) return rc;
    return mi3pt_read_aov(g->group->present, which, dst, nbytes);
}

int group_aov_ptr(mi3pt_ctx *g, int which, void **dev_ptr, size_t *nbytes)
{
    if (!dev_ptr) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = group_gather_aov(g, which, "mi3pt_aov_device_ptr")) return rc;
    return mi3pt_aov_device_ptr(g->group->present, which, dev_ptr, nbytes);
}

// ---- the moments image of a group: kept by every member for its rows; the presenting context's whole image is allocated by the first read
// (like a feature image: group_gather_aov), freed by its resize (free_textures) and by mi3pt_set_moments(0), and gathered whenever it is read.
// While it holds the gathered copy the presenting context counts as having moments enabled, so that its own mi3pt_read_moments and
// mi3pt_moments_device_ptr serve the image; it never runs an accumulate pass, so it never keeps moments of its own ----
int group_set_moments(mi3pt_ctx *g, int enabled)
{
    if (int rc = group_each(g, false, [&](mi3pt_ctx *m) { return mi3pt_set_moments(m, enabled); })) return rc;
    mi3pt_ctx *p = g->group->present;
    if (!enabled && p->d_moments) {
        if (int rc = require_ctx(p)) return rc;
        HIP_TRY(ctx_stream_sync(p, p->stream));
        p->d_moments.reset();
    }
    if (!enabled) p->moments = false;
    return MI3PT_OK;
}

static int group_gather_moments(mi3pt_ctx *g, const char *what)
{
    GroupState *gs = g->group;
    if (!gs->members[0]->moments) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + ": the moments image is not enabled (mi3pt_set_moments)");
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + " before resize");
    auto everything = [&]() -> int {
        if (int rc = group_sync(g)) return rc;
        return require_idle(gs->present);
    };
    if (int rc = gather_lazy_image(gs, [](mi3pt_ctx *c) -> DevBuf<float4> & { return c->d_moments; }, everything)) return rc;
    gs->present->moments = true;
    return MI3PT_OK;
}

int group_read_moments(mi3pt_ctx *g, void *dst, size_t nbytes)
{
    GroupState *gs = g->group;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    const size_t need = (size_t)gs->width * gs->height * 16;
    if (gs->width && gs->members[0]->moments && nbytes != need)
        return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the image (a group reads whole images: height x width x 16 bytes)");
    if (int rc = group_gather_moments(g, "mi3pt_read_moments")) return rc;
    return mi3pt_read_moments(gs->present, dst, nbytes);
}

int group_moments_ptr(mi3pt_ctx *g, void **dev_ptr, size_t *nbytes)
{
    if (!dev_ptr) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (int rc = group_gather_moments(g, "mi3pt_moments_device_ptr")) return rc;
    return mi3pt_moments_device_ptr(g->group->present, dev_ptr, nbytes);
}

// ---- the error estimate: mi3pt_estimate_convergence goes to every member (PT_GROUP_ALL); the summaries combine on the host -- counts add,
// max of max, min of min -- and so do the tile maps, which are kilobytes: no peer copies ----
int group_read_convergence(mi3pt_ctx *g, mi3pt_convergence *out)
{
    if (!out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    mi3pt_convergence all = {};
    bool first = true;
    for (mi3pt_ctx *m : g->group->members) {
        mi3pt_convergence c;
        if (int rc = mi3pt_read_convergence(m, &c)) return rc;
        all.tiles += c.tiles; all.tiles_above += c.tiles_above; all.tiles_young += c.tiles_young; all.tiles_nonfinite += c.tiles_nonfinite;
        all.texels += c.texels;
        all.worst_tile = fmaxf(all.worst_tile, c.worst_tile);
        all.worst_texel = fmaxf(all.worst_texel, c.worst_texel);
        if (c.tiles) {
            all.n_min = first ? c.n_min : fminf(all.n_min, c.n_min);
            first = false;
        }
        all.threshold = c.threshold;
    }
    *out = all;
    return MI3PT_OK;
}

int group_read_convergence_tiles(mi3pt_ctx *g, float *dst, size_t nfloats)
{
    GroupState *gs = g->group;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_read_convergence_tiles before resize");
    if (gs->block_rows % 8)
        return pt_set_error(MI3PT_ERR_STATE, "mi3pt_read_convergence_tiles: the members' tiles only form the image's tile map when the group's block_rows is a multiple of 8 (read each member's map: mi3pt_group_member)");
    for (mi3pt_ctx *m : gs->members)
        if (!m->conv_valid) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_read_convergence_tiles: nothing has been estimated since the last resize (mi3pt_estimate_convergence)");
    const size_t tiles_x = ((size_t)gs->width + 7) / 8, tiles_y = ((size_t)gs->height + 7) / 8;
    if (nfloats != tiles_x * tiles_y * 4)
        return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the tile map (a group reads the whole map: ceil(height / 8) x ceil(width / 8) x 4 floats)");
    const int n = (int)gs->members.size();
    std::vector<float> part;
    for (int i = 0; i < n; i++) {
        mi3pt_ctx *m = gs->members[(size_t)i];
        const size_t rows = conv_tiles_y(m);
        part.resize(rows * tiles_x * 4);
        if (rows == 0) continue;
        if (int rc = mi3pt_read_convergence_tiles(m, part.data(), part.size())) return rc;
        for (size_t t = 0; t < rows; t++) {
            const size_t gt = (size_t)mi3pt_tile_global_row((int)t, i, n, gs->block_rows / 8);
            if (gt >= tiles_y) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_read_convergence_tiles: a member's tile row lies outside the image");
            std::memcpy(dst + gt * tiles_x * 4, part.data() + t * tiles_x * 4, tiles_x * 16);
        }
    }
    return MI3PT_OK;
}

// ---- the sample mask: the whole image's map in and out, scattered to / assembled from the members' maps on the host by the row rule of
// group_read_convergence_tiles; the freeze rule runs on the WHOLE map, so its guard ring is the image's ----
static int group_mask_shape(mi3pt_ctx *g, const char *what, size_t *tiles_x, size_t *tiles_y)
{
    GroupState *gs = g->group;
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, std::string(what) + " before resize");
    if (gs->block_rows % 8)
        return pt_set_error(MI3PT_ERR_STATE, std::string(what) + ": the members' tiles only form the image's tile map when the group's block_rows is a multiple of 8 (use each member's mask: mi3pt_group_member)");
    *tiles_x = ((size_t)gs->width + 7) / 8;
    *tiles_y = ((size_t)gs->height + 7) / 8;
    return MI3PT_OK;
}

int group_set_sample_mask(mi3pt_ctx *g, const uint8_t *tiles, size_t ntiles)
{
    GroupState *gs = g->group;
    size_t tiles_x = 0, tiles_y = 0;
    if (int rc = group_mask_shape(g, "mi3pt_set_sample_mask", &tiles_x, &tiles_y)) return rc;
    if (!tiles && ntiles == 0) return group_each(g, false, [&](mi3pt_ctx *m) { return mi3pt_set_sample_mask(m, nullptr, 0); });
    if (!tiles) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (ntiles != tiles_x * tiles_y)
        return pt_set_error(MI3PT_ERR_INVALID, "the mask's size does not match the tile map (a group takes the whole map: ceil(height / 8) x ceil(width / 8) bytes)");
    const int n = (int)gs->members.size();
    std::vector<uint8_t> part;
    for (int i = 0; i < n; i++) {
        mi3pt_ctx *m = gs->members[(size_t)i];
        const size_t rows = conv_tiles_y(m);
        part.assign(rows * tiles_x, 0);
        for (size_t t = 0; t < rows; t++) {
            const size_t gt = (size_t)mi3pt_tile_global_row((int)t, i, n, gs->block_rows / 8);
            if (gt >= tiles_y) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_set_sample_mask: a member's tile row lies outside the image");
            std::memcpy(part.data() + t * tiles_x, tiles + gt * tiles_x, tiles_x);
        }
        if (rows == 0) continue;
        if (int rc = mi3pt_set_sample_mask(m, part.data(), part.size())) return rc;
    }
    return MI3PT_OK;
}

int group_read_sample_mask(mi3pt_ctx *g, uint8_t *dst, size_t ntiles, uint32_t *sampled_out)
{
    GroupState *gs = g->group;
    size_t tiles_x = 0, tiles_y = 0;
    if (int rc = group_mask_shape(g, "mi3pt_read_sample_mask", &tiles_x, &tiles_y)) return rc;
    if (ntiles != tiles_x * tiles_y)
        return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the tile map (a group reads the whole map: ceil(height / 8) x ceil(width / 8) bytes)");
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    const int n = (int)gs->members.size();
    std::vector<uint8_t> part;
    uint32_t sampled = 0;
    for (int i = 0; i < n; i++) {
        mi3pt_ctx *m = gs->members[(size_t)i];
        const size_t rows = conv_tiles_y(m);
        if (rows == 0) continue;
        part.resize(rows * tiles_x);
        uint32_t mine = 0;
        if (int rc = mi3pt_read_sample_mask(m, part.data(), part.size(), &mine)) return rc;
        sampled += mine;
        for (size_t t = 0; t < rows; t++) {
            const size_t gt = (size_t)mi3pt_tile_global_row((int)t, i, n, gs->block_rows / 8);
            if (gt >= tiles_y) return pt_set_error(MI3PT_ERR_STATE, "mi3pt_read_sample_mask: a member's tile row lies outside the image");
            std::memcpy(dst + gt * tiles_x, part.data() + t * tiles_x, tiles_x);
        }
    }
    if (sampled_out) *sampled_out = sampled;
    return MI3PT_OK;
}

int group_freeze_converged(mi3pt_ctx *g, int guard, uint32_t *sampled_out)
{
    GroupState *gs = g->group;
    if (guard != 0 && guard != 1) return pt_set_error(MI3PT_ERR_INVALID, "mi3pt_freeze_converged: guard must be 0 or 1");
    size_t tiles_x = 0, tiles_y = 0;
    if (int rc = group_mask_shape(g, "mi3pt_freeze_converged", &tiles_x, &tiles_y)) return rc;
    const size_t n = tiles_x * tiles_y;
    std::vector<float> records(n * 4);
    if (int rc = group_read_convergence_tiles(g, records.data(), records.size())) return rc;
    std::vector<uint8_t> mask(n);
    if (int rc = group_read_sample_mask(g, mask.data(), n, nullptr)) return rc;
    const mi3pt_ctx *m0 = gs->members[0];
    uint32_t sampled = 0;
    if (int rc = mi3pt_host_freeze_tiles(records.data(), (int)tiles_x, (int)tiles_y, m0->conv_threshold, m0->conv_min_frames, guard, mask.data(), &sampled)) return rc;
    if (int rc = group_set_sample_mask(g, mask.data(), n)) return rc;
    if (sampled_out) *sampled_out = sampled;
    return MI3PT_OK;
}

static int group_draw_canvas(mi3pt_ctx *g)
{
    GroupState *gs = g->group;
    if (int rc = group_gather(g)) return rc;
    if (gs->want_present) {
        if (int rc = mi3pt_submit(gs->present, MI3PT_SUBMIT_FULLSCREEN)) return rc;
        gs->want_present = false;
    }
    return MI3PT_OK;
}

int group_read_texture(mi3pt_ctx *g, int which, float *dst, size_t nfloats)
{
    GroupState *gs = g->group;
    if (!dst) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, "read before resize");
    const size_t need = (size_t)gs->width * gs->height * 4;
    if (nfloats != need) return pt_set_error(MI3PT_ERR_INVALID, "destination size does not match the texture (a group reads whole images)");
    if (which == MI3PT_TEX_ACCUMULATION) {
        if (int rc = group_gather(g)) return rc;
        return mi3pt_read_texture(gs->present, which, dst, nfloats);
    }
    if (which == MI3PT_TEX_CANVAS) {
        if (int rc = group_draw_canvas(g)) return rc;
        return mi3pt_read_texture(gs->present, which, dst, nfloats);
    }
    if (which != MI3PT_TEX_OUTPUT) return pt_set_error(MI3PT_ERR_INVALID, "unknown texture");
    // the last frame's radiance: not part of any exchange -- read member by member and de-interleaved on the host
    const int n = (int)gs->members.size(), br = gs->block_rows;
    const size_t row = (size_t)gs->width * 4;
    std::vector<float> part;
    for (int i = 0; i < n; i++) {
        mi3pt_ctx *m = gs->members[(size_t)i];
        part.resize((size_t)m->local_rows * row);
        if (int rc = mi3pt_read_texture(m, which, part.data(), part.size())) return rc;
        for (int ly = 0; ly < m->local_rows; ly++) {
            const size_t gy = group_global_row(ly, i, n, br);
            std::memcpy(dst + gy * row, part.data() + (size_t)ly * row, row * 4);
        }
    }
    return MI3PT_OK;
}

int group_write_texture(mi3pt_ctx *g, int which, const float *src, size_t nfloats)
{
    GroupState *gs = g->group;
    if (!src) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (gs->width == 0) return pt_set_error(MI3PT_ERR_STATE, "write before resize");
    if (nfloats != (size_t)gs->width * gs->height * 4) return pt_set_error(MI3PT_ERR_INVALID, "source size does not match the texture (a group writes whole images)");
    const int n = (int)gs->members.size(), br = gs->block_rows;
    const size_t row = (size_t)gs->width * 4;
    std::vector<float> part;
    for (int i = 0; i < n; i++) {
        mi3pt_ctx *m = gs->members[(size_t)i];
        part.resize((size_t)m->local_rows * row);
        for (int ly = 0; ly < m->local_rows; ly++) {
            const size_t gy = group_global_row(ly, i, n, br);
            std::memcpy(part.data() + (size_t)ly * row, src + gy * row, row * 4);
        }
        if (int rc = mi3pt_write_texture(m, which, part.data(), part.size())) return rc;
    }
    gs->gathered = false;
    return MI3PT_OK;
}

int group_read_canvas(mi3pt_ctx *g, uint8_t *dst, size_t nbytes)
{
    if (int rc = group_draw_canvas(g)) return rc;
    return mi3pt_read_canvas_rgba8(g->group->present, dst, nbytes);
}

int group_accumulation_ptr(mi3pt_ctx *g, void **dev_ptr, size_t *nbytes)
{
    if (int rc = group_gather(g)) return rc;
    return mi3pt_accumulation_device_ptr(g->group->present, dev_ptr, nbytes);
}

// per-pass GPU time: the passes of the members run side by side -> the slowest member's; the fullscreen pass: the presenting context's
int group_pass_time(mi3pt_ctx *g, int pass, float *us)
{
    if (!us) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    if (pass == MI3PT_PASS_FULLSCREEN) return mi3pt_pass_time_us(g->group->present, pass, us);
    float worst = 0.0f;
    for (mi3pt_ctx *m : g->group->members) {
        float t = 0.0f;
        if (int rc = mi3pt_pass_time_us(m, pass, &t)) return rc;
        if (t > worst) worst = t;
    }
    *us = worst;
    return MI3PT_OK;
}

int group_launch_stats(mi3pt_ctx *g, int reset, double *total_ms, uint64_t *launches, uint64_t *frames)
{
    double worst = 0.0;
    uint64_t l0 = 0, f0 = 0;
    bool first = true;
    for (mi3pt_ctx *m : g->group->members) {
        double t = 0.0;
        uint64_t l = 0, f = 0;
        if (int rc = mi3pt_raytrace_launch_stats(m, reset, &t, &l, &f)) return rc;
        if (t > worst) worst = t;
        if (first) { l0 = l; f0 = f; first = false; }
    }
    if (total_ms) *total_ms = worst;
    if (launches) *launches = l0;
    if (frames) *frames = f0;
    return MI3PT_OK;
}

int group_launch_span(mi3pt_ctx *g, double *span_ms)
{
    if (!span_ms) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    double worst = 0.0;
    for (mi3pt_ctx *m : g->group->members) {
        double t = 0.0;
        if (int rc = mi3pt_raytrace_launch_span(m, &t)) return rc;
        if (t > worst) worst = t;
    }
    *span_ms = worst;
    return MI3PT_OK;
}

// MI3PT_OPT_HOST_ANALYSES: the sum over the members (one scene compile per scene change, whatever the group's size);
// MI3PT_OPT_GATHER_STAGED: 1 = every member's rows reach the presenting context through pinned host memory (the path the gather falls
// back to when peer access is unavailable or a direct copy failed: forced here so that it can be tested on one GPU)
int group_get_option(mi3pt_ctx *g, int option, int *value)
{
    if (!value) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    GroupState *gs = g->group;
    if (option == MI3PT_OPT_HOST_ANALYSES) {
        uint64_t n = 0;
        for (mi3pt_ctx *m : gs->members) n += m->host_analyses;
        *value = (int)n;
        return MI3PT_OK;
    }
    if (option == MI3PT_OPT_GATHER_STAGED) {
        int direct = 0;
        for (char d : gs->peer_direct) direct += d ? 1 : 0;
        *value = direct == 0 ? 1 : 0;
        return MI3PT_OK;
    }
    return mi3pt_debug_get_option(gs->members[0], option, value);
}

int group_set_option(mi3pt_ctx *g, int option, int value)
{
    GroupState *gs = g->group;
    if (option == MI3PT_OPT_GATHER_STAGED) {
        for (size_t i = 0; i < gs->peer_direct.size(); i++)
            gs->peer_direct[i] = value ? 0 : (gs->members[i]->device == gs->present->device ? 1 : gs->peer_direct[i]);
        gs->gathered = false;
        for (bool &a : gs->aov_gathered) a = false;
        return MI3PT_OK;
    }
    return group_each(g, false, [&](mi3pt_ctx *m) { return mi3pt_debug_set_option(m, option, value); });
}

int group_counters(mi3pt_ctx *g, uint64_t *out)
{
    if (!out) return pt_set_error(MI3PT_ERR_INVALID, "null argument");
    for (int k = 0; k < MI3PT_CNT_COUNT; k++) out[k] = 0;
    for (mi3pt_ctx *m : g->group->members) {
        uint64_t c[MI3PT_CNT_COUNT];
        if (int rc = mi3pt_get_counters(m, c)) return rc;
        for (int k = 0; k < MI3PT_CNT_COUNT; k++) out[k] += c[k];
    }
    return MI3PT_OK;
}
