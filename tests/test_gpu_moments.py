"""The moments image (mi3pt_set_moments) on the GPU against tests/moments_reference.py::welford over the ORACLE's frames and means: every
comparison is bit for bit (ptcommon.same_bits).  The same four frames go through every path that forms a mean, and in every one of them
the accumulation image, the counters and mi3pt_debug_last_launch equal those of a run with moments off.  What keeps a case from passing
vacuously (texels with a spread) is asserted on the reference alone."""
import ctypes

import numpy as np
import pytest

import moments_reference as mr
import ptcommon as pc
import shading_cases as sh
from mi3pt_host import capi

pytestmark = pytest.mark.gpu
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
BASE_STEPS = tuple((f, f, 1) for f in range(1, 5))          # (raytrace frame, accumulate frame, enabled)
_cache = {}


@pytest.fixture(scope="module")
def ctx(built):
    """A context of this module's own: the session's shared one never opts into the moments image"""
    c = capi.Context(0)
    yield c
    c.close()


def _reference(orc, sc, env, w, h, steps, bounces=4, f16=False, tile=(0, 1, 8), res=None):
    key = (sc.name, w, h, tuple(steps), bounces, f16, tile, res)
    if key not in _cache:
        rw, rh = res if res is not None else (w, h)
        inside = None
        if res is not None:
            inside = (np.arange(w)[None, :] < rw) & (np.arange(h)[:, None] < rh)
        mean, m, _, _ = mr.oracle_steps(orc, pc.oracle_scene(orc, sc, env), steps, w, h,
                                        lambda f: pc.rt_uniforms(sc, w, h, frame=f, bounces=bounces, res=res).tobytes(),
                                        lambda f, e: pc.acc_uniforms(rw, rh, f, e).tobytes(), *tile, store_f16=f16, inside=inside)
        _cache[key] = (mean, m)
    return _cache[key]


def _device(ctx, sc, env, w, h, steps, moments, submit="frames", bounces=4, f16=False, tile=(0, 1, 8), res=None, pipelining=True,
            variant=0, batch=None, present_at=None):
    """One run.  submit: "frames" = one submit_frames for the whole run (steps must be consecutive), "each" = a submit per step,
    "separate" = RAYTRACE and ACCUMULATE as submits of their own.  present_at: the step that also presents (EXACT).  Returns
    (accumulation, moments or None, counters, last_launch)."""
    rw, rh = res if res is not None else (w, h)
    ctx.set_kernel_variant(variant)
    ctx.set_storage(capi.STORAGE_F16 if f16 else capi.STORAGE_F32)
    ctx.set_pipelining(pipelining)
    ctx.set_present_mode(capi.PRESENT_EXACT)
    ctx.set_option(capi.OPT_BATCH, batch if batch is not None else 256)
    ctx.set_tile(*tile)
    ctx.set_moments(moments)
    pc.upload_scene(ctx, sc, env)
    ctx.resize(w, h)
    ctx.reset_counters()
    ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(w, h, 1.0, 0, 1).tobytes())

    def uniforms(step):
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=step[0], bounces=bounces, res=res).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(rw, rh, step[1], step[2]).tobytes())

    if submit == "frames":
        uniforms(steps[0])
        ctx.submit_frames(MASK, len(steps))
    else:
        for k, step in enumerate(steps):
            uniforms(step)
            if submit == "separate":
                ctx.submit(capi.SUBMIT_RAYTRACE)
                ctx.submit(capi.SUBMIT_ACCUMULATE)
            else:
                ctx.submit(MASK | (capi.SUBMIT_FULLSCREEN if k == present_at else 0))
    acc = ctx.read_texture(capi.TEX_ACCUMULATION)
    out = (acc, ctx.read_moments() if moments else None, ctx.counters(), ctx.last_launch())
    ctx.set_moments(False)
    return out


def _check(ctx, orc, sc, env, w, h, steps, what, same_launch=True, **kw):
    ref_kw = {k: kw[k] for k in ("bounces", "f16", "tile", "res") if k in kw}
    want_mean, want_m = _reference(orc, sc, env, w, h, steps, **ref_kw)
    off_acc, _, off_cnt, off_launch = _device(ctx, sc, env, w, h, steps, False, **kw)
    acc, m, cnt, launch = _device(ctx, sc, env, w, h, steps, True, **kw)
    assert m.shape == want_m.shape and m.dtype == np.float32
    assert pc.same_bits(m, want_m), f"{what}: moments: " + pc.describe_diff(m, want_m)
    assert pc.same_bits(acc, want_mean), f"{what}: mean: " + pc.describe_diff(acc, want_mean)
    assert acc.tobytes() == off_acc.tobytes(), f"{what}: the mean with moments on differs from the mean with moments off"
    # (the box / triangle-test counts of the culling walks depend on which lanes walk together, i.e. on the job order of the launch, which
    # the cost feedback changes from run to run with or without moments: compared where the walk is the reference's, variants 1 - 8)
    for k in pc.PATH_COUNTERS + (pc.WALK_COUNTERS if 1 <= kw.get("variant", 0) <= 8 else ()):
        assert cnt[k] == off_cnt[k], f"{what}: counter {k}: {cnt[k]} != {off_cnt[k]}"
    if same_launch:
        assert launch == off_launch, f"{what}: last launch {launch} != {off_launch}"
    return m, want_m


def test_reference_base_case_is_not_vacuous(orc, demo, env):
    """Asserted on the reference alone (measured: 1.000 of the texels at 4 frames in F32 and F16; no negative channel)."""
    for f16 in (False, True):
        _, m = _reference(orc, demo, env, 64, 64, BASE_STEPS, f16=f16)
        share = float((((m[..., 0] + m[..., 1]) + m[..., 2]) > 0).mean())
        print(f"F16 {f16}: {share:.3f} of the texels have a spread")
        assert share >= 0.9
        assert not (m[..., :3] < 0).any() and np.all(m[..., 3] == 4)


PATHS = {
    "one batched launch": dict(submit="frames"),
    "a submit per frame, queued": dict(submit="each"),
    "EXACT presentation in the middle of a batch": dict(submit="each", present_at=1),
    "pipelining off": dict(submit="each", pipelining=False),
    "separate RAYTRACE and ACCUMULATE submits": dict(submit="separate"),
    "F16 storage, batched": dict(submit="frames", f16=True),
    "F16 storage, pipelining off": dict(submit="each", f16=True, pipelining=False),
}


@pytest.mark.parametrize("path", list(PATHS), ids=[p.replace(" ", "-") for p in PATHS])
def test_base_case_through_every_path(ctx, orc, demo, env, path):
    _check(ctx, orc, demo, env, 64, 64, BASE_STEPS, path, **PATHS[path])


def test_moments_are_carried_across_launches(ctx, orc, demo, env):
    """7 frames with MI3PT_OPT_BATCH 3: launches of 3, 3 and 1 frames"""
    steps = tuple((f, f, 1) for f in range(1, 8))
    m, _ = _check(ctx, orc, demo, env, 64, 64, steps, "batch 3", submit="frames", batch=3)
    assert np.all(m[..., 3] == 7)


@pytest.mark.parametrize("variant", [1, 2])
def test_per_pixel_kernels_run_two_passes(ctx, orc, demo, env, variant):
    """Variants 1 / 2 fold the accumulate pass into the raytrace kernel; with moments on the two passes run separately: same image, same
    counters (the launch is not compared)."""
    pc.set_variant_or_skip(ctx, variant)
    _check(ctx, orc, demo, env, 64, 64, BASE_STEPS, f"variant {variant}", same_launch=False, submit="each", variant=variant)


@pytest.mark.parametrize("rank,nranks", [(1, 2), (2, 3)])
def test_ranks_of_a_tile_split(ctx, orc, demo, env, rank, nranks):
    """100 x 52: ragged blocks; the image is the rank's compact rows"""
    for submit in ("frames", "separate"):
        m, _ = _check(ctx, orc, demo, env, 100, 52, BASE_STEPS, f"rank {rank} of {nranks}, {submit}", submit=submit, tile=(rank, nranks, 8))
        assert m.shape[0] == capi.tile_local_rows(52, rank, nranks, 8) < 52


def _group_run(g, demo, env, w, h, moments):
    g.set_moments(moments)
    pc.upload_scene(g, demo, env)
    g.resize(w, h)
    g.reset_counters()
    g.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=1, bounces=4).tobytes())
    g.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1).tobytes())
    g.submit_frames(MASK, 4)
    return g.read_texture(capi.TEX_ACCUMULATION), g.counters(), g.last_launch()


def test_group_gathers_the_single_context_image(ctx, orc, demo, env):
    """A group of [0, 0]: mean, path counters and launch equal a run of the group with moments off (and the oracle's mean); the gathered
    moments image equals the reference's and the single context's"""
    w, h = 100, 52
    want_mean, want_m = _reference(orc, demo, env, w, h, BASE_STEPS)
    with capi.Context(devices=[0, 0]) as g:
        off_acc, off_cnt, off_launch = _group_run(g, demo, env, w, h, False)
        with pytest.raises(capi.Mi3ptError) as e:
            g.read_moments()
        assert e.value.code == 4
        acc, cnt, launch = _group_run(g, demo, env, w, h, True)
        assert pc.same_bits(acc, want_mean), pc.describe_diff(acc, want_mean)
        assert acc.tobytes() == off_acc.tobytes(), "group: the mean with moments on differs from the mean with moments off"
        for k in pc.PATH_COUNTERS:
            assert cnt[k] == off_cnt[k], f"group: counter {k}: {cnt[k]} != {off_cnt[k]}"
        assert launch == off_launch, f"group: last launch {launch} != {off_launch}"
        m = g.read_moments()
        assert m.shape == (h, w, 4)
        assert pc.same_bits(m, want_m), pc.describe_diff(m, want_m)
        assert g.read_texture(capi.TEX_ACCUMULATION).tobytes() == acc.tobytes()             # (the gather of one image leaves the other alone)
        ptr, nbytes = g.moments_device_ptr()
        assert ptr and nbytes == w * h * 16
        with pytest.raises(capi.Mi3ptError) as e:
            g.write_moments(m)
        assert e.value.code == 4
        # the staged gather (no peer access) moves the same bytes
        g.set_option(capi.OPT_GATHER_STAGED, 1)
        assert g.read_moments().tobytes() == m.tobytes()
        # a resize zeroes every member's image and frees the gathered copy; reset zeroes
        g.resize(w, h)
        assert not g.read_moments().any()
        g.set_moments(False)
        with pytest.raises(capi.Mi3ptError) as e:
            g.read_moments()
        assert e.value.code == 4
    single, _ = _check(ctx, orc, demo, env, w, h, BASE_STEPS, "single context 100 x 52", submit="frames")
    assert single.tobytes() == m.tobytes()


def test_binding_another_accumulation_image_restarts_the_moments(ctx, demo, env):
    """mi3pt_bind_accumulation swaps another image in as the mean (here: back to the context's own): like write_texture it zeroes the moments"""
    w = h = 16
    ctx.set_tile(0, 1, 8)
    ctx.set_moments(True)
    pc.upload_scene(ctx, demo, env)
    ctx.resize(w, h)
    ctx.write_moments(np.full((h, w, 4), 3.0, np.float32))
    assert ctx.read_moments().all()
    ctx.bind_accumulation(None, 0)
    assert not ctx.read_moments().any()
    ctx.set_moments(False)


RESTARTS = {
    "frame counters 1, 2, 3, 1, 2": ((1, 1, 1), (2, 2, 1), (3, 3, 1), (4, 1, 1), (5, 2, 1)),
    "enabled 0 in the middle": ((1, 1, 1), (2, 2, 1), (3, 3, 0), (4, 4, 1)),
    "enabled 0 at the end": ((1, 1, 1), (2, 2, 1), (3, 3, 0)),
    "0xFFFFFFFF followed by 0": ((7, 0xFFFFFFFE, 1), (8, 0xFFFFFFFF, 1), (9, 0, 1)),
    "0xFFFFFFFF, 0, 1, 2": ((7, 0xFFFFFFFE, 1), (8, 0xFFFFFFFF, 1), (9, 0, 1), (10, 1, 1), (11, 2, 1)),
}


@pytest.mark.parametrize("name", list(RESTARTS), ids=[n.replace(" ", "-").replace(",", "") for n in RESTARTS])
@pytest.mark.parametrize("pipelining", [True, False], ids=["queued", "immediate"])
def test_restarts(ctx, orc, demo, env, name, pipelining):
    steps = RESTARTS[name]
    m, want = _check(ctx, orc, demo, env, 64, 64, steps, name, submit="each", pipelining=pipelining)
    last_restart = max(k for k, s in enumerate(steps) if (s[1] & 0xFFFFFFFF) <= 1 or s[2] != 1)
    assert np.all(want[..., 3] == len(steps) - last_restart)


def test_consecutive_counters_that_wrap_in_one_batch(ctx, orc, demo, env):
    """raytrace and accumulate counters both run through 2^32 inside one submit_frames: the batch kernel restarts at 0 and at 1"""
    steps = tuple(((0xFFFFFFFE + k) & 0xFFFFFFFF, (0xFFFFFFFE + k) & 0xFFFFFFFF, 1) for k in range(5))
    m, want = _check(ctx, orc, demo, env, 64, 64, steps, "wrap in a batch", submit="frames")
    assert np.all(want[..., 3] == 2)


def test_resolution_smaller_than_the_texture(ctx, orc, demo, env):
    w = h = 64
    res = (40, 24)
    for submit in ("frames", "separate"):
        m, want = _check(ctx, orc, demo, env, w, h, BASE_STEPS, f"resolution {res}, {submit}", submit=submit, res=res)
        assert not want[24:].any() and not want[:, 40:].any() and np.all(want[:24, :40, 3] == 4)
        assert not m[24:].any() and not m[:, 40:].any()


@pytest.mark.parametrize("submit", ["frames", "separate"])
def test_past_the_grid_cap(ctx, orc, demo, env, submit):
    """1100 x 1000 = 1.1 M texels: 4297 blocks of 256, past the 4096- and 2048-block grids of the two kernels, which stride beyond"""
    steps = tuple((f, f, 1) for f in range(1, 4))
    m, want = _check(ctx, orc, demo, env, 1100, 1000, steps, f"1100 x 1000, {submit}", submit=submit, bounces=1)
    assert np.all(want[..., 3] == 3) and (want[-1, :, :3] > 0).any()


CAP_CASES = {
    # the accumulate-only path of mi3pt_submit launches at most 2048 blocks of 256: 1024 x 520 is 2080
    "accumulate-only-1024x520": dict(w=1024, h=520, cap=2048, submit="separate"),
    # the batched path at most 4096: 1024 x 1032 is 4128
    "batched-f32-1024x1032": dict(w=1024, h=1032, cap=4096, submit="frames"),
    "batched-f16-1024x1032": dict(w=1024, h=1032, cap=4096, submit="frames", f16=True),
}


@pytest.mark.parametrize("case", list(CAP_CASES))
def test_one_row_of_blocks_past_each_grid_cap(ctx, orc, demo, env, case):
    """Three frames at two bounces, at the smallest sizes of 1024 columns whose block count exceeds each caller's cap: the last 32 blocks'
    texels are the strided second iteration of 8192 threads and of no other.  The radiance and the means are the ORACLE's
    (moments_reference.oracle_steps, as everywhere in this module: 0.5 - 0.7 s for the three frames); the strided texels have n = 3 and a
    spread in the reference."""
    c = dict(CAP_CASES[case])
    w, h, cap = c.pop("w"), c.pop("h"), c.pop("cap")
    steps = tuple((f, f, 1) for f in range(1, 4))
    assert cap * 256 < w * h <= 2 * cap * 256
    m, want = _check(ctx, orc, demo, env, w, h, steps, case, bounces=2, **c)
    strided = want.reshape(-1, 4)[cap * 256:]
    spread = (strided[:, :3] != 0).any(axis=1)
    print(f"{case}: {len(strided)} strided texels, {spread.mean():.4f} of them with a non-zero M2")
    assert np.all(strided[:, 3] == 3) and spread.mean() > 0.5       # (measured on the CPU: 1.00 in F32, 0.91 in F16)


def test_non_finite_radiance_is_carried(ctx, orc, env):
    """Two frames of the palette of tests/shading_cases.py (six bounces: NaN and inf radiance): NaNs sit where the reference puts them"""
    sc = sh.palette_scene()
    steps = ((sh.PALETTE_FRAMES[0], 1, 1), (sh.PALETTE_FRAMES[1], 2, 1))
    m, want = _check(ctx, orc, sc, env, sh.W, sh.H, steps, "palette", submit="each", bounces=sh.PALETTE_BOUNCES)
    bad = ~np.isfinite(want[..., :3])
    print(f"palette: {int(np.isnan(want[..., :3]).sum())} NaN and {int(np.isinf(want[..., :3]).sum())} infinite M2 values")
    assert bad.any() and np.isnan(want[..., :3]).any()
    assert np.array_equal(np.isnan(m), np.isnan(want))


def _code(fn, *a, **kw):
    with pytest.raises(capi.Mi3ptError) as e:
        fn(*a, **kw)
    return e.value.code


def test_life_cycle_and_errors(orc, demo, env):
    w = h = 16
    rng = np.random.default_rng(5)
    with capi.Context(0) as c:
        assert _code(c.read_moments) == 4 and _code(c.moments_device_ptr) == 4          # never enabled
        assert _code(c.write_moments, np.zeros((1, 1, 4), np.float32)) == 4
        c.set_moments(True)
        assert _code(c.read_moments) == 4 and _code(c.moments_device_ptr) == 4          # enabled, before resize
        pc.upload_scene(c, demo, env)
        c.resize(w, h)
        assert not c.read_moments().any()                                                # allocated and zeroed with the textures
        image = rng.random((h, w, 4), dtype=np.float32)
        c.write_moments(image)
        assert c.read_moments().tobytes() == image.tobytes()                             # round trip
        out = np.empty((h, w, 4), np.float32)
        p = out.ctypes.data_as(ctypes.c_void_p)
        for call in (c.lib.mi3pt_read_moments, c.lib.mi3pt_write_moments):
            assert call(c.handle, p, out.nbytes - 16) == 1 and call(c.handle, p, out.nbytes + 16) == 1      # wrong nbytes
            assert call(c.handle, None, out.nbytes) == 1
        assert c.lib.mi3pt_moments_device_ptr(c.handle, None, None) == 1
        assert c.read_moments().tobytes() == image.tobytes()
        c.reset()
        assert not c.read_moments().any()                                                # reset zeroes
        c.write_moments(image)
        c.write_texture(capi.TEX_ACCUMULATION, rng.random((h, w, 4), dtype=np.float32))
        assert not c.read_moments().any()                                                # a mean from outside: unknown spread
        c.write_moments(image)                                                           # ... and a checkpoint restores it
        assert c.read_moments().tobytes() == image.tobytes()
        c.resize(w + 3, h + 1)
        assert c.read_moments().shape == (h + 1, w + 3, 4) and not c.read_moments().any()       # resize re-allocates and zeroes
        c.set_moments(False)
        assert _code(c.read_moments) == 4 and _code(c.moments_device_ptr) == 4
        assert _code(c.write_moments, np.zeros((h + 1, w + 3, 4), np.float32)) == 4
        c.set_moments(True)                                                              # enabled after resize: allocated and zeroed now
        assert not c.read_moments().any()
        # frames queued before the switch are launched first: the image counts exactly the frames submitted after it
        c.set_moments(False)
        c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w + 3, h + 1, frame=1, bounces=2).tobytes())
        c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w + 3, h + 1, 1).tobytes())
        c.submit_frames(MASK, 2)
        c.set_moments(True)
        c.submit_frames(MASK, 3)
        assert np.all(c.read_moments()[..., 3] == 3)
        # the device pointer holds the bytes of read_moments
        try:
            hip = ctypes.CDLL("libamdhip64.so")
        except OSError:
            import os
            hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        want = c.read_moments()
        ptr, nbytes = c.moments_device_ptr()
        assert ptr and nbytes == want.nbytes
        host = np.empty_like(want)
        assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ptr, nbytes, 2) == 0          # hipMemcpyDeviceToHost
        assert host.tobytes() == want.tobytes()
    assert capi.load_library().mi3pt_abi_version() == 4
