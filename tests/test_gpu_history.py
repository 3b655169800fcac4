"""The held history on the GPU (mi3pt_hold_history, mi3pt_merge_history; csrc/pt_history.hip) against its numpy restatement
tests/history_reference.py, bit for bit (ptcommon.same_bits, no tolerance anywhere).  The reference is given what the kernel is given:
the two (mean, moments) pairs written with mi3pt_write_texture / mi3pt_write_moments, or sampled, as the device returns them."""
import ctypes

import numpy as np
import pytest

import history_reference as hr
import moments_edge_cases as ec
import ptcommon as pc
import reproject_scene_cases as cases
import test_gpu_reproject as tgr
from mi3pt_host import capi

pytestmark = pytest.mark.gpu
RT, ACC = capi.SUBMIT_RAYTRACE, capi.SUBMIT_ACCUMULATE
TEX = capi.TEX_ACCUMULATION
F = np.float32
# neither dimension a multiple of the kernel's 32 x 8 tile, more than one block each way; 8 x 8 with radius 3: the window exceeds the image
SIZES = [(48, 32), (40, 24)]


@pytest.fixture(scope="module")
def ctx(built):
    c = capi.Context(0)
    yield c
    c.close()


def _code(fn):
    with pytest.raises(capi.Mi3ptError) as e:
        fn()
    return e.value.code


def _random_pair(w, h, seed, near=None):
    """tgr._random_images (n of 0, 1, 2 and 500 among the texels) with a NaN count; near: a mean to stay close to on half of the texels, so
    that the test keeps all, some and none of the history among them"""
    rng = np.random.default_rng(seed)
    acc, mo = tgr._random_images(w, h, seed)
    mo[..., :3] *= F(0.02) * np.maximum(mo[..., 3:], F(1))          # a per-sample variance of up to 1
    if near is not None:
        step = (rng.random((h, w, 3), dtype=F) - F(0.5)) * rng.choice(np.array([0.0, 0.05, 0.5], F), size=(h, w, 1))
        acc[..., :3] = np.where(rng.random((h, w, 1)) < 0.7, near[..., :3] + step, acc[..., :3])
    mo[rng.integers(h), rng.integers(w), 3] = np.nan
    return acc, mo


def _write(c, pair):
    c.write_texture(TEX, pair[0])
    c.write_moments(pair[1])
    return c.read_texture(TEX), c.read_moments()


def _case(c, w, h, seed=1, rect=None, f16=False, **params):
    """the held pair written and held, the fresh pair written, the merge.  Returns (device (A', M'), reference (A', M', info), the two
    pairs as the device returned them)"""
    c.reset()
    c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(*(rect or (w, h)), 2).tobytes())
    held = _random_pair(w, h, seed)
    if f16:
        held = (held[0].astype(np.float16).astype(F), held[1])
    held = _write(c, held)
    c.hold_history()
    zeroed = c.read_texture(TEX), c.read_moments()
    assert not zeroed[0].view(np.uint32).any() and not zeroed[1].view(np.uint32).any(), "the live pair after the hold"
    live = _random_pair(w, h, seed + 100, near=held[0])
    if f16:
        live = (live[0].astype(np.float16).astype(F), live[1])
    live = _write(c, live)
    c.merge_history(**params)
    got = c.read_texture(TEX), c.read_moments()
    kw = {k: params[k] for k in ("radius", "z_keep", "z_drop") if k in params}
    want = hr.merge_history(live[0], live[1], held[0], held[1], rect, store_f16=f16, **kw)
    return got, want, (live, held)


def _every_branch(info):
    return all(info[k].any() for k in ("merged", "dropped", "only_held", "neither"))


def _merge(c, w, h, held, live, rect=None, f16=False, **params):
    """_case with the two pairs given.  Returns (device (A', M'), reference (A', M', info), the two pairs as the device returned them)"""
    c.reset()
    c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(*(rect or (w, h)), 2).tobytes())
    if f16:
        held, live = (hr.store_round(held[0], True), held[1]), (hr.store_round(live[0], True), live[1])
    held = _write(c, held)
    c.hold_history()
    live = _write(c, live)
    c.merge_history(**params)
    got = c.read_texture(TEX), c.read_moments()
    kw = {k: params[k] for k in ("radius", "z_keep", "z_drop") if k in params}
    want = hr.merge_history(live[0], live[1], held[0], held[1], rect, store_f16=f16, **kw)
    return got, want, (live, held)


def edge_pairs(w, h, seed, finite):
    """(held, live): _random_pair's pairs with the catalogue of tests/moments_edge_cases.py written over BOTH sides, under different
    permutations, so that an edge texel meets plain ones and other edge texels; on both sides of x = 31 | 32 and y = 7 | 8 (and every
    other multiple of 8): the halo staging carries edge values"""
    held = _random_pair(w, h, seed)
    live = _random_pair(w, h, seed + 100, near=held[0])
    where_held = ec.overlay(held[0], held[1], seed, finite)
    where_live = ec.overlay(live[0], live[1], seed + 1, finite)
    assert not ec.seam_sides(where_held, w, h) and not ec.seam_sides(where_live, w, h)
    return held, live


def describe_branches(info, live, held, what):
    """the merge's value branches taken by a reference run, printed; returns the counts"""
    both = (live[1][..., 3] >= 1) & (held[1][..., 3] >= 1)
    lam = info["lam"][both]
    count = {k: int(info[k].sum()) for k in ("merged", "dropped", "only_held", "neither")}
    count.update(lam0=int((lam == 0).sum()), lam1=int((lam == 1).sum()), between=int(((lam > 0) & (lam < 1)).sum()), lam_nan=int(np.isnan(lam).sum()),
                 one_kept=int((info["merged"] & (info["nk"] == 1)).sum()))
    print(f"{what}: {count}")
    return count


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_device_equals_the_reference(ctx, demo, env, w, h, radius):
    tgr._configure(ctx, demo, env, w, h)
    got, want, (live, held) = _case(ctx, w, h, seed=radius + 1, radius=radius)
    tgr._same(got, want, f"radius {radius}, {w} x {h}")
    info = want[2]
    both = (live[1][..., 3] >= 1) & (held[1][..., 3] >= 1)
    print(f"radius {radius}, {w} x {h}: merged {int(info['merged'].sum())}, dropped {int(info['dropped'].sum())}, only held "
          f"{int(info['only_held'].sum())}, neither {int(info['neither'].sum())}; of {int(both.sum())} texels with both sides "
          f"{int((info['lam'][both] == 1).sum())} keep all, {int((info['lam'][both] == 0).sum())} none")
    assert _every_branch(info)
    part = both & (info["lam"] > 0) & (info["lam"] < 1)
    assert part.any() and (info["lam"][both] == 1).any() and (info["lam"][both] == 0).any()
    # other thresholds
    got, want, _ = _case(ctx, w, h, seed=radius + 11, radius=radius, z_keep=0.0, z_drop=1.5)
    tgr._same(got, want, f"radius {radius}, {w} x {h}, z 0 / 1.5")


def test_a_window_larger_than_the_image(ctx, demo, env):
    tgr._configure(ctx, demo, env, 8, 8)
    for seed in (1, 2):
        got, want, _ = _case(ctx, 8, 8, seed=seed, radius=3)
        tgr._same(got, want, f"8 x 8, radius 3, seed {seed}")


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_value_edges(ctx, demo, env, w, h, radius):
    """the finite catalogue on both sides: counts on either side of `n >= 1` and `n >= 2`, M2 that the fmaxf clamps or that overflow the
    pooled variance, means whose difference overflows.  Finite inputs, but not finite results: compared with ptcommon.same_bits_or_nan,
    every texel.  At radius 1 also under F16 storage (the means 65504 and 65520: the largest binary16 and an infinity once stored)"""
    tgr._configure(ctx, demo, env, w, h)
    held, live = edge_pairs(w, h, 20 + radius, finite=True)
    got, want, (live, held) = _merge(ctx, w, h, held, live, radius=radius)
    count = describe_branches(want[2], live, held, f"radius {radius}, {w} x {h}")
    assert _every_branch(want[2]) and count["lam0"] and count["lam1"] and count["between"] and count["one_kept"]
    tgr._same_or_nan(got, want, f"radius {radius}, {w} x {h}")
    if radius == 1:
        try:
            tgr._configure(ctx, demo, env, w, h, f16=True)
            held, live = edge_pairs(w, h, 30, finite=True)
            got, want, (live, held) = _merge(ctx, w, h, held, live, f16=True, radius=1)
            assert (live[0] == 65504).any() and np.isinf(live[0]).any() and want[2]["merged"].any()
            tgr._same_or_nan(got, want, f"F16, radius 1, {w} x {h}")
        finally:
            tgr._restore(ctx)


def test_threshold_edges(ctx, demo, env):
    """the worked examples of tests/moments_edge_cases.py (THRESHOLDS) as texels of a 40 x 24 image without samples anywhere else, radius
    0, each at three places (one on either side of y = 7 | 8; the eight that share z 2 / 4 lie across x = 31 | 32): z2 exactly at keep2 and at
    drop2, one ulp inside either, lam = 1/2 with nk - 1 = 0, counts of 1.5, an M2 that is a NaN on one side only in the channel that
    decides (var()'s fmaxf drops it), and a z-score that is a NaN in one channel (the fmaxf over the channels drops it).  The device against the reference, and the reference against the stated
    values"""
    w, h = SIZES[1]
    tgr._configure(ctx, demo, env, w, h)
    for z in sorted({t["z"] for t in ec.THRESHOLDS}):
        group = [t for t in ec.THRESHOLDS if t["z"] == z]
        held, live = (np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)), (np.zeros((h, w, 4), F), np.zeros((h, w, 4), F))
        at = {}
        for i, t in enumerate(group):
            at[t["name"]] = [(1 + 3 * i, 2), (7, 29 + i), (8, 29 + i)]
            for y, x in at[t["name"]]:
                for pair, (mean, m2, n) in ((live, t["live"]), (held, t["held"])):
                    pair[0][y, x] = (*mean, 1)
                    pair[1][y, x] = (*m2, n)
        got, want, _ = _merge(ctx, w, h, held, live, radius=0, z_keep=z[0], z_drop=z[1])
        tgr._same(got, want, f"thresholds, z {z}")
        info = want[2]
        for t in group:
            for y, x in at[t["name"]]:
                print(f"{t['name']} at ({x}, {y}): z2 {info['z2'][y, x]!r}, lam {info['lam'][y, x]!r}, nk {info['nk'][y, x]}, mean {want[0][y, x, 0]!r}, "
                      f"M2 {want[1][y, x, 0]!r}, N {want[1][y, x, 3]}")
                assert abs(float(info["lam"][y, x]) - float(t["lam"])) <= 1e-9 and info["nk"][y, x] == t["nk"], t["name"]
                assert bool(info["merged"][y, x]) == (t["merged"] is not None) and bool(info["dropped"][y, x]) == (t["merged"] is None), t["name"]
                if t["merged"] is not None:
                    assert (want[0][y, x, 0], want[1][y, x, 0], want[1][y, x, 3]) == t["merged"], t["name"]
                    assert (got[0][y, x, 0], got[1][y, x, 0], got[1][y, x, 3]) == t["merged"], t["name"]
                else:
                    assert pc.same_bits(got[0][y, x], live[0][y, x]) and pc.same_bits(got[1][y, x], live[1][y, x]), t["name"]


@pytest.mark.parametrize("case", ec.Z_EXTREMES, ids=[c["name"] for c in ec.Z_EXTREMES])
def test_parameter_extremes(ctx, demo, env, case):
    """z_drop whose square overflows; squares that are both 0; squares that are the same subnormal: lam = 0 wherever both sides hold
    samples -- except, for the equal non-zero squares, at a texel whose pooled difference is exactly 0: z2 = 0, the quotient is +inf and
    lam = 1 (the header's formula; _random_pair leaves the live mean equal to the held one at a sixth of the texels)"""
    w, h = SIZES[0]
    tgr._configure(ctx, demo, env, w, h)
    z_keep, z_drop = case["z"]
    got, want, (live, held) = _case(ctx, w, h, seed=7, radius=0, z_keep=z_keep, z_drop=z_drop)
    tgr._same(got, want, case["name"])
    both = (live[1][..., 3] >= 1) & (held[1][..., 3] >= 1)
    d0 = both & (live[0][..., :3] == held[0][..., :3]).all(axis=-1)
    lam = want[2]["lam"]
    print(f"{case['name']}: {int(both.sum())} texels with both sides, {int(d0.sum())} of them with a difference of exactly 0; lam there "
          f"{np.unique(lam[d0]).tolist()}, elsewhere {np.unique(lam[both & ~d0]).tolist()}")
    assert d0.sum() >= 20 and (both & ~d0).sum() >= 20
    assert np.all(lam[d0] == case["lam_d0"]) and np.all(lam[both & ~d0] == case["lam"])
    if case["lam_d0"] == 1:
        assert np.all(got[1][..., 3][d0] == live[1][..., 3][d0] + np.floor(held[1][..., 3][d0]))          # the whole held history is kept there
    got, want, _ = _case(ctx, w, h, seed=8, radius=2, z_keep=z_keep, z_drop=z_drop)
    tgr._same(got, want, case["name"] + ", radius 2")


@pytest.mark.parametrize("radius", [0, 3])
def test_non_finite_images(ctx, demo, env, radius):
    """the whole catalogue, NaN and infinite counts, sums and means included, on both sides, over a rectangle smaller than the image: inside,
    the reference's bits and a NaN where it has one (every texel); outside, the live bits exactly.  pt_history.hip: "images of NaNs or
    infinities neither hang nor fault" -- no index depends on a value"""
    w, h = SIZES[0]
    tgr._configure(ctx, demo, env, w, h)
    rect = (w - 9, h - 5)
    held, live = edge_pairs(w, h, 40 + radius, finite=False)
    got, want, (live, held) = _merge(ctx, w, h, held, live, rect=rect, radius=radius)
    describe_branches(want[2], live, held, f"non-finite, radius {radius}")
    assert _every_branch(want[2])
    tgr._same_or_nan(got, want, f"non-finite, radius {radius}")
    for g, written in zip(got, live):
        assert np.array_equal(g[rect[1]:].view(np.uint32), written[rect[1]:].view(np.uint32))
        assert np.array_equal(g[:, rect[0]:].view(np.uint32), written[:, rect[0]:].view(np.uint32))


@pytest.mark.parametrize("w,h", SIZES)
def test_f16_storage_a_rectangle_and_a_bound_image(ctx, demo, env, w, h):
    try:
        tgr._configure(ctx, demo, env, w, h, f16=True)
        got, want, _ = _case(ctx, w, h, f16=True, radius=1)
        tgr._same(got, want, f"F16, {w} x {h}")
        assert want[2]["merged"].any() and pc.same_bits(got[0], got[0].astype(np.float16).astype(F))
        tgr._configure(ctx, demo, env, w, h)
        rect = (w - 9, h - 5)
        got, want, (live, _) = _case(ctx, w, h, rect=rect, radius=2)
        tgr._same(got, want, f"rectangle {rect}, {w} x {h}")
        assert pc.same_bits(got[0][rect[1]:], live[0][rect[1]:]) and pc.same_bits(got[1][:, rect[0]:], live[1][:, rect[0]:])
        # a caller-owned accumulation image: copied out on the stream by the hold, the result copied into it by the merge
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipFree.argtypes = [ctypes.c_void_p]
        bound, nbytes = ctypes.c_void_p(), h * w * 16
        assert hip.hipMalloc(ctypes.byref(bound), nbytes) == 0 and hip.hipMemset(bound, 0, nbytes) == 0 and hip.hipDeviceSynchronize() == 0
        ctx.bind_accumulation(bound.value, nbytes)
        try:
            got, want, _ = _case(ctx, w, h, rect=rect, radius=1)
            tgr._same(got, want, f"bound image, {w} x {h}")
            host = np.empty((h, w, 4), F)
            assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), bound, nbytes, 2) == 0          # hipMemcpyDeviceToHost
            assert pc.same_bits(host, want[0])
        finally:
            ctx.bind_accumulation(None, 0)
            hip.hipFree(bound)
    finally:
        tgr._restore(ctx)


def _sampled(c, demo, w, h, frames, first_frame, prepare):
    """`prepare`, then `frames` frames of the demo scene under the mean by count: (mean, moments)"""
    c.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h, frame=first_frame).tobytes())
    c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
    prepare()
    c.submit_frames(RT | ACC, frames)
    return c.read_texture(TEX), c.read_moments()


def test_hold_is_a_reset_that_remembers(ctx, demo, env):
    w, h = SIZES[1]
    tgr._configure(ctx, demo, env, w, h)
    ctx.reset()
    _sampled(ctx, demo, w, h, 2, 2, lambda: None)
    before = ctx.counters(), ctx.last_launch()
    held = _sampled(ctx, demo, w, h, 3, 40, ctx.hold_history)
    again = _sampled(ctx, demo, w, h, 3, 40, ctx.reset)
    tgr._same(held, again, "hold + 3 frames against reset + 3 frames")
    assert held[1][..., 3].max() == 3 and before[0]["rays"] < ctx.counters()["rays"]


def test_reproject_scene_hold_frames_merge(ctx, demo, env):
    """mi3pt_reproject_scene -> hold -> 4 frames -> merge equals the numpy law on the pairs the device returns on the way; no counter and
    nothing mi3pt_debug_last_launch reports moves in hold or merge; the sample mask stays"""
    w, h = SIZES[0]
    tgr._configure(ctx, demo, env, w, h)
    ctx.reset()
    _sampled(ctx, demo, w, h, 8, 2, lambda: None)
    ctx.render_aovs(capi.AOV_ALL)
    ctx.keep_geometry(True)
    try:
        pc.upload_scene(ctx, cases.box_moved(demo, shift=(0.6, 0.0, 0.0), degrees=0.0))
        ctx.reproject_scene()
        carried = ctx.read_texture(TEX), ctx.read_moments()
        mask = np.ones(((h + 7) // 8, (w + 7) // 8), np.uint8)
        mask[0, 0] = 0
        ctx.set_sample_mask(mask)
        before = ctx.counters(), ctx.last_launch()
        ctx.hold_history()
        assert (ctx.counters(), ctx.last_launch()) == before and np.array_equal(ctx.read_sample_mask(), mask)
        fresh = _sampled(ctx, demo, w, h, 4, 70, lambda: None)
        before = ctx.counters(), ctx.last_launch()
        ctx.merge_history(radius=1)
        got = ctx.read_texture(TEX), ctx.read_moments()
        assert (ctx.counters(), ctx.last_launch()) == before and np.array_equal(ctx.read_sample_mask(), mask)
    finally:
        ctx.keep_geometry(False)
        pc.upload_scene(ctx, demo)
    want = hr.merge_history(fresh[0], fresh[1], carried[0], carried[1], radius=1)
    tgr._same(got, want, "reproject_scene, hold, 4 frames, merge")
    info = want[2]
    share = hr.kept_share(fresh[1], got[1], carried[1])
    print(f"merged {int(info['merged'].sum())}, dropped {int(info['dropped'].sum())}, only held {int(info['only_held'].sum())}; kept share {share:.3f}")
    assert info["merged"].any() and info["only_held"].any()          # (the masked tile took no fresh frame)
    assert got[1][..., 3].max() == 12


def test_queued_frames_are_flushed_under_the_old_images(ctx, demo, env):
    """frames queued but not launched before a hold belong to the held history; frames queued before a merge are fresh samples"""
    w, h = SIZES[1]
    tgr._configure(ctx, demo, env, w, h)

    def run(flush):
        ctx.reset()
        ctx.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
        ctx.submit_frames(RT | ACC, 5)
        if flush:
            ctx.sync()
        ctx.hold_history()
        ctx.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h, frame=30).tobytes())
        ctx.submit_frames(RT | ACC, 2)
        if flush:
            ctx.sync()
        ctx.merge_history()
        return ctx.read_texture(TEX), ctx.read_moments()

    queued, flushed = run(False), run(True)
    tgr._same(queued, flushed, "queued against flushed")
    assert flushed[1][..., 3].max() == 7


def test_states_and_error_codes(ctx, demo, env):
    lib = capi.load_library()
    good = capi.HistoryParams(1, 2.0, 4.0, 0)
    assert lib.mi3pt_merge_history(None, ctypes.byref(good)) == 1 and lib.mi3pt_hold_history(None) == 1
    w, h = SIZES[1]
    tgr._configure(ctx, demo, env, w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
    # nothing held; merged twice; a second hold replaces the first
    assert _code(ctx.merge_history) == 4
    ctx.hold_history()
    ctx.merge_history()
    assert _code(ctx.merge_history) == 4
    first = _write(ctx, _random_pair(w, h, 5))
    ctx.hold_history()
    second = _write(ctx, _random_pair(w, h, 6))
    ctx.hold_history()
    ctx.merge_history()
    nothing = np.zeros((h, w, 4), F)
    want = hr.merge_history(nothing, nothing, second[0], second[1])
    tgr._same((ctx.read_texture(TEX), ctx.read_moments()), want, "a second hold replaces the first")
    assert want[2]["only_held"].any() and not want[2]["merged"].any() and not pc.same_bits(first[0], second[0])
    # the arguments
    ctx.hold_history()
    assert lib.mi3pt_merge_history(ctx.handle, None) == 1
    for bad in (dict(radius=-1), dict(radius=4), dict(z_keep=-0.5), dict(z_keep=float("nan")), dict(z_keep=float("inf"), z_drop=float("inf")),
                dict(z_drop=2.0), dict(z_drop=1.0), dict(z_drop=float("nan")), dict(z_drop=float("inf")), dict(flags=1)):
        assert _code(lambda: ctx.merge_history(**bad)) == 1, bad
    ctx.merge_history(radius=0, z_keep=0.0, z_drop=1e-3)
    # what drops a held history
    ctx.hold_history()
    ctx.reset()
    assert _code(ctx.merge_history) == 4
    ctx.hold_history()
    ctx.resize(w, h)
    assert _code(ctx.merge_history) == 4
    ctx.set_uniforms(capi.PASS_RAYTRACE, tgr._uniforms(demo, w, h).tobytes())
    ctx.render_aovs(capi.AOV_ALL)
    ctx.hold_history()
    ctx.reproject()
    assert _code(ctx.merge_history) == 4
    # the mode and the image
    ctx.hold_history()
    ctx.set_mean_by_count(False)
    assert _code(ctx.merge_history) == 4 and _code(ctx.hold_history) == 4
    ctx.set_mean_by_count(True)
    ctx.merge_history()
    ctx.hold_history()
    ctx.set_moments(False)
    assert _code(ctx.merge_history) == 4 and _code(ctx.hold_history) == 4
    ctx.set_moments(True)
    ctx.set_mean_by_count(True)
    assert _code(ctx.merge_history) == 4          # (dropped with the moments image)
    # before resize; a rank of a tile split; a device group
    with capi.Context(0) as c:
        c.set_moments(True)
        c.set_mean_by_count(True)
        assert _code(c.hold_history) == 4 and _code(c.merge_history) == 4
        c.set_tile(0, 2, 8)
        pc.upload_scene(c, demo, env)
        c.resize(w, h)
        assert _code(c.hold_history) == 4 and _code(c.merge_history) == 4
    with capi.Context(devices=[0, 0]) as g:
        g.set_moments(True)
        g.set_mean_by_count(True)
        pc.upload_scene(g, demo, env)
        g.resize(w, h)
        assert _code(g.hold_history) == 4 and _code(g.merge_history) == 4


def test_the_pass_is_timed(ctx, demo, env):
    w, h = SIZES[0]
    tgr._configure(ctx, demo, env, w, h)
    ctx.enable_timing(True)
    try:
        assert _code(lambda: ctx.pass_time_us(capi.PASS_HISTORY)) == 4
        _case(ctx, w, h, radius=1)
        assert ctx.pass_time_us(capi.PASS_HISTORY) > 0
    finally:
        ctx.enable_timing(False)
