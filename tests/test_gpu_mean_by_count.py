"""The mean by count on the GPU (mi3pt_set_mean_by_count): the by-count twins of the two accumulate kernels against the DEFAULT law run
with accumulate frames 1 .. N on the same context -- bit for bit, mean and moments (ptcommon.same_bits, no tolerance anywhere) -- and,
where the two laws part (a tile thawed under a sample mask), against the numpy restatement tests/reproject_reference.py.  Past the grid
caps of the two callers of k_accumulate_frames (2048 and 4096 blocks), where the kernel strides, the restatement is applied to the
oracle's frames."""
import ctypes

import numpy as np
import pytest

import moments_edge_cases as ec
import moments_reference as mr
import ptcommon as pc
import reproject_reference as rr
from mi3pt_host import capi

pytestmark = pytest.mark.gpu
RT, ACC = capi.SUBMIT_RAYTRACE, capi.SUBMIT_ACCUMULATE
TEX = capi.TEX_ACCUMULATION
F = np.float32
SIZES = [(64, 48), (50, 37)]
N = 12


@pytest.fixture(scope="module")
def ctx(built):
    """A context of this module's own: the session's shared one never opts into the moments image or the mode"""
    c = capi.Context(0)
    yield c
    c.close()


def _configure(c, sc, env, w, h, f16=False, variant=0, pipelining=True):
    c.set_tile(0, 1, 8)
    c.set_kernel_variant(variant)
    c.set_pipelining(pipelining)
    c.set_storage(capi.STORAGE_F16 if f16 else capi.STORAGE_F32)
    c.set_moments(True)
    pc.upload_scene(c, sc, env)
    c.resize(w, h)


def _restore(c):
    c.set_mean_by_count(False)
    c.set_kernel_variant(0)
    c.set_pipelining(True)
    c.set_storage(capi.STORAGE_F32)


def _frames(c, sc, w, h, rt_first, acc_first, n, how):
    """n frames: raytrace frames rt_first .., accumulate frames acc_first ..; "frames": one submit_frames (queued where the context
    queues); "split": a RAYTRACE submit and an ACCUMULATE-only submit per frame"""
    if how == "frames":
        c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=rt_first, bounces=4).tobytes())
        c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, acc_first).tobytes())
        c.submit_frames(RT | ACC, n)
        return
    for k in range(n):
        c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=rt_first + k, bounces=4).tobytes())
        c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, acc_first + k).tobytes())
        c.submit(RT)
        c.submit(ACC)


def _snap(c):
    return c.read_texture(TEX), c.read_moments()


def _same(got, want, what):
    assert pc.same_bits(got[0], want[0]), f"{what}: mean: " + pc.describe_diff(got[0], want[0])
    assert pc.same_bits(got[1], want[1]), f"{what}: moments: " + pc.describe_diff(got[1], want[1])


def _both_laws(c, sc, w, h, how, mask=False, chunks=(N,)):
    """the default law with accumulate frames 1 .. N, then the mode with accumulate frames that are anything but (they do not enter)"""
    out = []
    for by_count, acc_first in ((False, 1), (True, 1000)):
        c.set_mean_by_count(by_count)
        c.reset()
        if mask:
            c.set_sample_mask(np.ones(((h + 7) // 8, (w + 7) // 8), np.uint8))
        done = 0
        for n in chunks:
            _frames(c, sc, w, h, 2 + done, acc_first + done, n, how)
            done += n
        out.append(_snap(c))
    return out


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("how", ["queued", "queued in chunks", "split", "unpipelined", "mask queued", "mask split"])
def test_by_count_equals_the_default_law_with_frames_one_to_n(ctx, demo, env, how, f16):
    try:
        for w, h in SIZES:
            _configure(ctx, demo, env, w, h, f16=f16, pipelining=how != "unpipelined")
            default, counted = _both_laws(ctx, demo, w, h, "split" if "split" in how else "frames", mask="mask" in how,
                                          chunks=(5, 1, 6) if "chunks" in how else (N,))
            assert np.all(default[1][..., 3] == N) and default[0][..., :3].any()
            _same(counted, default, f"{how}, {w} x {h}")
    finally:
        _restore(ctx)


@pytest.mark.parametrize("variant", [1, 9, 14])
def test_by_count_on_other_kernel_variants(ctx, demo, env, variant):
    """(1: the per-pixel kernel, which runs its two passes unfused while moments are on)"""
    try:
        w, h = SIZES[1]
        _configure(ctx, demo, env, w, h, variant=variant)
        for how in ("frames", "split"):
            default, counted = _both_laws(ctx, demo, w, h, how)
            assert np.all(default[1][..., 3] == N)
            _same(counted, default, f"variant {variant}, {how}")
    finally:
        _restore(ctx)


CAP_CASES = {
    # the accumulate-only path of mi3pt_submit launches at most 2048 blocks of 256: 1024 x 520 is 2080
    "accumulate-only-1024x520": (1024, 520, 2048, "split", False),
    # the batched path at most 4096: 1024 x 1032 is 4128
    "batched-f32-1024x1032": (1024, 1032, 4096, "frames", False),
    "batched-f16-1024x1032": (1024, 1032, 4096, "frames", True),
}


@pytest.mark.parametrize("case", list(CAP_CASES))
def test_one_row_of_blocks_past_each_grid_cap(ctx, orc, demo, env, case):
    """The by-count kernel where it strides: three frames at two bounces, at the smallest sizes of 1024 columns whose block count
    exceeds each caller's cap, so the last 32 blocks' texels are the second iteration of 8192 threads.  Against the numpy law
    (reproject_reference.by_count_step) applied frame by frame to the ORACLE's radiance (moments_reference.oracle_steps: 0.5 - 0.7 s for
    the three frames; the device's per-frame image is pinned to it elsewhere).  With raytrace frames 1 .. 3 the law's mean is also the
    oracle's own running mean: asserted on the reference.  The accumulate block's frame numbers (1000 ..) do not enter."""
    w, h, cap, how, f16 = CAP_CASES[case]
    frames = 3
    assert cap * 256 < w * h <= 2 * cap * 256
    want_mean, want_m, radiance, _ = mr.oracle_steps(orc, pc.oracle_scene(orc, demo, env), [(f, f, 1) for f in range(1, frames + 1)], w, h,
                                                     lambda f: pc.rt_uniforms(demo, w, h, frame=f, bounces=2).tobytes(),
                                                     lambda f, e: pc.acc_uniforms(w, h, f, e).tobytes(), store_f16=f16)
    mean, moments = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    for k in range(frames):
        mean, moments = rr.by_count_step(mean, moments, radiance[k], store_f16=f16)
    assert pc.same_bits(mean, want_mean) and pc.same_bits(moments, want_m)
    strided = moments.reshape(-1, 4)[cap * 256:]
    spread = (strided[:, :3] != 0).any(axis=1)
    print(f"{case}: {len(strided)} strided texels, {spread.mean():.4f} of them with a non-zero M2")
    assert np.all(strided[:, 3] == frames) and spread.mean() > 0.5       # (measured on the CPU: 1.00 in F32, 0.91 in F16)
    try:
        _configure(ctx, demo, env, w, h, f16=f16)
        ctx.set_mean_by_count(True)
        ctx.reset()
        for k in range(1 if how == "frames" else frames):
            ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=1 + k, bounces=2).tobytes())
            ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1000 + k).tobytes())
            if how == "frames":
                ctx.submit_frames(RT | ACC, frames)
            else:
                ctx.submit(RT)
                ctx.submit(ACC)
        _same(_snap(ctx), (mean, moments), case)
    finally:
        _restore(ctx)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_a_thawed_tile_continues_as_a_sample_mean(ctx, demo, env, f16):
    """frames 1 .. 4 everywhere, 5 .. 8 with the left half of the tiles frozen, 9 .. 12 everywhere again: the numpy law bit for bit, on the
    queued and on the immediate path; the default law's result differs in the thawed half and nowhere else"""
    try:
        w, h = SIZES[1]
        _configure(ctx, demo, env, w, h, f16=f16)
        ty, tx = (h + 7) // 8, (w + 7) // 8
        half = np.ones((ty, tx), np.uint8)
        half[:, :tx // 2] = 0
        sampled = np.repeat(np.repeat(half != 0, 8, axis=0), 8, axis=1)[:h, :w]
        # the radiance of every frame, and the default law's run
        ctx.set_mean_by_count(False)
        ctx.reset()
        radiance = []
        for k in range(N):
            if k in (4, 8):
                ctx.set_sample_mask(half if k == 4 else None)
            ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=2 + k, bounces=4).tobytes())
            ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1 + k).tobytes())
            ctx.submit(RT)
            radiance.append(ctx.read_texture(capi.TEX_OUTPUT))
            ctx.submit(ACC)
        default = _snap(ctx)
        mean, moments = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
        for k in range(N):
            mean, moments = rr.by_count_step(mean, moments, radiance[k], store_f16=f16, inside=sampled if 4 <= k < 8 else None)
        assert np.all(moments[..., 3] == np.where(sampled, 12, 8))
        ctx.set_mean_by_count(True)
        for how in ("frames", "split"):
            ctx.reset()
            for first, n, m in ((0, 4, "keep"), (4, 4, half), (8, 4, None)):
                if not isinstance(m, str):
                    ctx.set_sample_mask(m)
                _frames(ctx, demo, w, h, 2 + first, 1 + first, n, how)
            _same(_snap(ctx), (mean, moments), f"{how}, f16 {f16}")
        assert pc.same_bits(default[0][sampled], mean[sampled]) and pc.same_bits(default[1][sampled], moments[sampled])
        assert not pc.same_bits(default[0][~sampled], mean[~sampled])
    finally:
        _restore(ctx)


_radiance = {}


def _four_frames(c, sc, w, h, f16):
    """the radiance of raytrace frames 2 .. 5 at two bounces, read from TEX_OUTPUT after a RAYTRACE-only submit (once per storage format)"""
    if f16 not in _radiance:
        frames = []
        for k in range(4):
            c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2 + k, bounces=2).tobytes())
            c.submit(RT)
            frames.append(c.read_texture(capi.TEX_OUTPUT))
        _radiance[f16] = frames
    return _radiance[f16]


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("how", ["queued", "split", "mask of ones", "half mask"])
def test_written_counts(ctx, demo, env, how, f16):
    """Per-texel heterogeneous counts, as mi3pt_reproject and mi3pt_write_moments leave them, against the numpy law: the whole catalogue of
    tests/moments_edge_cases.py written with write_texture + write_moments at 50 x 37 (on both sides of every 256th texel, where
    k_accumulate_frames' blocks meet, and of the 8 x 8 tile seams, where k_accumulate_tiles' waves do), then four frames at two bounces on
    k_accumulate_frames' batched route, on the ACCUMULATE-only submit, and under an all-ones and a half sample mask (k_accumulate_tiles).
    reproject_reference.by_count_step applied to the frames' radiance; NaN, negative, zero and fractional counts below 1 restart, 1.5
    continues, 2^24 and beyond stop growing.  Every texel, ptcommon.same_bits_or_nan; a frozen tile keeps its bits exactly"""
    try:
        w, h = SIZES[1]
        _configure(ctx, demo, env, w, h, f16=f16)
        ctx.set_mean_by_count(True)
        ctx.reset()
        radiance = _four_frames(ctx, demo, w, h, f16)
        mean, moments, where = ec.placed(w, h, 5, finite=False, linear=256)
        assert not ec.seam_sides(where, w, h)
        ctx.reset()
        ctx.write_texture(TEX, mean)
        ctx.write_moments(moments)
        mean, moments = _snap(ctx)
        start = mean.copy(), moments.copy()
        ty, tx = (h + 7) // 8, (w + 7) // 8
        mask = np.ones((ty, tx), np.uint8)
        if how == "half mask":
            mask[:, :tx // 2] = 0
        sampled = np.repeat(np.repeat(mask != 0, 8, axis=0), 8, axis=1)[:h, :w]
        if "mask" in how:
            ctx.set_sample_mask(mask)
        restarts = ~(moments[..., 3] >= 1) & sampled
        for k in range(4):
            mean, moments = rr.by_count_step(mean, moments, radiance[k], store_f16=f16, inside=sampled)
        n0, n4 = start[1][..., 3], moments[..., 3]
        print(f"{how}, f16 {f16}: {int(restarts.sum())} texels restart, {int((sampled & ~restarts).sum())} continue, "
              f"{int((sampled & ~restarts & (n4 == n0)).sum())} of those with a count that no longer grows; NaN in "
              f"{float(np.isnan(mean).any(axis=-1).mean()):.3f} of the mean's texels")
        assert restarts.any() and np.all(n4[restarts] == 4) and (sampled & ~restarts & (n4 == n0)).any() and (n4 == F(5.5)).any()
        if how == "split":
            for k in range(4):
                ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=2 + k, bounces=2).tobytes())
                ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1000 + k).tobytes())
                ctx.submit(RT)
                ctx.submit(ACC)
        else:
            ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=2, bounces=2).tobytes())
            ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1000).tobytes())
            ctx.submit_frames(RT | ACC, 4)
        got = _snap(ctx)
        pc.assert_same_or_nan(got, (mean, moments), f"{how}, f16 {f16}")
        for g, s in zip(got, start):
            assert np.array_equal(g[~sampled].view(np.uint32), s[~sampled].view(np.uint32))
    finally:
        _restore(ctx)


def test_the_mode_switches_off_again_and_leaves_the_default_bits(ctx, demo, env):
    try:
        w, h = SIZES[1]
        _configure(ctx, demo, env, w, h)
        ctx.reset()
        _frames(ctx, demo, w, h, 2, 2, N, "frames")          # the hosts' frames: 2, 3, ...
        want = _snap(ctx)
        ctx.set_mean_by_count(True)
        ctx.reset()
        _frames(ctx, demo, w, h, 2, 2, N, "frames")
        counted = _snap(ctx)
        assert not pc.same_bits(counted[0], want[0])          # the sample mean: brighter by (N + 1) / N
        lit = (want[0][..., :3] > 0.01).all(axis=-1)
        assert np.allclose(counted[0][lit][:, :3] / np.maximum(want[0][lit][:, :3], 1e-6), (N + 1) / N, rtol=1e-4)
        ctx.set_mean_by_count(False)
        ctx.reset()
        _frames(ctx, demo, w, h, 2, 2, N, "frames")
        _same(_snap(ctx), want, "enabled, then disabled")
        # mi3pt_set_moments(0) switches the mode off with the image
        ctx.set_mean_by_count(True)
        ctx.set_moments(False)
        ctx.set_moments(True)
        ctx.reset()
        _frames(ctx, demo, w, h, 2, 2, N, "frames")
        _same(_snap(ctx), want, "moments off and on again")
    finally:
        _restore(ctx)


def test_error_codes(built):
    lib = capi.load_library()
    assert lib.mi3pt_set_mean_by_count(None, 1) == 1
    with capi.Context(0) as c:
        with pytest.raises(capi.Mi3ptError) as e:
            c.set_mean_by_count(True)
        assert e.value.code == 4 and "mi3pt_set_moments" in e.value.message
        c.set_mean_by_count(False)                            # switching off needs nothing
        c.set_moments(True)
        c.set_mean_by_count(True)                             # before mi3pt_resize: the image comes with the textures
        c.set_moments(False)
        with pytest.raises(capi.Mi3ptError) as e:
            c.set_mean_by_count(True)
        assert e.value.code == 4
