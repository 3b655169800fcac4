"""Adaptive sampling on the GPU (mi3pt_set_sample_mask, mi3pt_freeze_converged, renderUntil(adaptive=True)).

Every expectation but two is built from an UNMASKED run of the unchanged kernels on the same context settings: snapshots of the mean and
the moments after each chunk of frames, put together per tile by adaptive_reference.composite -- "every texel equals the unmasked run's
texel after the last frame its tile was sampled in" -- and compared bit for bit (ptcommon.same_bits), no tolerance anywhere.  The two:
one direct comparison with the oracle, and the end-to-end run against the loop replayed on the oracle with the numpy restatement."""
import ctypes

import numpy as np
import pytest

import adaptive_reference as ar
import convergence_reference as cr
import moments_reference as mr
import ptcommon as pc
from mi3pt_host import capi

pytestmark = pytest.mark.gpu
RT, ACC = capi.SUBMIT_RAYTRACE, capi.SUBMIT_ACCUMULATE
MASK = RT | ACC
TEX = capi.TEX_ACCUMULATION
F = np.float32
_cache = {}


@pytest.fixture(scope="module")
def ctx(built):
    """A context of this module's own: the session's shared one never opts into the moments image or a mask"""
    c = capi.Context(0)
    yield c
    c.close()


def _configure(c, sc, env, w, h, f16=False, moments=True, variant=0, tile=(0, 1, 8), pipelining=True):
    c.set_tile(*tile)
    c.set_kernel_variant(variant)
    c.set_pipelining(pipelining)
    c.set_storage(capi.STORAGE_F16 if f16 else capi.STORAGE_F32)
    c.set_moments(moments)
    pc.upload_scene(c, sc, env)
    c.resize(w, h)


def _restore(c):
    c.set_tile(0, 1, 8)
    c.set_kernel_variant(0)
    c.set_pipelining(True)
    c.set_storage(capi.STORAGE_F32)


def _chunk(c, sc, w, h, first, n, how="frames", rect=None):
    """n frames numbered first, first + 1, ...; how "frames": submit_frames (queued wherever the context queues); "split": a RAYTRACE
    submit and an ACCUMULATE-only submit per frame.  rect: the accumulate block's resolution (smaller than the image: never queued)"""
    rw, rh = rect or (w, h)
    if how == "frames":
        c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=first, bounces=4).tobytes())
        c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(rw, rh, first).tobytes())
        c.submit_frames(MASK, n)
        return
    for f in range(first, first + n):
        c.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=f, bounces=4).tobytes())
        c.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(rw, rh, f).tobytes())
        c.submit(RT)
        c.submit(ACC)


def _snap(c, moments=True):
    return c.read_texture(TEX), (c.read_moments() if moments else None)


def _unmasked(c, sc, w, h, first, chunks, moments=True, **kw):
    """snapshots[k] = (mean, moments) after chunk k of a run without a mask, k = 0 before the first"""
    c.reset()
    snaps = [_snap(c, moments)]
    for n in chunks:
        _chunk(c, sc, w, h, first, n, **kw)
        first += n
        snaps.append(_snap(c, moments))
    return snaps


def _masked(c, sc, w, h, first, chunks, masks, moments=True, **kw):
    """The same run with masks[k] set in front of chunk k (None: the mask is left as it is).  Returns (snapshot, last): last[tile] = the
    last chunk (1-based) the tile was sampled in, 0 = never"""
    c.reset()
    shape = ((c.local_rows + 7) // 8, (w + 7) // 8)
    cur = np.ones(shape, bool)
    last = np.zeros(shape, np.int64)
    for k, (n, m) in enumerate(zip(chunks, masks)):
        if m is not None:
            c.set_sample_mask(m)
            cur = np.asarray(m).reshape(shape) != 0
        _chunk(c, sc, w, h, first, n, **kw)
        first += n
        last[cur] = k + 1
    return _snap(c, moments), last


def _held(got, snaps, last, what):
    want = ar.composite([s[0] for s in snaps], last)
    assert pc.same_bits(got[0], want), f"{what}: mean: " + pc.describe_diff(got[0], want)
    if got[1] is not None:
        want = ar.composite([s[1] for s in snaps], last)
        assert pc.same_bits(got[1], want), f"{what}: moments: " + pc.describe_diff(got[1], want)


def _masks(ty, tx):
    """The masks of the issue, by name, for a ty x tx map"""
    one = lambda y, x, v: np.where((np.arange(ty)[:, None] == y) & (np.arange(tx)[None, :] == x), v, 1 - v).astype(np.uint8)
    out = {"zero": np.zeros((ty, tx), np.uint8), "one": np.ones((ty, tx), np.uint8),
           "one sampled": one(ty // 2, tx // 2, 1), "one frozen": one(ty - 1, 0, 0),
           "checkerboard": ((np.arange(ty)[:, None] + np.arange(tx)[None, :]) % 2).astype(np.uint8),
           "right": np.zeros((ty, tx), np.uint8), "bottom": np.zeros((ty, tx), np.uint8)}
    out["right"][:, -1] = 1
    out["bottom"][-1, :] = 1
    return out


SIZES = [(1, 1), (7, 5), (8, 8), (9, 17), (100, 52)]


@pytest.mark.parametrize("w,h", SIZES)
def test_masked_mean_kernel_edges(ctx, demo, env, w, h):
    """Two chunks, a mask set between them: every mask of the issue at 4 + 4 frames from frame 2; then 1 + 1, 5 + 5 (the unroll's
    remainder) and 4 + 5 frames, from frame 1 (a step of weight 1) and 2, under the two masks that mix tiles; then a mask from the start
    (frozen tiles stay zero, the restart at frame 1 runs inside the masked run) narrowed between the chunks"""
    _configure(ctx, demo, env, w, h)
    masks = _masks((h + 7) // 8, (w + 7) // 8)
    snaps = _unmasked(ctx, demo, w, h, 2, (4, 4))
    assert snaps[2][0][..., :3].any() and not pc.same_bits(snaps[1][0], snaps[2][0])           # (the chunks do change the image)
    for name, m in masks.items():
        got, last = _masked(ctx, demo, w, h, 2, (4, 4), (None, m))
        _held(got, snaps, last, f"{w} x {h}, mask {name}")
        assert np.array_equal(ctx.read_sample_mask(), m)
    for chunks in ((1, 1), (5, 5), (4, 5)):
        for first in (1, 2):
            snaps = _unmasked(ctx, demo, w, h, first, chunks)
            for name in ("checkerboard", "one frozen"):
                got, last = _masked(ctx, demo, w, h, first, chunks, (None, masks[name]))
                _held(got, snaps, last, f"{w} x {h}, mask {name}, frames {chunks} from {first}")
            both = masks["checkerboard"] & masks["one frozen"]
            got, last = _masked(ctx, demo, w, h, first, chunks, (masks["checkerboard"], both))
            assert (last == 0).any() or both.all()
            _held(got, snaps, last, f"{w} x {h}, masked from the start, frames {chunks} from {first}")


def _hip():
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        import os
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    return hip


@pytest.mark.parametrize("how", ["F16", "bound", "no moments", "F16 no moments"])
@pytest.mark.parametrize("w,h", [(9, 17), (100, 52)])
def test_storage_and_moments(ctx, demo, env, w, h, how):
    f16, moments = "F16" in how, "no moments" not in how
    _configure(ctx, demo, env, w, h, f16=f16, moments=moments)
    hip, bound = None, ctypes.c_void_p()
    if how == "bound":      # a caller-owned image (the HIP runtime the library has loaded)
        hip = _hip()
        nbytes = h * w * 16
        assert hip.hipMalloc(ctypes.byref(bound), nbytes) == 0 and hip.hipMemset(bound, 0, nbytes) == 0
        assert hip.hipDeviceSynchronize() == 0
        ctx.bind_accumulation(bound.value, nbytes)
    try:
        masks = _masks((h + 7) // 8, (w + 7) // 8)
        for first in (1, 2):
            snaps = _unmasked(ctx, demo, w, h, first, (4, 5), moments=moments)
            for name in ("checkerboard", "one frozen", "right", "bottom"):
                got, last = _masked(ctx, demo, w, h, first, (4, 5), (None, masks[name]), moments=moments)
                _held(got, snaps, last, f"{how}, {w} x {h}, mask {name}, from {first}")
    finally:
        if hip is not None:
            ctx.bind_accumulation(None, 0)
            hip.hipFree(bound)
        ctx.set_moments(True)
        _restore(ctx)


@pytest.mark.parametrize("w,h,rect", [(9, 17, (5, 9)), (100, 52, (61, 37)), (100, 52, (100, 20))])
def test_an_accumulate_rectangle_smaller_than_the_image(ctx, demo, env, w, h, rect):
    """(such frames are never queued: the immediate path of mi3pt_submit under a mask)"""
    _configure(ctx, demo, env, w, h)
    masks = _masks((h + 7) // 8, (w + 7) // 8)
    snaps = _unmasked(ctx, demo, w, h, 1, (3, 3), rect=rect)
    assert not snaps[2][0][rect[1]:].any() and not snaps[2][0][:, rect[0]:].any() and snaps[2][0][:rect[1], :rect[0], :3].any()
    for name in ("checkerboard", "one frozen", "zero", "right"):
        got, last = _masked(ctx, demo, w, h, 1, (3, 3), (None, masks[name]), rect=rect)
        _held(got, snaps, last, f"{w} x {h}, rectangle {rect}, mask {name}")


@pytest.mark.parametrize("block_rows", [4, 8])
def test_a_rank_of_a_tile_split(ctx, demo, env, block_rows):
    """Rank 1 of 2, 100 x 52: with block_rows 4 the eight local rows of a tile are two blocks of the image, not eight consecutive rows"""
    w, h = 100, 52
    try:
        _configure(ctx, demo, env, w, h, tile=(1, 2, block_rows))
        rows = ctx.local_rows
        assert 0 < rows < h
        masks = _masks((rows + 7) // 8, (w + 7) // 8)
        for chunks in ((4, 5), (8, 8)):              # (8 frames: the empty tiles of the view leave the job list)
            snaps = _unmasked(ctx, demo, w, h, 2, chunks)
            for name in ("checkerboard", "one frozen", "bottom", "one sampled"):
                got, last = _masked(ctx, demo, w, h, 2, chunks, (None, masks[name]))
                _held(got, snaps, last, f"rank 1 of 2, block_rows {block_rows}, mask {name}, frames {chunks}")
    finally:
        _restore(ctx)


def test_every_route_gives_the_same_image(ctx, demo, env):
    """The shipped variant's unmasked snapshots are the expectation; the masked run equals their composite with the shipped variant
    (the job list carries the mask), variant 7 (every tile traced, the mean masked) and variant 1 (the per-pixel kernels, unfused under a
    mask), pipelined and not, and with RAYTRACE and ACCUMULATE submitted separately"""
    w, h = 100, 52
    masks = _masks(7, 13)
    try:
        _configure(ctx, demo, env, w, h)
        snaps = _unmasked(ctx, demo, w, h, 2, (8, 8))
        variants = pc.variants_available(ctx, (0, 7, 1))
        assert 0 in variants
        for variant in variants:
            for pipelining in (True, False):
                for how in ("frames", "split"):
                    _configure(ctx, demo, env, w, h, variant=variant, pipelining=pipelining)
                    for name in ("checkerboard", "bottom", "one frozen"):
                        got, last = _masked(ctx, demo, w, h, 2, (8, 8), (None, masks[name]), how=how)
                        _held(got, snaps, last, f"variant {variant}, pipelining {pipelining}, {how}, mask {name}")
    finally:
        _restore(ctx)


def _counted(c, sc, w, h, first, n, mask):
    """counter deltas and the last launch of n queued frames under `mask`, after reset"""
    c.reset()
    if mask is not None:
        c.set_sample_mask(mask)
    c.reset_counters()
    _chunk(c, sc, w, h, first, n)
    cnt = c.counters()
    return {k: cnt[k] for k in ("pixels", "rays", "misses", "hits")}, c.last_launch()


def test_the_saving_is_real(ctx, demo, env):
    """64 x 64, 8 frames per launch (the sky split is on), shipped variant.  The per-tile truth: the launch under each single-tile mask;
    the 64 of them add up to the unmasked launch, and a launch under any mask counts the sum of its tiles.  The grid follows the jobs."""
    w = h = 64
    n = 8
    _configure(ctx, demo, env, w, h)
    empty = capi.host_sky_tiles(demo.nodes, pc.rt_uniforms(demo, w, h, frame=2, bounces=4).tobytes(), w, h) != 0
    assert 0 < empty.sum() < 32                                        # (the demo's top band is sky)
    whole, launch = _counted(ctx, demo, w, h, 2, n, None)
    assert launch["kind"] == 1 and launch["lean"] and 9 <= launch["variant"] <= 14
    assert launch["workgroups"] == n * int((~empty).sum())             # one wave per job: the empty tiles are not jobs
    assert whole["pixels"] == n * w * h
    per_tile = {}
    for t in range(64):
        m = np.zeros(64, np.uint8)
        m[t] = 1
        per_tile[t], one = _counted(ctx, demo, w, h, 2, n, m.reshape(8, 8))
        assert per_tile[t]["pixels"] == n * 64
        assert one["workgroups"] == n                                  # one tile, n jobs -- an empty one is then the job list
        if empty.reshape(-1)[t]:
            assert per_tile[t]["rays"] == per_tile[t]["misses"] == n * 64 and per_tile[t]["hits"] == 0
    total = {k: sum(p[k] for p in per_tile.values()) for k in whole}
    assert total == whole, f"the single-tile launches add up to {total}, the unmasked launch counted {whole}"
    masks = _masks(8, 8)
    masks["sky"] = empty.astype(np.uint8)                              # every sampled tile is sky
    masks["sky and one"] = masks["sky"] | masks["one sampled"]
    for name, m in masks.items():
        got, launch = _counted(ctx, demo, w, h, 2, n, m)
        tiles = np.flatnonzero(m.reshape(-1))
        want = {k: sum(per_tile[t][k] for t in tiles) for k in whole}
        assert got == want, f"mask {name}: counted {got}, its tiles add up to {want}"
        a, s = ar.compose_lists(m, empty)
        if name == "zero":
            continue
        jobs = len(a) if len(a) else len(s)
        assert launch["workgroups"] == n * jobs, f"mask {name}: {launch}, {len(a)} traced + {len(s)} sky tiles"
    # no tile sampled: nothing ran, the counters stand still -- and the next launches, masked and unmasked after a reset, still run
    ctx.reset()
    ctx.set_sample_mask(masks["zero"])
    ctx.reset_counters()
    for first in (2, 10, 18):
        _chunk(ctx, demo, w, h, first, n)
        ctx.flush()
    assert not any(ctx.counters().values()) and not ctx.read_texture(TEX).any()
    ctx.set_sample_mask(masks["one sampled"])
    _chunk(ctx, demo, w, h, 26, n)
    assert ctx.counters()["pixels"] == n * 64
    again, launch = _counted(ctx, demo, w, h, 2, n, None)
    assert again == whole and launch["workgroups"] == n * int((~empty).sum())
    assert pc.same_bits(ctx.read_texture(TEX), _unmasked(ctx, demo, w, h, 2, (n,))[1][0])


def test_no_mask_nothing_changes(ctx, demo, env):
    """After set_sample_mask(None), and after reset, counters, last launch, image and moments equal a fresh context's"""
    w, h = 100, 52

    def run(c, prepare):
        _configure(c, demo, env, w, h)
        prepare(c)
        c.reset_counters()
        _chunk(c, demo, w, h, 2, 8)
        _chunk(c, demo, w, h, 10, 3)
        # (the path counters: the shipped walk's box and triangle tests depend on which jobs share a wave, and differ from run to run)
        cnt = c.counters()
        return {k: cnt[k] for k in pc.PATH_COUNTERS}, c.last_launch(), c.read_texture(TEX).tobytes(), c.read_moments().tobytes()

    with capi.Context(0) as fresh:
        want = run(fresh, lambda c: None)
    checker = _masks(7, 13)["checkerboard"]

    def masked_then_cleared(c):
        c.set_sample_mask(checker)
        _chunk(c, demo, w, h, 2, 8)
        c.set_sample_mask(None)
        assert c.read_sample_mask().all()
        c.reset()

    def masked_then_reset(c):
        c.set_sample_mask(checker)
        _chunk(c, demo, w, h, 2, 8)
        c.reset()
        assert c.read_sample_mask().all()

    def masked_then_resized(c):
        c.set_sample_mask(checker)
        c.resize(w, h)
        assert c.read_sample_mask().all()

    for prepare in (masked_then_cleared, masked_then_reset, masked_then_resized):
        got = run(ctx, prepare)
        assert got[:2] == want[:2], f"{prepare.__name__}: {got[:2]} != {want[:2]}"
        assert got[2] == want[2] and got[3] == want[3], prepare.__name__
    # write_texture, bind_accumulation(None) and set_moments leave the mask
    ctx.set_sample_mask(checker)
    ctx.write_texture(TEX, np.zeros((h, w, 4), F))
    ctx.bind_accumulation(None, 0)
    ctx.set_moments(True)
    assert np.array_equal(ctx.read_sample_mask(), checker)
    ctx.reset()


def _oracle(orc, sc, env, w, h, frames, first=1):
    """The oracle's mean and the reference's moments after each of `frames` frames (frame numbers first, first + 1, ...), bounces 4"""
    key = (sc.name, w, h, frames, first)
    if key not in _cache:
        osc = pc.oracle_scene(orc, sc, env)
        mean, m, out = None, None, []
        for f in range(first, first + frames):
            mean, m, _, _ = mr.oracle_steps(orc, osc, [(f, f, 1)], w, h, lambda k: pc.rt_uniforms(sc, w, h, frame=k, bounces=4).tobytes(),
                                            lambda k, e: pc.acc_uniforms(w, h, k, e).tobytes(), mean=mean, moments=m)
            out.append((mean, m))
        _cache[key] = out
    return _cache[key]


def test_the_oracle_directly(ctx, orc, demo, env):
    """40 x 24, six frames, the mask set after three: frozen tiles hold the oracle's mean and the reference's moments after 3 frames, the
    others after 6"""
    w, h = 40, 24
    steps = _oracle(orc, demo, env, w, h, 6)
    _configure(ctx, demo, env, w, h)
    m = _masks(3, 5)["checkerboard"]
    got, last = _masked(ctx, demo, w, h, 1, (3, 3), (None, m))
    sel = ar.tile_texels(m, h, w)
    for k, name in ((0, "mean"), (1, "moments")):
        want = np.where(sel[..., None], steps[5][k], steps[2][k])
        assert pc.same_bits(got[k], want), f"{name}: " + pc.describe_diff(got[k], want)
    assert not pc.same_bits(steps[5][0], steps[2][0])


def _code(fn, *a):
    with pytest.raises(capi.Mi3ptError) as e:
        fn(*a)
    return e.value.code


@pytest.mark.parametrize("guard", [0, 1])
def test_freeze_converged(ctx, demo, env, guard):
    """Equals the restatement applied to read_convergence_tiles and the mask so far, check after check; the threshold is the median of
    the tiles' own error, so both verdicts occur"""
    w, h = 100, 52
    _configure(ctx, demo, env, w, h)
    ctx.reset()
    _chunk(ctx, demo, w, h, 2, 8)
    ctx.estimate_convergence(0.0, 0)
    tiles = ctx.read_convergence_tiles()
    threshold = float(np.sqrt(np.median(tiles[..., 0] / tiles[..., 2]) / 3.0))
    mask = None
    seen = []
    for check in range(3):
        ctx.estimate_convergence(threshold, 4)
        tiles = ctx.read_convergence_tiles()
        want, want_left = ar.freeze_tiles(tiles, threshold, 4, guard, mask)
        left = ctx.freeze_converged(guard)
        got = ctx.read_sample_mask()
        assert left == want_left and np.array_equal(got, want), f"check {check}: {left} tiles left, the restatement leaves {want_left}"
        mask = got
        seen.append(left)
        _chunk(ctx, demo, w, h, 10 + 8 * check, 8)
    print(f"guard {guard}: threshold {threshold:.5f}, tiles left {seen} of {tiles.shape[0] * tiles.shape[1]}")
    assert 0 < seen[0] < tiles.shape[0] * tiles.shape[1]
    ctx.reset()


def test_error_table(built):
    with capi.Context(0) as c:
        ones = np.ones((2, 3), np.uint8)
        assert _code(c.set_sample_mask, ones) == 4 and _code(c.set_sample_mask, None) == 4           # before resize
        c.local_rows, c.width = 12, 20                                                                 # (the wrapper's shape only)
        assert _code(c.read_sample_mask) == 4 and _code(c.freeze_converged, 1) == 4
        c.set_moments(True)
        c.resize(20, 12)
        assert _code(c.freeze_converged, 1) == 4 and _code(c.freeze_converged, 0) == 4                # no estimate yet
        assert _code(c.freeze_converged, 2) == 1 and _code(c.freeze_converged, -1) == 1
        assert c.read_sample_mask().tolist() == [[1, 1, 1], [1, 1, 1]]
        p = ones.ctypes.data_as(ctypes.c_void_p)
        n = ctypes.c_uint32(99)
        lib, hd = c.lib, c.handle
        assert lib.mi3pt_set_sample_mask(hd, p, 5) == 1 and lib.mi3pt_set_sample_mask(hd, p, 7) == 1 and lib.mi3pt_set_sample_mask(hd, None, 6) == 1
        assert lib.mi3pt_set_sample_mask(hd, p, 0) == 1
        assert lib.mi3pt_read_sample_mask(hd, p, 5, ctypes.byref(n)) == 1 and lib.mi3pt_read_sample_mask(hd, None, 6, ctypes.byref(n)) == 1
        assert lib.mi3pt_set_sample_mask(hd, p, 6) == 0 and lib.mi3pt_read_sample_mask(hd, p, 6, ctypes.byref(n)) == 0 and n.value == 6
        assert lib.mi3pt_read_sample_mask(hd, p, 6, None) == 0
        c.set_sample_mask([[1, 0, 2], [0, 0, 255]])
        assert c.read_sample_mask().tolist() == [[1, 0, 1], [0, 0, 1]]
        c.estimate_convergence(0.1, 16)
        assert c.freeze_converged(1) == 0 and not c.read_sample_mask().any()                          # zeroed moments: nothing counts, all frozen
        assert _code(c.freeze_converged, 3) == 1
        c.resize(20, 12)                                                                               # a resize drops the mask and the estimate
        assert c.read_sample_mask().all() and _code(c.freeze_converged, 1) == 4
        c.set_sample_mask(None)
    assert capi.load_library().mi3pt_abi_version() == 4


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["two", "three"])
def test_device_group(ctx, demo, env, devices):
    """40 x 28 (a ragged last round), block_rows 8: the whole map in and out, the freeze on the whole map, the image is the single
    context's; block_rows 4: MI3PT_ERR_STATE"""
    w, h = 40, 28
    shape = (4, 5)
    m = _masks(*shape)["checkerboard"]

    def run(c):
        c.set_moments(True)
        pc.upload_scene(c, demo, env)
        c.resize(w, h)
        out = []
        _chunk(c, demo, w, h, 1, 4)
        c.set_sample_mask(m)
        out.append(c.read_sample_mask().copy())
        _chunk(c, demo, w, h, 5, 4)
        c.estimate_convergence(0.0, 0)
        tiles = c.read_convergence_tiles()
        threshold = float(np.sqrt(np.quantile(tiles[..., 0] / tiles[..., 2], 0.85) / 3.0))      # (a few tiles above: the ring bites, not everywhere)
        c.estimate_convergence(threshold, 4)
        left = c.freeze_converged(1)
        out.append(c.read_sample_mask().copy())
        _chunk(c, demo, w, h, 9, 4)
        return out, left, threshold, tiles, c.read_texture(TEX), c.read_moments()

    _restore(ctx)
    single = run(ctx)
    want, want_left = ar.freeze_tiles(single[3], single[2], 4, 1, m)
    assert np.array_equal(single[0][1], want) and single[1] == want_left
    print(f"{want_left} of {int(m.sum())} sampled tiles left; without the ring {ar.freeze_tiles(single[3], single[2], 4, 0, m)[1]}")
    assert 0 < want_left < m.sum(), "the freeze must change the mask and leave something to sample"
    with capi.Context(devices=devices, block_rows=8) as g:
        got = run(g)
        assert got[0][0].shape == shape and np.array_equal(got[0][0], m) and np.array_equal(got[0][1], want) and got[1] == want_left
        assert got[3].tobytes() == single[3].tobytes()
        assert pc.same_bits(got[4], single[4]), pc.describe_diff(got[4], single[4])
        assert pc.same_bits(got[5], single[5]), pc.describe_diff(got[5], single[5])
        members = [g.member(i).read_sample_mask() for i in range(len(devices))]      # each member holds its rows of the map
        for i, mm in enumerate(members):
            rows = [capi.tile_global_row(t, i, len(devices), 1) for t in range(mm.shape[0])]
            assert np.array_equal(mm, want[rows]), f"member {i}"
        g.set_sample_mask(None)
        assert g.read_sample_mask().all()
        g.reset()
    with capi.Context(devices=devices, block_rows=4) as g:
        g.set_moments(True)
        pc.upload_scene(g, demo, env)
        g.resize(w, h)
        _chunk(g, demo, w, h, 1, 4)
        g.estimate_convergence(0.1, 4)
        assert _code(g.set_sample_mask, m) == 4 and _code(g.read_sample_mask) == 4 and _code(g.freeze_converged, 1) == 4
        assert _code(g.set_sample_mask, None) == 4
    ctx.reset()


# ---- renderUntil(adaptive=True) end to end: the Python host on the device against the same loop replayed on the oracle ----
UNTIL = dict(w=64, h=64, check_every=16, max_frames=160, min_frames=16)


def _replay(orc, demo, env):
    """The oracle's (mean, moments) after 1 .. 160 frames as Renderer.render() numbers them (the first sample is frame 2) and the tile
    maps of the unmasked run after 16, 32, ... frames"""
    if "until" not in _cache:
        steps = _oracle(orc, demo, env, UNTIL["w"], UNTIL["h"], UNTIL["max_frames"], first=2)
        _cache["until"] = steps, {n: cr.tile_map(*steps[n - 1]) for n in range(16, UNTIL["max_frames"] + 1, 16)}
    return _cache["until"]


def until_cases():
    return [(0.08, 0, False), (0.08, 1, False), (0.08, 1, True), (0.05, 1, False), (0.05, 1, True)]


@pytest.mark.parametrize("threshold,guard,lookahead", until_cases())
def test_render_until_adaptive_end_to_end(built, orc, demo, env, threshold, guard, lookahead):
    """Same stop frame, same "sampled", same mask, and mean and moments bit-identical to the per-tile composite of the oracle's images.
    Threshold 0.08 converges within the budget; 0.05 does not (the end-of-budget branch)."""
    from mi3pt_host import RaytracingCamera, RaytracingScene, Renderer
    steps, maps = _replay(orc, demo, env)
    want = ar.render_until_adaptive(lambda n: maps[n], (8, 8), threshold, UNTIL["min_frames"], UNTIL["max_frames"], UNTIL["check_every"],
                                    lookahead=lookahead, guard=guard)
    left = [int(m.sum()) for m in want["history"]]
    print(f"threshold {threshold}, guard {guard}, lookahead {lookahead}: the replay stops at {want['frames']}, sampled tiles after each "
          f"decision {left}, {want['sampled'] * 64} texel-samples, converged {want['converged']}")
    # what makes the case worth running, asserted on the replay itself before the device is asked
    frozen_at = [64 - left[0]] + [left[k - 1] - left[k] for k in range(1, len(left))]
    assert sum(1 for f in frozen_at if f > 0) >= 3, "tiles must freeze at three or more different checks"
    assert frozen_at[0] >= 32, "at least half of the tiles must freeze at the first check"
    assert len(left) >= 5 and left[4] > 0, "at least one tile must still be sampled after the fifth check"
    assert want["converged"] == (threshold == 0.08)
    r = Renderer.create()
    try:
        r.scalingFactor = 1
        r.presentEveryFrame = False
        r.setUniforms("raytrace", {"maxBounces": 4, "envMapIntensity": 1.0})
        r.setUniforms("accumulate", {"enabled": 1})
        r.setMoments(True)
        r.resize(UNTIL["w"], UNTIL["h"])
        scene = RaytracingScene(demo, env)
        scene.needsUpdate = True
        events = []
        r.on("converged", lambda s: events.append("converged"))
        r.on("complete", lambda: events.append("complete"))
        out = r.renderUntil(scene, RaytracingCamera(45.0), threshold, minFrames=UNTIL["min_frames"], maxFrames=UNTIL["max_frames"],
                            checkEvery=UNTIL["check_every"], lookahead=lookahead, adaptive=True, guard=guard)
        print({k: v for k, v in out.items() if k != "summary"}, out["summary"])
        assert out["converged"] is want["converged"] and out["frames"] == want["frames"] and out["sampled"] == want["sampled"]
        assert r.frame == want["frames"] + 1 and r.status == "idle"
        assert events == (["converged", "complete"] if want["converged"] and want["frames"] < UNTIL["max_frames"] else ["complete"])
        assert np.array_equal(r.readSampleMask(), want["history"][-1])
        assert cr.same_summary(out["summary"], cr.summary(want["tiles"], threshold, UNTIL["min_frames"]))
        snaps = {n: steps[n - 1] for n in np.unique(want["last"])}
        for k, got in ((0, r.readAccumulation()), (1, r.readMoments())):
            expect = np.zeros_like(got)
            for n, s in snaps.items():
                sel = ar.tile_texels(want["last"] == n, UNTIL["h"], UNTIL["w"])
                expect[sel] = s[k][sel]
            assert pc.same_bits(got, expect), ("mean: ", "moments: ")[k] + pc.describe_diff(got, expect)
        r.reset()                                        # a camera move: the next accumulation starts whole
        assert r.readSampleMask().all()
    finally:
        r.destroy()
