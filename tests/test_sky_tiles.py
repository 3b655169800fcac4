"""The empty tiles of a view (mi3pt_host_sky_tiles, PROOFS.md section 5): 8x8 tiles whose camera rays can reach no geometry are shaded by a
streaming kernel instead of being traced (MI3PT_OPT_SKY_TILES).

CPU: for many seeded exterior cameras, every pixel of every tile the library calls empty renders, in the oracle, exactly as it does
on a scene with nothing in it -- on a copy of the scene whose every material EMITS, so that a single hit anywhere along the path would
show; the conditions under which the set must be empty; the share of empty tiles of the bench views.
GPU: switch on against off, identical image bits and identical path counters."""
import math

import numpy as np
import pytest

import ptcommon
from mi3pt_host import capi, layout, scenes

W, H = 160, 96          # 20 x 12 tiles


def _pixel_mask(empty, w, h):
    return np.kron(empty, np.ones((8, 8), np.uint8))[:h, :w].astype(bool)


def _emitting(sc):
    """The scene with every material emitting: light = light + emission x throughput at every hit (raytrace.wgsl:380-395)."""
    mats = [dict(m, emissive=(1.0, 0.5, 0.25), emissiveIntensity=7.0) for m in sc.materials]
    return layout.pack_materials(mats)


def _nothing(orc, env):
    """A scene with nothing in view: no BVH at all, every ray misses."""
    tri = np.zeros(112, np.uint8)
    return orc.OracleScene(tri, layout.pack_materials([scenes.WHITE]), None, env)


def _look(position, target):
    d = np.array(target, np.float64) - np.array(position, np.float64)
    return d / math.sqrt(float(d @ d))


def _cameras(rng, n):
    """Exterior cameras around and above a scene that sits on the 5 x 5 floor: (position, direction, fov, focal distance)."""
    cams = []
    # the default view; direction components of exactly zero; the camera level with a box face (the floor's plane y = 0, the demo
    # box's top 0.8, the sphere's top 1.0 -- the default camera's height)
    cams.append(((0.0, 1.0, 4.0), _look((0.0, 1.0, 4.0), (0.0, 0.0, 0.0)), 45.0, 1.0))
    for y in (0.0, 0.8, 1.0, 0.5):
        cams.append(((0.0, y, 4.0), (0.0, 0.0, -1.0), 45.0, 1.0))
        cams.append(((5.0, y, 0.0), (-1.0, 0.0, 0.0), 60.0, 0.3))
        cams.append(((0.0, y, -6.0), (0.0, 0.0, 1.0), 30.0, 10.0))
        cams.append(((3.0, y, 3.0), (-1.0, 0.0, -1.0), 75.0, 2.0))
    cams.append(((0.0, 6.0, 0.5), (0.0, -1.0, -0.25), 50.0, 1.0))
    cams.append(((2.5, 0.0, 4.0), (0.0, 0.0, -1.0), 40.0, 0.05))       # in the plane of a face of the floor's box, looking along it
    while len(cams) < n:
        az = rng.uniform(0.0, 2.0 * math.pi)
        dist = rng.uniform(2.0, 12.0)
        y = rng.choice([rng.uniform(0.02, 1.5), rng.uniform(1.5, 9.0)])
        pos = (dist * math.cos(az), y, dist * math.sin(az))
        kind = rng.integers(0, 3)
        if kind == 0:        # at the scene
            target = rng.uniform(-0.6, 0.6, 3) + np.array([0.0, 0.4, 0.0])
        elif kind == 1:      # past it: the scene's boxes graze the frame's edge
            target = rng.uniform(-3.5, 3.5, 3) + np.array([0.0, 0.5, 0.0])
        else:                # a corner of the floor
            target = np.array([rng.choice([-2.5, 2.5]), 0.0, rng.choice([-2.5, 2.5])])
        fov = float(rng.uniform(20.0, 120.0))
        focal = float(math.exp(rng.uniform(math.log(0.05), math.log(50.0))))
        cams.append((pos, _look(pos, target), fov, focal))
    return cams


@pytest.fixture(scope="module")
def small_dragon(built):
    sc = scenes.dragon_class_scene(segments=48)
    sc.build_bvh()
    return sc


def _check_scene(orc, sc, env, cams, frames):
    lit = orc.OracleScene(sc.triangles, _emitting(sc), sc.nodes, env)
    nothing = _nothing(orc, env)
    with_empty = 0
    tiles = 0
    for k, (pos, direction, fov, focal) in enumerate(cams):
        u = ptcommon.rt_uniforms(sc, W, H, frame=1, fov=fov, focal=focal, position=pos, direction=direction, aperture=0.0)
        empty = capi.host_sky_tiles(sc.nodes, u.tobytes(), W, H)
        assert empty.shape == (H // 8, W // 8)
        if not empty.any():
            continue
        with_empty += 1
        tiles += int(empty.sum())
        mask = _pixel_mask(empty, W, H)
        for frame in frames:
            u.set({"frame": int(frame)})
            got, _ = orc.raytrace(lit, u.tobytes(), W, H)
            want, _ = orc.raytrace(nothing, u.tobytes(), W, H)
            assert ptcommon.same_bits(got[mask], want[mask]), \
                f"{sc.name} camera {k} {pos} {direction} fov {fov} focal {focal} frame {frame}: " + ptcommon.describe_diff(got[mask], want[mask])
            # ... and nothing was hit there: with every material emitting, a hit adds light the empty scene's path does not have
    return with_empty, tiles


def test_empty_tiles_render_as_an_empty_scene_does(built, orc, demo, small_dragon, env):
    rng = np.random.default_rng(20240607)
    total = 0
    for sc, n in ((demo, 110), (small_dragon, 110)):
        cams = _cameras(rng, n)
        with_empty, tiles = _check_scene(orc, sc, env, cams, frames=(1, 2, 77, 4000))
        # not vacuous: most exterior views have sky in them
        assert with_empty >= n // 3 and tiles >= 20 * with_empty, (sc.name, with_empty, tiles)
        total += n
    assert total >= 200


def test_the_set_is_empty_where_the_split_is_not_proven(built, demo):
    sc = demo
    def share(**kw):
        u = ptcommon.rt_uniforms(sc, W, H, **kw)
        return float(capi.host_sky_tiles(sc.nodes, u.tobytes(), W, H).mean())
    assert share() > 0.1                                        # the default view: sky above the floor's far edge
    assert share(aperture=0.01) == 0.0                          # thin lens: the ray's origin moves
    assert share(spf=2) == 0.0
    assert share(bounces=0) == 0.0                              # no segment is traced at all: the pixel is 0, not the environment
    assert share(position=(-0.0, 1.0, 4.0)) == 0.0              # a -0 camera coordinate: the kernel's thin-lens branch runs
    assert share(position=(0.0, 1.0, -0.0), direction=(0.0, -0.3, 1.0)) == 0.0
    assert share(position=(0.5, 0.0, 0.5), direction=(1.0, 0.2, 0.0)) == 0.0      # inside the floor's (flat) box
    assert share(position=(0.0, 0.4, 0.5), direction=(0.0, 0.0, -1.0)) == 0.0     # inside the demo box
    assert share(position=(0.0, 9.0, 0.0), direction=(0.0, -1.0, 0.0)) == 0.0     # straight down: the frame's `up` vector switches
    # a tree whose boxes are not nested has no cut
    nodes = np.array(sc.nodes, copy=True)
    raw = nodes.view(np.uint8).reshape(-1, 48)
    child = int(raw[0, 32:36].view(np.int32)[0])
    raw[child, 0:4] = np.array([-1000.0], np.float32).view(np.uint8)
    u = ptcommon.rt_uniforms(sc, W, H)
    assert not capi.host_sky_tiles(nodes, u.tobytes(), W, H).any()


def test_empty_tiles_of_a_rank_render_as_an_empty_scene_does(built, orc, demo, env):
    sc = demo
    h = 104
    lit = orc.OracleScene(sc.triangles, _emitting(sc), sc.nodes, env)
    nothing = _nothing(orc, env)
    u = ptcommon.rt_uniforms(sc, W, h, frame=5)
    seen = 0
    for nranks, block_rows in ((2, 8), (3, 8), (8, 8), (3, 5), (2, 16)):
        for rank in range(nranks):
            e = capi.host_sky_tiles(sc.nodes, u.tobytes(), W, h, rank, nranks, block_rows)
            got, _ = orc.raytrace(lit, u.tobytes(), W, h, rank, nranks, block_rows)
            want, _ = orc.raytrace(nothing, u.tobytes(), W, h, rank, nranks, block_rows)
            mask = _pixel_mask(e, W, got.shape[0])
            seen += int(mask.sum())
            assert ptcommon.same_bits(got[mask], want[mask]), (nranks, block_rows, rank)
    assert seen > 0


def test_bench_views_have_their_share_of_empty_tiles(built, demo):
    """Not vacuous where it is measured: the default camera at 1920 x 1080 on the demo and the dragon-class scene; none from close up."""
    import bench
    u = ptcommon.rt_uniforms(demo, 1920, 1080)
    share = float(capi.host_sky_tiles(demo.nodes, u.tobytes(), 1920, 1080).mean())
    print(f"demo: {share:.4f} of the tiles empty")
    assert share >= 0.15
    sc = scenes.dragon_class_scene()
    sc.build_bvh()
    u = ptcommon.rt_uniforms(sc, 1920, 1080)
    share = float(capi.host_sky_tiles(sc.nodes, u.tobytes(), 1920, 1080).mean())
    print(f"dragon-class: {share:.4f} of the tiles empty")
    assert share >= 0.15
    sc.camera.update(bench.CLOSEUP_CAMERA)
    u = ptcommon.rt_uniforms(sc, 1920, 1080)
    assert not capi.host_sky_tiles(sc.nodes, u.tobytes(), 1920, 1080).any()


# ---------------------------------------------------------------- GPU: switch on against off

MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE


def _run(ctx, sc, w, h, frames, per_call, on, present=False, **kw):
    """`frames` frames, `per_call` per launch, from a zeroed accumulation; (accumulation image, counters, last launch)."""
    ctx.set_option(capi.OPT_SKY_TILES, 1 if on else 0)
    ctx.reset()
    ctx.reset_counters()
    if present:
        ctx.set_uniforms(capi.PASS_FULLSCREEN, ptcommon.fs_uniforms(w, h).tobytes())
    f = 1
    while f < 1 + frames:
        k = min(per_call, 1 + frames - f)
        ctx.set_uniforms(capi.PASS_RAYTRACE, ptcommon.rt_uniforms(sc, w, h, frame=f, **kw).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, ptcommon.acc_uniforms(w, h, f).tobytes())
        if present:
            for _ in range(k):
                ctx.set_uniforms(capi.PASS_RAYTRACE, ptcommon.rt_uniforms(sc, w, h, frame=f, **kw).tobytes())
                ctx.set_uniforms(capi.PASS_ACCUMULATE, ptcommon.acc_uniforms(w, h, f).tobytes())
                ctx.submit(MASK | capi.SUBMIT_FULLSCREEN)
                f += 1
        else:
            ctx.submit_frames(MASK, k)
            f += k
        ctx.flush()
    img = ctx.read_texture(capi.TEX_ACCUMULATION)
    canvas = ctx.read_canvas_rgba8() if present else None
    return img, ctx.counters(), ctx.last_launch(), canvas


def _same(on, off, what):
    assert ptcommon.same_bits(on[0], off[0]), what + ": " + ptcommon.describe_diff(on[0], off[0])
    for k in ptcommon.PATH_COUNTERS:
        assert on[1][k] == off[1][k], f"{what}: counter {k} {on[1][k]} != {off[1][k]}"
    # (box tests are not compared: in the culling walks they depend on how the lanes of a wave happen to be filled -- a parked
    # triangle tested earlier culls more boxes -- and stay below the oracle's either way, ptcommon.check_counters)
    if on[3] is not None:
        assert np.array_equal(on[3], off[3]), what + ": canvas"


def _split_shows(ctx, sc, w, h, frames, on, off, **kw):
    """Was the persistent kernel given fewer jobs?  A traced sample of an empty tile counts at least its root box test (one per segment
    start), a streamed one none: with the split in use for `frames` frames the box tests fall by at least the empty tiles' pixels x frames.
    (Half of that is asked for: the culling walks' box count moves by some 0.01 % with the filling of the waves.)"""
    e = capi.host_sky_tiles(sc.nodes, ptcommon.rt_uniforms(sc, w, h, **kw).tobytes(), w, h)
    px = int(_pixel_mask(e, w, h).sum())
    return px > 0 and off[1]["box_tests"] - on[1]["box_tests"] >= 0.5 * px * frames


def _ab(ctx, sc, w, h, frames, per_call, what, **kw):
    off = _run(ctx, sc, w, h, frames, per_call, False, **kw)
    on = _run(ctx, sc, w, h, frames, per_call, True, **kw)
    _same(on, off, what)
    return on, off


@pytest.mark.gpu
def test_gpu_switch_on_equals_off_for_random_exterior_cameras(built, demo, small_dragon, env):
    rng = np.random.default_rng(99)
    used = 0
    with capi.Context(0) as ctx:
        assert ctx.get_option(capi.OPT_SKY_TILES) == 1           # on by default
        for sc in (demo, small_dragon):
            ptcommon.upload_scene(ctx, sc, env)
            for (w, h) in ((160, 96), (328, 200)):
                ctx.resize(w, h)
                cams = _cameras(rng, 40)
                for k, (pos, direction, fov, focal) in enumerate(cams[:2] + cams[-5:]):
                    kw = dict(fov=fov, focal=focal, position=pos, direction=direction, rotation=0.37 * k, aperture=0.0)
                    # batch depths 1 (an interactive host: the split starts once the camera has stood still for a launch), 16, 160
                    for frames, per_call in ((4, 1), (32, 16), (160, 160)):
                        on, off = _ab(ctx, sc, w, h, frames, per_call, f"{sc.name} {w}x{h} camera {k} depth {per_call}", **kw)
                        assert on[2]["kind"] == 1 and on[2]["lean"] and on[2]["variant"] >= 9
                        used += _split_shows(ctx, sc, w, h, frames - 1, on, off, **kw)
    assert used >= 12            # not vacuous: most of these views have sky in them


@pytest.mark.gpu
def test_gpu_switch_on_equals_off_for_the_bench_views(built, demo, env):
    import bench
    views = [("demo", demo, {})]
    sc = scenes.dragon_class_scene(segments=96)
    sc.build_bvh()
    views.append(("dragon", sc, {}))
    p = bench.CLOSEUP_CAMERA["position"]
    views.append(("closeup", sc, dict(position=p, direction=_look(p, bench.CLOSEUP_CAMERA["target"]))))
    forest = scenes.forest_scene(instances=60)
    forest.build_bvh()
    views.append(("forest", forest, {}))
    with capi.Context(0) as ctx:
        ctx.resize(480, 272)
        for name, sc, kw in views:
            ptcommon.upload_scene(ctx, sc, env)             # a scene upload between launches: the cached list must not survive it
            _ab(ctx, sc, 480, 272, 48, 16, name, **kw)


@pytest.mark.gpu
def test_gpu_cache_follows_camera_scene_and_size(built, demo, small_dragon, env):
    with capi.Context(0) as ctx:
        ptcommon.upload_scene(ctx, demo, env)
        ctx.resize(328, 200)
        on, off = _ab(ctx, demo, 328, 200, 12, 4, "default view")
        assert _split_shows(ctx, demo, 328, 200, 8, on, off)                   # (the first launch of four frames runs whole: the camera has not stood still yet)
        # with the switch left ON: a camera change, a scene upload and a resize between launches, against a fresh context with it off
        ctx.set_option(capi.OPT_SKY_TILES, 1)
        steps = [(demo, (328, 200), dict(position=(3.0, 2.0, 3.0), direction=_look((3.0, 2.0, 3.0), (0.0, 0.3, 0.0)))),
                 (small_dragon, (328, 200), {}), (small_dragon, (200, 120), {}), (small_dragon, (200, 120), dict(fov=80.0)),
                 (demo, (200, 120), {})]
        with capi.Context(0) as ref:
            ref.set_option(capi.OPT_SKY_TILES, 0)
            cur_sc, cur_size = demo, (328, 200)
            ptcommon.upload_scene(ref, demo, env)
            ref.resize(328, 200)
            for sc, size, kw in steps:
                for c in (ctx, ref):
                    if sc is not cur_sc:
                        ptcommon.upload_scene(c, sc, env)
                    if size != cur_size:
                        c.resize(*size)
                cur_sc, cur_size = sc, size
                got = _run(ctx, sc, size[0], size[1], 32, 16, True, **kw)
                want = _run(ref, sc, size[0], size[1], 32, 16, False, **kw)
                _same(got, want, f"{sc.name} {size} {sorted(kw)}")


@pytest.mark.gpu
def test_gpu_tile_splits_groups_storage_subrectangle_and_presenting_frames(built, demo, env):
    sc = demo
    w, h = 328, 200
    for nranks in (2, 3, 8):
        for rank in sorted({0, 1, nranks - 1}):
            with capi.Context(0) as ctx:
                ctx.set_tile(rank, nranks, 8)
                ptcommon.upload_scene(ctx, sc, env)
                ctx.resize(w, h)
                _ab(ctx, sc, w, h, 32, 16, f"rank {rank} of {nranks}")
    for members in (2, 3):
        with capi.Context(devices=[0] * members) as g:
            ptcommon.upload_scene(g, sc, env)
            g.resize(w, h)
            _ab(g, sc, w, h, 32, 16, f"group of {members}")
    with capi.Context(0) as ctx:
        ctx.set_storage(capi.STORAGE_F16)
        ptcommon.upload_scene(ctx, sc, env)
        ctx.resize(w, h)
        _ab(ctx, sc, w, h, 32, 16, "F16 storage")
    with capi.Context(0) as ctx:
        ptcommon.upload_scene(ctx, sc, env)
        ctx.resize(w, h)
        # a scalingFactor < 1 sub-rectangle: the resolution uniform is smaller than the textures (renderer.ts:283-312)
        res = (w // 2, h // 2)
        on, _ = _ab(ctx, sc, w, h, 32, 16, "sub-rectangle", res=res, aspect=res[0] / res[1])
        assert on[1]["pixels"] == 32 * res[0] * res[1]
        _ab(ctx, sc, w, h, 24, 8, "presenting frames", present=True)
        _ab(ctx, sc, w, h, 32, 16, "env rotation", rotation=2.1, intensity=0.7)
