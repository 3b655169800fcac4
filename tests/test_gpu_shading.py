"""The shading side of the path -- the hit branch of trace() (raytrace.wgsl:380-395: three copies on the device, the per-pixel
kernel, the experiment build's persistent kernel and the service step of the state-machine kernel) and the miss branch (shared by
that service step and the streaming kernel of MI3PT_OPT_SKY_TILES) -- against the oracle, at the inputs tests/shading_cases.py
lists: materials at and beyond the ends of their ranges, emission that overflows binary32 and binary16, NaN / inf / negative /
subnormal environment texels, draws of rand() forced to exactly 0 and exactly 1, frame counters that wrap.

Every comparison is bit for bit (NaN equal to NaN) plus the path counters.  What makes a case more than a repeat of the ordinary
frames -- a NaN pixel, an overflow, a draw that decides the other way -- is asserted on the ORACLE's output only
(shading_cases.check_* / *_reference, the same code tests/test_shading_cases.py runs without a GPU), never on the device's."""
import numpy as np
import pytest

import ptcommon as pc
import shading_cases as sh
from mi3pt_host import capi

pytestmark = pytest.mark.gpu

MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
VARIANTS = (0, 13, 14, 1, 2, 4, 7, 9, 10)
W, H = sh.W, sh.H


@pytest.fixture(scope="module")
def palette(built):
    return sh.palette_scene()


@pytest.fixture
def ctx(gpu_ctx):
    gpu_ctx.set_tile(0, 1, 8)
    gpu_ctx.set_storage(capi.STORAGE_F32)
    gpu_ctx.set_pipelining(True)
    sky = gpu_ctx.get_option(capi.OPT_SKY_TILES)
    yield gpu_ctx
    gpu_ctx.set_kernel_variant(0)
    gpu_ctx.set_pipelining(True)
    gpu_ctx.set_storage(capi.STORAGE_F32)
    gpu_ctx.set_option(capi.OPT_SKY_TILES, sky)
    gpu_ctx.resize(64, 64)


def select(ctx, variant):
    """Selects a kernel variant; the variant that will run (nothing falls back: these trees admit every walk)."""
    ctx.set_kernel_variant(variant)
    active = ctx.active_variant()
    assert active == variant if variant else active >= 9, (variant, active)
    return active


def check_launch(ctx, active, what):
    """The most recent raytrace launch ran the kernel that was asked for: the per-pixel kernel for variants 1 / 2, else the lean
    build of the state-machine kernel."""
    last = ctx.last_launch()
    want = (0, active) if active in (1, 2) else (1, active)
    assert (last["kind"], last["variant"]) == want and (last["lean"] or last["kind"] == 0), (what, last)


def check_frame(ctx, active, rt_u, want, want_cnt, what):
    """One raytrace pass alone against the oracle's image and counters."""
    ctx.reset_counters()
    pc.gpu_frame(ctx, rt_u)
    got = ctx.read_texture(capi.TEX_OUTPUT)
    assert pc.same_bits(got, want), what + ": " + pc.describe_diff(got, want)
    pc.check_counters(ctx.counters(), want_cnt, culled=active >= 9, what=what)
    check_launch(ctx, active, what)


# ---------------------------------------------------------------- a. the palette

@pytest.mark.parametrize("storage", [capi.STORAGE_F32, capi.STORAGE_F16], ids=["F32", "F16"])
def test_palette_matches_the_oracle_on_every_kernel(ctx, orc, env, palette, storage):
    """Frames 2 .. 5 of the 14-material palette, six bounces, accumulated: one submit_frames(.., 4) (the batched state-machine
    kernel + the ordered multi-frame accumulate) and four fused launches with pipelining off, on every kernel variant of this build,
    then the fullscreen pass on that mean.  Oracle's mean: F32 1 NaN pixel and 23 with an inf, F16 1 and 52 (printed)."""
    f16 = storage == capi.STORAGE_F16
    mean, cnt = sh.palette_reference(orc, palette, env, f16)
    twin, _ = sh.palette_reference(orc, palette, env, not f16)
    sh.check_palette_stats(*(sh.image_stats(m) for m in ((twin, mean) if f16 else (mean, twin))))
    pc.upload_scene(ctx, palette, env)
    ctx.set_storage(storage)
    ctx.resize(W, H)
    variants = pc.variants_available(ctx, VARIANTS)
    assert {0, 13, 2, 7, 9}.issubset(variants)
    for variant in variants:
        active = select(ctx, variant)
        for pipelined in (True, False):
            what = f"palette variant {variant} storage {storage} pipelined {pipelined}"
            ctx.set_pipelining(pipelined)
            ctx.reset()
            ctx.reset_counters()
            if pipelined:
                first = sh.PALETTE_FRAMES[0]
                ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(palette, W, H, frame=first, bounces=sh.PALETTE_BOUNCES).tobytes())
                ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, first).tobytes())
                ctx.submit_frames(MASK, len(sh.PALETTE_FRAMES))
            else:
                for f in sh.PALETTE_FRAMES:
                    pc.gpu_frame(ctx, pc.rt_uniforms(palette, W, H, frame=f, bounces=sh.PALETTE_BOUNCES), pc.acc_uniforms(W, H, f), MASK)
            got = ctx.read_texture(capi.TEX_ACCUMULATION)
            assert pc.same_bits(got, mean), what + ": " + pc.describe_diff(got, mean)
            pc.check_counters(ctx.counters(), cnt, culled=active >= 9, what=what)
            check_launch(ctx, active, what)
        # the mean is in the accumulation image: tone-map and draw it (NaN -> 0 in the RGBA8 canvas)
        for denoise, tonemapping in ((1, 1), (0, 2), (0, 0)):
            fs = pc.fs_uniforms(W, H, 1.0, denoise, tonemapping)
            ctx.set_uniforms(capi.PASS_FULLSCREEN, fs.tobytes())
            ctx.submit(capi.SUBMIT_FULLSCREEN)
            want_f, want_8 = orc.fullscreen(fs.tobytes(), mean)
            got_f = ctx.read_texture(capi.TEX_CANVAS)
            what = f"palette variant {variant} storage {storage} denoise {denoise} tonemapping {tonemapping}"
            assert pc.same_bits(got_f, want_f), what + ": " + pc.describe_diff(got_f, want_f)
            assert np.array_equal(ctx.read_canvas_rgba8(), want_8), what + ": RGBA8 canvas"


# ---------------------------------------------------------------- b. the environment

def test_edge_environment_on_every_kernel(ctx, orc, palette):
    """The palette under an environment with 1e38, inf, NaN, -2, a subnormal and 0 around the horizon: frame 3, five bounces, the
    raytrace pass alone.  Oracle: 320 / 216 / 256 / 242 of 3072 pixels with a NaN / an inf / a negative / a subnormal component."""
    env = sh.edge_env()
    want, cnt, _ = sh.oracle_run(orc, pc.oracle_scene(orc, palette, env), palette, (sh.EDGE_FRAME,), bounces=sh.EDGE_BOUNCES)
    sh.check_edge_env_stats(sh.image_stats(want))
    pc.upload_scene(ctx, palette, env)
    ctx.resize(W, H)
    u = pc.rt_uniforms(palette, W, H, frame=sh.EDGE_FRAME, bounces=sh.EDGE_BOUNCES)
    for variant in pc.variants_available(ctx, VARIANTS):
        check_frame(ctx, select(ctx, variant), u, want, cnt, f"edge environment variant {variant}")


@pytest.mark.parametrize("camera", list(sh.SKY_CAMERAS))
def test_edge_environment_through_the_sky_tile_kernel(ctx, orc, palette, camera):
    """Six accumulated frames in three launches of two: from the second launch on the tiles that see no geometry are shaded by the
    streaming kernel (MI3PT_OPT_SKY_TILES 1, the default) -- from the edge texels.  With the option at 0 and at 1 against the oracle;
    that the split was in use shows in the box tests (a streamed sample has none)."""
    kw = sh.SKY_CAMERAS[camera]
    env = sh.edge_env()
    mean, cnt, _ = sh.oracle_run(orc, pc.oracle_scene(orc, palette, env), palette, sh.SKY_FRAMES, sh.SKY_FRAMES, bounces=sh.EDGE_BOUNCES, **kw)
    print(f"{camera}: oracle's mean of frames {sh.SKY_FRAMES}: {sh.image_stats(mean)}")
    pc.upload_scene(ctx, palette, env)
    ctx.resize(W, H)
    active = select(ctx, 0)
    box_tests = {}
    for on in (0, 1):
        what = f"edge environment, {camera}, sky tiles {on}"
        ctx.set_option(capi.OPT_SKY_TILES, on)
        ctx.reset()
        ctx.reset_counters()
        for f in sh.SKY_FRAMES[::sh.SKY_PER_LAUNCH]:
            ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(palette, W, H, frame=f, bounces=sh.EDGE_BOUNCES, **kw).tobytes())
            ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, f).tobytes())
            ctx.submit_frames(MASK, sh.SKY_PER_LAUNCH)
            ctx.flush()
        got = ctx.read_texture(capi.TEX_ACCUMULATION)
        assert pc.same_bits(got, mean), what + ": " + pc.describe_diff(got, mean)
        counters = ctx.counters()
        pc.check_counters(counters, cnt, culled=True, what=what)
        check_launch(ctx, active, what)
        box_tests[on] = counters["box_tests"]
    empty = capi.host_sky_tiles(palette.nodes, pc.rt_uniforms(palette, W, H, **kw).tobytes(), W, H)
    streamed = int(empty.sum()) * 64 * (len(sh.SKY_FRAMES) - sh.SKY_PER_LAUNCH)          # samples of the launches behind the first
    print(f"{camera}: box tests {box_tests}, {streamed} samples in empty tiles behind the first launch")
    # Not a condition on the case (those are the oracle's, above) but on the route, like check_launch: no entry point says whether a
    # launch split its tiles, the counters do.  A traced sample of an empty tile costs at least the root's box test, a streamed one
    # none, so the split saves at least `streamed` box tests; half of that is asked for, because the culling walks' own count moves
    # with the filling of the waves -- by some 0.01 % of a few hundred thousand, far below the other half (tests/test_sky_tiles.py,
    # _split_shows, where the bound comes from).
    assert box_tests[0] - box_tests[1] >= streamed // 2


def test_environment_intensity_and_rotation(ctx, orc, env, palette):
    """envMapIntensity 0 (what is left is emission: material 9's negative and material 13's subnormal radiance show, 7 and 18 pixels),
    negative (3042 negative pixels) and huge (49 with an inf); envMapRotation one ulp above 2 pi, negative and 100 rad (inside the
    range the sine / cosine tests cover)."""
    pc.upload_scene(ctx, palette, env)
    ctx.resize(W, H)
    osc = pc.oracle_scene(orc, palette, env)
    variants = pc.variants_available(ctx, VARIANTS)
    for intensity, rotation in sh.ENV_SETTINGS:
        kw = dict(bounces=sh.EDGE_BOUNCES, intensity=intensity, rotation=rotation)
        want, cnt, _ = sh.oracle_run(orc, osc, palette, (sh.EDGE_FRAME,), **kw)
        print(f"envMapIntensity {intensity} envMapRotation {rotation}: {sh.image_stats(want)}")
        if intensity == 0.0:
            sh.check_dark_env_stats(sh.image_stats(want))
        u = pc.rt_uniforms(palette, W, H, frame=sh.EDGE_FRAME, **kw)
        for variant in variants:
            check_frame(ctx, select(ctx, variant), u, want, cnt, f"intensity {intensity} rotation {rotation} variant {variant}")


def test_cameras_looking_straight_up_and_down(ctx, orc, env, palette):
    """Camera at (0, 3, 0) with direction (0, 1, 0) and (0, -1, 0): cameraToRay takes its other up vector (|w . up| > 0.99999) and
    yields finite rays -- the centre ray is the direction itself, the corner rays (-+0.368, +-0.888, -0.276); looking up every pixel
    is sky, looking down the image is full of geometry (tests/test_shading_cases.py::test_pole_cameras)."""
    pc.upload_scene(ctx, palette, env)
    ctx.resize(W, H)
    osc = pc.oracle_scene(orc, palette, env)
    variants = pc.variants_available(ctx, VARIANTS)
    for direction in sh.POLE_DIRECTIONS:
        kw = dict(bounces=sh.EDGE_BOUNCES, position=sh.POLE_POSITION, direction=direction)
        want, cnt, _ = sh.oracle_run(orc, osc, palette, (sh.EDGE_FRAME,), **kw)
        print(f"camera direction {direction}: {sh.image_stats(want)}, {cnt['hits']} hits, {cnt['misses']} misses")
        assert (cnt["hits"] == 0 and cnt["misses"] == W * H) if direction[1] > 0 else cnt["hits"] > 1000
        u = pc.rt_uniforms(palette, W, H, frame=sh.EDGE_FRAME, **kw)
        for variant in variants:
            check_frame(ctx, select(ctx, variant), u, want, cnt, f"camera direction {direction} variant {variant}")


# ---------------------------------------------------------------- c. forced draws

@pytest.mark.parametrize("name", list(sh.FORCED_CASES))
def test_forced_draws(ctx, orc, env, name):
    """The frame counter chosen so that one draw of one pixel is exactly 0 (log(0) in randNormal: a NaN direction, a NaN pixel; a
    zero jitter radius; metalness 0 >= 0) or exactly 1 (an angle of 2 pi; metalness 1 >= 1).  Raytrace frames (F - 1, F, F + 1)
    under accumulate frames (1, 2, 3) in one batched launch, and frame F alone from the per-pixel kernel and the shipped one."""
    ref = sh.forced_reference(orc, env, name)
    sc = ref["scene"]
    pc.upload_scene(ctx, sc, env)
    ctx.resize(W, H)
    active = select(ctx, 0)
    ctx.reset()
    ctx.reset_counters()
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, W, H, frame=ref["rt_frames"][0], bounces=sh.PALETTE_BOUNCES).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, 1).tobytes())
    ctx.submit_frames(MASK, 3)
    got = ctx.read_texture(capi.TEX_ACCUMULATION)
    assert pc.same_bits(got, ref["mean"]), name + ", batched: " + pc.describe_diff(got, ref["mean"])
    pc.check_counters(ctx.counters(), ref["mean_counters"], culled=True, what=name)
    check_launch(ctx, active, name)
    ctx.set_pipelining(False)
    u = pc.rt_uniforms(sc, W, H, frame=ref["frame"], bounces=sh.PALETTE_BOUNCES)
    for variant in (2, 0):
        check_frame(ctx, select(ctx, variant), u, ref["image"], ref["counters"], f"{name}, frame F alone, variant {variant}")


# ---------------------------------------------------------------- d. frame counters at the ends of u32

@pytest.mark.parametrize("name", list(sh.WRAP_CASES))
def test_frame_counters_wrap(ctx, orc, demo, env, name):
    """Frames whose raytrace `frame` runs 0xFFFFFFFE, 0xFFFFFFFF, 0, 1 behind one ordinary frame: with the accumulate `frame`
    wrapping alongside (its step at 0 has weight 1 and replaces the mean), starting at 0, and with accumulation disabled -- one
    submit_frames against separate launches with pipelining off and against the oracle.  The step behind accumulate frame 0 is
    frame 1, which replaces the mean again whatever frame 0 did; so two more runs END at accumulate frame 0 (three frames from
    0xFFFFFFFE, four from 0xFFFFFFFD): there the image compared is the last frame alone, over 2000 pixels away from the mean in
    front of it (asserted on the oracle), and a step at 0 with any other weight than 1 fails."""
    ref = sh.wrap_reference(orc, demo, env, name)
    pc.upload_scene(ctx, demo, env)
    ctx.resize(W, H)
    active = select(ctx, 0)
    images = {}
    for batched in (True, False):
        what = f"{name}, {'one submit_frames' if batched else 'a launch per frame'}"
        ctx.set_pipelining(batched)
        ctx.reset()
        ctx.reset_counters()
        pc.gpu_frame(ctx, pc.rt_uniforms(demo, W, H, frame=sh.WRAP_SEED_FRAME, bounces=4), pc.acc_uniforms(W, H, 1), MASK)
        ctx.flush()
        if batched:
            ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, W, H, frame=ref["rt_frames"][0], bounces=4).tobytes())
            ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, ref["acc_frames"][0], ref["enabled"]).tobytes())
            ctx.submit_frames(MASK, len(ref["rt_frames"]))
        else:
            for f, g in zip(ref["rt_frames"], ref["acc_frames"]):
                pc.gpu_frame(ctx, pc.rt_uniforms(demo, W, H, frame=f, bounces=4), pc.acc_uniforms(W, H, g, ref["enabled"]), MASK)
        images[batched] = ctx.read_texture(capi.TEX_ACCUMULATION)
        assert pc.same_bits(images[batched], ref["mean"]), what + ": " + pc.describe_diff(images[batched], ref["mean"])
        pc.check_counters(ctx.counters(), ref["counters"], culled=True, what=what)
        check_launch(ctx, active, what)
    assert pc.same_bits(images[True], images[False])
