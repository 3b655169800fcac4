"""The images of a context -- textures, canvas, feature images, filtered image, variance image, moments image -- behind one read /
write / pointer path (pt_context.hip: read_plane; pt_ctx_image.hip: write_plane, hand_out_plane): what every entry point answers in every state, and a rank without rows.

The codes of EXPECTED are what the library answered before the entry points shared that path: the table was printed by this loop on the
library of the commit before (the separate copies of the plumbing) and committed as a literal, so that "the order of the checks is
kept" is asserted.  1 = MI3PT_ERR_INVALID, 4 = MI3PT_ERR_STATE."""
import ctypes

import numpy as np
import pytest

import ptcommon as pc
from mi3pt_host import capi

pytestmark = pytest.mark.gpu
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
W = H = 16
TEXELS = W * H


def _reader(name, *lead):
    return lambda lib, h, buf, n: getattr(lib, name)(h, *lead, buf, n)


def _pointer(name, *lead):
    def call(lib, h, buf, n):
        p, nbytes = ctypes.c_void_p(), ctypes.c_size_t()
        return getattr(lib, name)(h, *lead, ctypes.byref(p), ctypes.byref(nbytes))
    return call


# name -> (call, the size argument of an image of `texels` texels, one element of it); a pointer entry point takes no buffer: its "short"
# column is the ready state asked once more
def _entry_points(texels):
    return {
        "read_texture(output)": (_reader("mi3pt_read_texture", capi.TEX_OUTPUT), texels * 4, 1),
        "read_texture(accumulation)": (_reader("mi3pt_read_texture", capi.TEX_ACCUMULATION), texels * 4, 1),
        "read_texture(canvas)": (_reader("mi3pt_read_texture", capi.TEX_CANVAS), texels * 4, 1),
        "read_canvas_rgba8": (_reader("mi3pt_read_canvas_rgba8"), texels * 4, 4),
        "read_aov": (_reader("mi3pt_read_aov", capi.AOV_NORMAL), texels * 16, 16),
        "aov_device_ptr": (_pointer("mi3pt_aov_device_ptr", capi.AOV_NORMAL), 0, 0),
        "read_guided": (_reader("mi3pt_read_guided"), texels * 16, 16),
        "guided_device_ptr": (_pointer("mi3pt_guided_device_ptr"), 0, 0),
        "read_guided_variance": (_reader("mi3pt_read_guided_variance"), texels, 1),
        "read_moments": (_reader("mi3pt_read_moments"), texels * 16, 16),
        "write_moments": (_reader("mi3pt_write_moments"), texels * 16, 16),
        "moments_device_ptr": (_pointer("mi3pt_moments_device_ptr"), 0, 0),
        "write_texture": (_reader("mi3pt_write_texture", capi.TEX_ACCUMULATION), texels * 4, 1),
        "accumulation_device_ptr": (_pointer("mi3pt_accumulation_device_ptr"), 0, 0),
    }


ENTRY_POINTS = _entry_points(TEXELS)
STATES = ("before resize", "resized, nothing rendered / filtered / enabled", "ready, buffer one element short", "ready")

EXPECTED_SINGLE = {
    "read_texture(output)": (4, 0, 1, 0),
    "read_texture(accumulation)": (4, 0, 1, 0),
    "read_texture(canvas)": (4, 0, 1, 0),
    "read_canvas_rgba8": (4, 0, 1, 0),
    "read_aov": (4, 4, 1, 0),
    "aov_device_ptr": (4, 4, 0, 0),
    "read_guided": (4, 4, 1, 0),
    "guided_device_ptr": (4, 4, 0, 0),
    "read_guided_variance": (4, 4, 1, 0),
    "read_moments": (4, 4, 1, 0),
    "write_moments": (4, 4, 1, 0),
    "moments_device_ptr": (4, 4, 0, 0),
    "write_texture": (4, 0, 1, 0),
    "accumulation_device_ptr": (4, 0, 0, 0),
}
# a group [0, 0]: whole images through the presenting context; the filter and write_moments are refused in every state
EXPECTED_GROUP = dict(EXPECTED_SINGLE, **{name: (4, 4, 4, 4) for name in ("read_guided", "guided_device_ptr", "read_guided_variance", "write_moments")})


def answers(ctx, demo, env, group):
    """{entry point: its code in each of STATES}; every call goes to the C function itself (the Python wrappers size their buffers)"""
    buf = np.zeros((H, W, 4), np.float32)          # 4096 bytes: as large as the largest image here
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    table = {name: [] for name in ENTRY_POINTS}

    def ask(short):
        for name, (call, size, element) in ENTRY_POINTS.items():
            table[name].append(call(ctx.lib, ctx.handle, ptr, size - (element if short else 0)))

    pc.upload_scene(ctx, demo, env)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, W, H, frame=1, bounces=2).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, 1).tobytes())
    ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(W, H, 1.0, 0, 1).tobytes())
    ask(False)
    ctx.resize(W, H)
    ask(False)
    ctx.set_moments(True)
    ctx.submit_frames(MASK, 2)
    ctx.render_aovs(capi.AOV_ALL)
    if not group:          # (the filter is not built for a group: its entry points answer the same in every state)
        ctx.denoise_guided(levels=2, flags=capi.GUIDED_VARIANCE)
    ask(True)
    ask(False)
    return {name: tuple(codes) for name, codes in table.items()}


def _assert_table(got, want, what):
    print(what)
    for name, codes in got.items():
        print(f"    {name!r}: {codes},")
    bad = {name: (codes, want.get(name)) for name, codes in got.items() if codes != want.get(name)}
    assert not bad and set(got) == set(want), f"{what}: (got, expected) per entry point over {STATES}: {bad}"


def test_every_entry_point_answers_as_before_in_every_state(built, demo, env):
    with capi.Context(0) as ctx:
        _assert_table(answers(ctx, demo, env, False), EXPECTED_SINGLE, "single context")


def test_a_group_answers_as_before_in_every_state(built, demo, env):
    with capi.Context(devices=[0, 0]) as g:
        _assert_table(answers(g, demo, env, True), EXPECTED_GROUP, "group [0, 0]")


def test_a_rank_without_rows(built, demo, env):
    """16 x 8, rank 2 of 3 with 8-row blocks: the one block goes to rank 0, this rank has no rows.  Its images are 16-byte placeholders:
    every pass, read and pointer answers OK, the reads are empty and the pointers non-null over 0 bytes."""
    w, h = 16, 8
    assert capi.tile_local_rows(h, 2, 3, 8) == 0
    with capi.Context(0) as ctx:
        ctx.set_tile(2, 3, 8)
        ctx.set_moments(True)
        pc.upload_scene(ctx, demo, env)
        ctx.resize(w, h)
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=1, bounces=2).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1).tobytes())
        ctx.submit_frames(MASK, 2)
        ctx.submit(MASK)
        ctx.render_aovs(capi.AOV_ALL)
        reads = [ctx.read_texture(capi.TEX_OUTPUT), ctx.read_texture(capi.TEX_ACCUMULATION), ctx.read_moments()]
        reads += [ctx.read_aov(k) for k in range(capi.AOV_COUNT)]
        for image in reads:
            assert image.shape == (0, w, 4)
        ctx.write_texture(capi.TEX_ACCUMULATION, reads[1])
        ctx.write_moments(reads[2])
        pointers = [ctx.accumulation_device_ptr(), ctx.moments_device_ptr()] + [ctx.aov_device_ptr(k) for k in range(capi.AOV_COUNT)]
        for p, nbytes in pointers:
            assert p and nbytes == 0
        assert len({p for p, _ in pointers}) == len(pointers)
        ctx.sync()
        assert ctx.counters()["pixels"] == 0


# ---- the state a second resize leaves behind ----
W2, H2 = 20, 12          # a partial 8 x 8 tile on both axes
TILES2 = ((H2 + 7) // 8) * ((W2 + 7) // 8)

# what brings every per-size resource of a 16 x 16 context to life, in this order (name, call); the codes are part of the literal: a group
# refuses some of these, and what it refuses must stay refused
SETUP = (
    ("set_moments", lambda lib, h: lib.mi3pt_set_moments(h, 1)),
    ("set_mean_by_count", lambda lib, h: lib.mi3pt_set_mean_by_count(h, 1)),
    ("enable_timing", lambda lib, h: lib.mi3pt_enable_timing(h, 1)),
    ("submit_frames(2)", lambda lib, h: lib.mi3pt_submit_frames(h, MASK, 2)),
    ("submit(all three passes)", lambda lib, h: lib.mi3pt_submit(h, MASK | capi.SUBMIT_FULLSCREEN)),
    ("render_aovs", lambda lib, h: lib.mi3pt_render_aovs(h, capi.AOV_ALL)),
    ("set_guided_despike", lambda lib, h: lib.mi3pt_set_guided_despike(h, 1)),
    ("denoise_guided", lambda lib, h: lib.mi3pt_denoise_guided(h, ctypes.byref(capi.GuidedParams(2, 1.0, 0.35, 0.1, 0.05, capi.GUIDED_VARIANCE)))),
    ("reproject", lambda lib, h: lib.mi3pt_reproject(h, ctypes.byref(capi.ReprojectParams(0.02, 0.9, 64, 0)))),
    ("hold_history", lambda lib, h: lib.mi3pt_hold_history(h)),
    ("estimate_convergence", lambda lib, h: lib.mi3pt_estimate_convergence(h, 0.1, 1)),
    ("set_sample_mask", lambda lib, h: lib.mi3pt_set_sample_mask(h, np.array([0, 1, 1, 1], np.uint8).ctypes.data_as(ctypes.c_void_p), 4)),
)


def _extras(lib, h, ptr):
    """the entry points beside the table's, asked after the second resize: (name, code or (code, what it answered))"""
    count, sampled = ctypes.c_uint32(0xdead), ctypes.c_uint32(0xdead)
    conv, us = capi.Convergence(), ctypes.c_float()
    yield "read_guided_despiked", lib.mi3pt_read_guided_despiked(h, ctypes.byref(count))
    yield "read_convergence", lib.mi3pt_read_convergence(h, ctypes.byref(conv))
    yield "read_convergence_tiles", lib.mi3pt_read_convergence_tiles(h, ptr, TILES2 * 4)
    mask = np.zeros(TILES2, np.uint8)
    rc = lib.mi3pt_read_sample_mask(h, mask.ctypes.data_as(ctypes.c_void_p), TILES2, ctypes.byref(sampled))
    yield "read_sample_mask", (rc, sampled.value, mask.tolist())
    yield "merge_history", lib.mi3pt_merge_history(h, ctypes.byref(capi.HistoryParams(1, 2.0, 4.0, 0)))
    yield "reproject", lib.mi3pt_reproject(h, ctypes.byref(capi.ReprojectParams(0.02, 0.9, 64, 0)))
    for name, which in (("raytrace", capi.PASS_RAYTRACE), ("accumulate", capi.PASS_ACCUMULATE), ("fullscreen", capi.PASS_FULLSCREEN)):
        yield f"pass_time_us({name})", lib.mi3pt_pass_time_us(h, which, ctypes.byref(us))


def _two_frames(ctx, demo):
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, W2, H2, frame=1, bounces=2).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W2, H2, 1).tobytes())
    ctx.submit_frames(MASK, 2)
    return ctx.read_texture(capi.TEX_ACCUMULATION)


def after_second_resize(ctx, demo, env):
    """({step or entry point: answer}, the accumulation image of two frames rendered after it)"""
    buf = np.zeros((H, W, 4), np.float32)          # (as large as the largest image of either size)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    pc.upload_scene(ctx, demo, env)
    ctx.resize(W, H)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, W, H, frame=1, bounces=2).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, 1).tobytes())
    ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(W, H, 1.0, 0, 1).tobytes())
    table = {f"setup: {name}": call(ctx.lib, ctx.handle) for name, call in SETUP}
    ctx.resize(W2, H2)
    for name, (call, size, _) in _entry_points(W2 * H2).items():
        table[name] = call(ctx.lib, ctx.handle, ptr, size)
    table.update(_extras(ctx.lib, ctx.handle, ptr))
    return table, _two_frames(ctx, demo)


EXPECTED_AFTER_RESIZE_SINGLE = {
    "setup: set_moments": 0,
    "setup: set_mean_by_count": 0,
    "setup: enable_timing": 0,
    "setup: submit_frames(2)": 0,
    "setup: submit(all three passes)": 0,
    "setup: render_aovs": 0,
    "setup: set_guided_despike": 0,
    "setup: denoise_guided": 0,
    "setup: reproject": 0,
    "setup: hold_history": 0,
    "setup: estimate_convergence": 0,
    "setup: set_sample_mask": 0,
    "read_texture(output)": 0,
    "read_texture(accumulation)": 0,
    "read_texture(canvas)": 0,
    "read_canvas_rgba8": 0,
    "read_aov": 4,
    "aov_device_ptr": 4,
    "read_guided": 4,
    "guided_device_ptr": 4,
    "read_guided_variance": 4,
    "read_moments": 0,
    "write_moments": 0,
    "moments_device_ptr": 0,
    "write_texture": 0,
    "accumulation_device_ptr": 0,
    "read_guided_despiked": 4,
    "read_convergence": 4,
    "read_convergence_tiles": 4,
    "read_sample_mask": (0, 6, [1, 1, 1, 1, 1, 1]),
    "merge_history": 4,
    "reproject": 4,
    "pass_time_us(raytrace)": 0,
    "pass_time_us(accumulate)": 0,
    "pass_time_us(fullscreen)": 0,
}
EXPECTED_AFTER_RESIZE_GROUP = {
    "setup: set_moments": 0,
    "setup: set_mean_by_count": 0,
    "setup: enable_timing": 0,
    "setup: submit_frames(2)": 0,
    "setup: submit(all three passes)": 0,
    "setup: render_aovs": 0,
    "setup: set_guided_despike": 0,
    "setup: denoise_guided": 4,
    "setup: reproject": 4,
    "setup: hold_history": 4,
    "setup: estimate_convergence": 0,
    "setup: set_sample_mask": 0,
    "read_texture(output)": 0,
    "read_texture(accumulation)": 0,
    "read_texture(canvas)": 0,
    "read_canvas_rgba8": 0,
    "read_aov": 4,
    "aov_device_ptr": 4,
    "read_guided": 4,
    "guided_device_ptr": 4,
    "read_guided_variance": 4,
    "read_moments": 0,
    "write_moments": 4,
    "moments_device_ptr": 0,
    "write_texture": 0,
    "accumulation_device_ptr": 0,
    "read_guided_despiked": 4,
    "read_convergence": 4,
    "read_convergence_tiles": 4,
    "read_sample_mask": (0, 6, [1, 1, 1, 1, 1, 1]),
    "merge_history": 4,
    "reproject": 4,
    "pass_time_us(raytrace)": 0,
    "pass_time_us(accumulate)": 0,
    "pass_time_us(fullscreen)": 4,
}


@pytest.fixture(scope="module")
def fresh_two_frames(built, demo, env):
    """two frames at 20 x 12 on a context that did nothing else"""
    with capi.Context(0) as ctx:
        pc.upload_scene(ctx, demo, env)
        ctx.resize(W2, H2)
        image = _two_frames(ctx, demo)
    image.setflags(write=False)
    return image


@pytest.mark.parametrize("group", [False, True], ids=["single", "group"])
def test_a_second_resize_leaves_nothing_of_the_first_size_behind(built, demo, env, fresh_two_frames, group):
    """Every per-size resource brought to life at 16 x 16 (moments, feature images, the guided filter with its variance and pre-pass images,
    reprojection scratch, held history, convergence records, a sample mask, timers), then a resize to 20 x 12: what every entry point
    answers afterwards is the committed literal, printed by this loop on the library of the commit before the context's resources were
    owned by lifetime -- and two frames rendered then are, bit for bit, a fresh context's."""
    with capi.Context(**({"devices": [0, 0]} if group else {"device": 0})) as ctx:
        table, image = after_second_resize(ctx, demo, env)
    what = "group [0, 0]" if group else "single context"
    print(what)
    for name, answer in table.items():
        print(f"    {name!r}: {answer},")
    assert image.shape == fresh_two_frames.shape and pc.same_bits(image, fresh_two_frames), pc.describe_diff(image, fresh_two_frames)
    want = EXPECTED_AFTER_RESIZE_GROUP if group else EXPECTED_AFTER_RESIZE_SINGLE
    bad = {name: (answer, want.get(name)) for name, answer in table.items() if answer != want.get(name)}
    assert not bad and list(table) == list(want), f"{what}: (got, expected): {bad}"
