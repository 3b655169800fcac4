"""The images of a context -- textures, canvas, feature images, filtered image, variance image, moments image -- behind one read /
write / pointer path (pt_context.hip: read_plane, write_plane): what every entry point answers in every state, and a rank without rows.

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


# name -> (call, the size argument of a 16 x 16 image, one element of it); a pointer entry point takes no buffer: its "short" column is
# the ready state asked once more
ENTRY_POINTS = {
    "read_texture(output)": (_reader("mi3pt_read_texture", capi.TEX_OUTPUT), TEXELS * 4, 1),
    "read_texture(accumulation)": (_reader("mi3pt_read_texture", capi.TEX_ACCUMULATION), TEXELS * 4, 1),
    "read_texture(canvas)": (_reader("mi3pt_read_texture", capi.TEX_CANVAS), TEXELS * 4, 1),
    "read_canvas_rgba8": (_reader("mi3pt_read_canvas_rgba8"), TEXELS * 4, 4),
    "read_aov": (_reader("mi3pt_read_aov", capi.AOV_NORMAL), TEXELS * 16, 16),
    "aov_device_ptr": (_pointer("mi3pt_aov_device_ptr", capi.AOV_NORMAL), 0, 0),
    "read_guided": (_reader("mi3pt_read_guided"), TEXELS * 16, 16),
    "guided_device_ptr": (_pointer("mi3pt_guided_device_ptr"), 0, 0),
    "read_guided_variance": (_reader("mi3pt_read_guided_variance"), TEXELS, 1),
    "read_moments": (_reader("mi3pt_read_moments"), TEXELS * 16, 16),
    "write_moments": (_reader("mi3pt_write_moments"), TEXELS * 16, 16),
    "moments_device_ptr": (_pointer("mi3pt_moments_device_ptr"), 0, 0),
    "write_texture": (_reader("mi3pt_write_texture", capi.TEX_ACCUMULATION), TEXELS * 4, 1),
    "accumulation_device_ptr": (_pointer("mi3pt_accumulation_device_ptr"), 0, 0),
}
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
