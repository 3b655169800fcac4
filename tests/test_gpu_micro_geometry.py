"""The walks on micro-geometry (tests/micro_geometry.py): packets that are tiny and close to the origin, seen from far away, where the box
test of the compressed-packet walks accepts EMPTY child slots (PROOFS.md 4a; tests/test_packet_walk_reference.py shows on the CPU that
these scenes put thousands of rays there).  The 4-ary walk (variant 13) then pushes an empty entry; the 8-wide walk (variant 14) must keep
the slot out of its hit masks by the packet's occupancy mask -- without it the slot reads as a leaf and the triangle step indexes a record
of another packet or behind the records.  Every walk against the oracle's frames: the same bits, the same paths, never a triangle test the
reference does not make, and the walk that was asked for is the walk that ran.

tri_tests is held to `<=` the oracle's, not to equality: a distance-culling walk skips leaves that lie behind the closest hit (their own
box would pass), so equality does not hold for variant 13 on the demo scene either (tests/test_gpu_parity.py compares it the same way)."""
import numpy as np
import pytest

import micro_geometry as mg
import ptcommon as pc
from mi3pt_host import capi

pytestmark = pytest.mark.gpu

W, H, FRAMES, BOUNCES = 64, 48, (2, 3), 4
VARIANTS = (2, 9, 10, 13, 14, 0)
RAN = {2: (0, 2), 9: (1, 9), 10: (1, 10), 13: (1, 13), 14: (1, 14), 0: (1, 13)}      # requested -> (kind, variant) of the launch; auto ships 13


def _uniforms(sc, w, h, frame, aperture, view):
    return pc.rt_uniforms(sc, w, h, frame=frame, bounces=BOUNCES, aperture=aperture, focal=sc.camera["focalDistance"], **mg.views(sc)[view])


def _oracle(orc, sc, env, w, h, aperture, view):
    osc = pc.oracle_scene(orc, sc, env)
    mean = np.zeros((h, w, 4), np.float32)
    total = {}
    for f in FRAMES:
        img, cnt = orc.raytrace(osc, _uniforms(sc, w, h, f, aperture, view).tobytes(), w, h)
        mean = orc.accumulate(pc.acc_uniforms(w, h, f).tobytes(), w, h, img, mean)
        for k, v in cnt.items():
            total[k] = total.get(k, 0) + v
    return mean, total


def _render(ctx, sc, w, h, aperture, view, variant):
    ctx.set_kernel_variant(variant)
    ctx.reset()
    ctx.reset_counters()
    for f in FRAMES:
        pc.gpu_frame(ctx, _uniforms(sc, w, h, f, aperture, view), pc.acc_uniforms(w, h, f), capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE)
    return ctx.read_texture(capi.TEX_ACCUMULATION), ctx.counters()


def _check(ctx, sc, w, h, aperture, view, variant, want, ocnt, what):
    ctx.set_kernel_variant(variant)
    kind, ran = RAN[variant]
    assert ctx.active_variant() == ran, f"{what}: asked for {variant}, the context would run {ctx.active_variant()}"
    got, cnt = _render(ctx, sc, w, h, aperture, view, variant)
    launch = ctx.last_launch()
    assert (launch["kind"], launch["variant"]) == (kind, ran), f"{what}: {launch}"
    assert pc.same_bits(got, want), f"{what}: " + pc.describe_diff(got, want)
    pc.check_counters(cnt, ocnt, culled=variant != 2, what=what)


@pytest.mark.parametrize("aperture", [0.0, 0.05])
@pytest.mark.parametrize("view", ["whole", "close-up"])
@pytest.mark.parametrize("scene", mg.SCENES)
def test_every_walk_renders_the_oracles_frames_on_micro_geometry(gpu_ctx, orc, env, scene, view, aperture):
    """view: micro_geometry.views -- the whole scene, and the close-up of one cluster whose camera rays pass that cluster's packets within
    5e-6 from 5 units away: 18 % of its un-jittered rays accept an empty slot in both walks (tests/test_packet_walk_reference.py)"""
    sc = mg.scene(scene)
    ctx = gpu_ctx
    # the host check first: no record index the 8-wide triangle step can form leaves the records, with either grouping
    for greedy in (False, True):
        assert capi.host_eight_wide_check(sc.nodes, sc.triangles, greedy)["offered"]
    want, ocnt = _oracle(orc, sc, env, W, H, aperture, view)
    assert 0 < ocnt["hits"] < ocnt["rays"] and ocnt["stack_overflows"] == 0
    pc.upload_scene(ctx, sc, env)
    ctx.set_storage(capi.STORAGE_F32)
    ctx.set_tile(0, 1, 8)
    ctx.resize(W, H)
    try:
        for collapse in (0, 1):
            ctx.set_option(capi.OPT_COLLAPSE, collapse)
            for variant in VARIANTS:
                _check(ctx, sc, W, H, aperture, view, variant, want, ocnt, f"{scene}, {view}, aperture {aperture}, collapse {collapse}, variant {variant}")
    finally:
        ctx.set_option(capi.OPT_COLLAPSE, -1)
        ctx.set_kernel_variant(0)
        ctx.resize(64, 64)


@pytest.mark.parametrize("size", [(1, 1), (13, 5)], ids=["1 ray", "65 rays"])
def test_tail_scene_eight_wide_with_lanes_beyond_the_last_ray(gpu_ctx, orc, env, size):
    """the scene whose last record-owning packet has leaves in its lowest slots only (build_cw8's records end behind them), one camera
    ray and one wave + one ray: the lanes beyond n vote and do nothing"""
    w, h = size
    sc = mg.scene("tail")
    ctx = gpu_ctx
    assert capi.host_eight_wide_check(sc.nodes, sc.triangles)["offered"]
    pc.upload_scene(ctx, sc, env)
    ctx.set_storage(capi.STORAGE_F32)
    ctx.set_tile(0, 1, 8)
    ctx.resize(w, h)
    try:
        for view in ("close-up", "whole"):
            for aperture in (0.0, 0.05):
                want, ocnt = _oracle(orc, sc, env, w, h, aperture, view)
                assert ocnt["pixels"] == w * h * len(FRAMES) and ocnt["hits"] > 0
                for variant in (14, 13):
                    _check(ctx, sc, w, h, aperture, view, variant, want, ocnt, f"tail {w} x {h}, {view}, aperture {aperture}, variant {variant}")
    finally:
        ctx.set_kernel_variant(0)
        ctx.resize(64, 64)
