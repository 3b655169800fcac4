"""The shipped walk's box, triangle and ray decisions ON THE DEVICE against the oracle, at the inputs where such code goes wrong
(tests/walk_probe_inputs.py; tests/test_walk_probe_inputs.py shows on the CPU that the cases are there).

mi3pt_debug_pairs calls the kernels' own device functions on one (ray, box) or (ray, triangle) pair per thread: ray_aabb,
ray_prepare, ray_aabb_pre, leaf_box_hit, slab_q0 / slab_margin / slab_hit, cwide_hit, ray_aabb_fast; ray_triangle, ray_triangle_e,
ray_triangle_flat_e.  mi3pt_debug_intersect_shipped runs the first-hit walk mi3pt_render_aovs ships (k_aov_cull's loop: compressed
wide packets, distance culling, wave votes between node and leaf steps, the leaf-rank tie rule) on rays from memory -- incoherent
within a wave, on node planes, at box corners and triangle edges, outside the fast path's guards.  No tolerance anywhere: every
comparison is bit for bit or one-sided."""
import numpy as np
import pytest

import micro_geometry as mg
import ptcommon as pc
import walk_probe_inputs as wpi
from mi3pt_host import capi

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- pairs

@pytest.fixture(scope="module")
def box_cases(orc):
    """name -> (rays, mn, mx, the oracle's answer), computed once"""
    return {name: (r, mn, mx, orc.ray_aabb_n(r, mn, mx)) for name, (r, mn, mx) in wpi.box_pairs().items()}


@pytest.fixture(scope="module")
def tri_cases(orc):
    return {name: (r, g, orc.ray_triangle_n(r, g)) for name, (r, g) in wpi.triangle_pairs().items()}


def _first(bad, r, *more):
    i = int(np.flatnonzero(bad)[0])
    return f"{int(bad.sum())} of {len(bad)}, first: pair {i} ray {r[i].tolist()} " + " ".join(str(m[i].tolist()) for m in more)


@pytest.mark.parametrize("forced_unsafe", [False, True], ids=["box_unsafe by the host's rule", "box_unsafe forced"])
def test_box_decisions_equal_the_oracle(gpu_ctx, box_cases, forced_unsafe):
    seen_fast = seen_undecided = 0
    for name, (r, mn, mx, want) in box_cases.items():
        unsafe = np.ones(len(r), bool) if forced_unsafe else wpi.box_unsafe_host(mn, mx)
        got = gpu_ctx.debug_pairs(0, r, np.concatenate([mn, mx, unsafe[:, None].astype(np.float32)], 1))
        w = want.astype(np.float32)
        for slot, fn in ((0, "ray_aabb"), (2, "ray_aabb_pre"), (3, "leaf_box_hit")):
            bad = got[:, slot] != w
            assert not bad.any(), f"{name}: {fn} differs from the oracle on " + _first(bad, r, mn, mx)
        flags = got[:, 1]
        bad = flags != wpi.ray_flags(r)
        assert not bad.any(), f"{name}: ray_prepare().flags off the documented guards on " + _first(bad, r)
        fast = (flags == 0) & ~unsafe
        assert ((got[:, 4] == -1) == ~fast).all(), f"{name}: the fast-path slots are reported exactly for flags == 0 && !box_unsafe"
        g, wf, rf = got[fast], w[fast], r[fast]
        bad = g[:, 7] != wf
        assert not bad.any(), f"{name}: ray_aabb_fast differs from the oracle on " + _first(bad, rf, mn[fast], mx[fast])
        decided = g[:, 4] == 1
        bad = decided & (g[:, 5] != wf)
        assert not bad.any(), f"{name}: slab_hit, margin > 0, differs from the oracle on " + _first(bad, rf, mn[fast], mx[fast], g)
        bad = (wf == 1) & (g[:, 6] != 1)
        assert not bad.any(), f"{name}: cwide_hit rejects a box the oracle passes on " + _first(bad, rf, mn[fast], mx[fast], g)
        seen_fast += int(fast.sum())
        seen_undecided += int((~decided).sum())
        if name == wpi.ORDINARY_BOX_FAMILY and not forced_unsafe:
            print(f"{name}: {int((~decided).sum())} of {len(g)} undecided")
            assert len(g) > len(r) // 2
            assert (~decided).sum() < wpi.UNDECIDED_BOUND * len(g), f"{int((~decided).sum())} of {len(g)} ordinary pairs undecided"
    if forced_unsafe:
        assert seen_fast == 0
    else:
        assert seen_fast > 100000 and seen_undecided > 1000          # both the deciding filter and its fallback did run


def test_triangle_decisions_equal_the_oracle(gpu_ctx, tri_cases):
    for name, (r, g, want) in tri_cases.items():
        got = gpu_ctx.debug_pairs(1, r, g)
        hit = want[:, 0] == 1
        for k, fn in ((0, "ray_triangle"), (4, "ray_triangle_e"), (8, "ray_triangle_flat_e")):
            bad = got[:, k] != want[:, 0]
            assert not bad.any(), f"{name}: {fn} hit flag differs from the oracle on " + _first(bad, r, g, want, got)
            tuv = got[:, k + 1:k + 4]
            bad = hit & (tuv.view(np.uint32) != want[:, 1:4].view(np.uint32)).any(1)
            assert not bad.any(), f"{name}: {fn} t, u, v differ from the oracle's bits on " + _first(bad, r, g, want, got)


# ---------------------------------------------------------------- rays against scenes

@pytest.fixture(scope="module")
def scene_cases():
    return wpi.scenes()


SCENE_NAMES = ("demo", "slivers", "tiny next to huge", "sphere", wpi.TIE_SCENE, "comb 40", "demo x 2^-6", "demo x 2^6",
               "demo + (1000, 1000, 1000)", "demo, broken boxes") + mg.SCENES


def _upload(ctx, nodes, tris, mats, env):
    ctx.set_kernel_variant(0)
    ctx.upload_bvh(nodes)
    ctx.upload_triangles(tris)
    ctx.upload_materials(mats)
    ctx.upload_environment(env)


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_every_walk_equals_the_oracle_ray_for_ray(gpu_ctx, orc, env, scene_cases, scene):
    assert sorted(scene_cases) == sorted(SCENE_NAMES)
    nodes, tris, mats = scene_cases[scene]
    ctx = gpu_ctx
    _upload(ctx, nodes, tris, mats, env)
    fam = wpi.scene_rays_of(scene, nodes, tris)
    names = list(fam)
    rays = np.concatenate([fam[k] for k in names])
    owner = np.concatenate([np.full(len(fam[k]), i) for i, k in enumerate(names)])
    want, cnt = orc.ray_scene_n(orc.OracleScene(tris, mats, nodes), rays)

    def check(got, what, n=None):
        n = len(rays) if n is None else n
        bad = ~((got[:, :9].view(np.uint32) == want[:n].view(np.uint32)) | (np.isnan(got[:, :9]) & np.isnan(want[:n]))).all(1)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{scene}, {what}: {int(bad.sum())} of {n} rays differ from the oracle; first: ray {i} ({names[owner[i]]}) "
                                 f"{rays[i].tolist()} gpu {got[i].tolist()} oracle {want[i].tolist()}")

    try:
        for variant in (1, 2, 4):
            ctx.set_kernel_variant(variant)
            check(ctx.debug_intersect(rays), f"debug_intersect, variant {variant}")
        ctx.set_kernel_variant(0)
        if scene in wpi.SHIPPED_WALK_REFUSED:
            # boxes that do not bound: mi3pt_render_aovs does not run the shipped walk there, and the probe must say so
            with pytest.raises(capi.Mi3ptError, match="would not run the shipped first-hit walk") as e:
                ctx.debug_intersect_shipped(rays)
            assert e.value.code == 4          # MI3PT_ERR_STATE
            return
        got = ctx.debug_intersect_shipped(rays)
        check(got, "debug_intersect_shipped")
        # a leaf whose own box passes is a triangle the reference tests: never more of them than the reference's count
        over = got[:, 10] > cnt[:, 1]
        assert not over.any(), f"{scene}: the shipped walk passes more leaves than the oracle tests triangles on ray {int(np.flatnonzero(over)[0])}"
        assert (got[:, 11] == 0).all() and (got[:, 9] >= 0).all()
        assert got[:, 9].max() > 0 and got[:, 10].max() > 0            # the counted walk did walk
        # ray counts around one wave (lanes beyond n vote and do nothing), from the incoherent family
        for n in wpi.WAVE_COUNTS:
            check(ctx.debug_intersect_shipped(rays[:n]), f"debug_intersect_shipped, n = {n}", n)
    finally:
        ctx.set_kernel_variant(0)


def test_the_shipped_probe_refuses_what_render_aovs_would_not_run(gpu_ctx, env, scene_cases):
    """Never another walk in the shipped one's place: with distance culling or the wide walk switched off the probe is a state error."""
    nodes, tris, mats = scene_cases["demo"]
    ctx = gpu_ctx
    _upload(ctx, nodes, tris, mats, env)
    rays = wpi.scene_rays(nodes, tris)["incoherent"][:64]
    ctx.debug_intersect_shipped(rays)
    for opt in (capi.OPT_CULL, capi.OPT_WIDE):
        ctx.set_option(opt, 0)
        try:
            with pytest.raises(capi.Mi3ptError, match="would not run the shipped first-hit walk"):
                ctx.debug_intersect_shipped(rays)
        finally:
            ctx.set_option(opt, 1)
    ctx.debug_intersect_shipped(rays)
