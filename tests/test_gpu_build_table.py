"""Every k_raytrace_sm instantiation of the release library (tests/route_table.py: RELEASE_BUILDS, the list tests/test_route_table.py
holds the routing table to) launched once: selected through the public switches -- the kernel variant, MI3PT_OPT_SIX_WAVES (five / six
waves), MI3PT_OPT_WALK_MIN (the walk threshold of very large trees), MI3PT_OPT_LEAF_MIN (off its default: the diagnostic twin) -- on a scene
that leads there: the demo scene (no one-axis culling condition: YMAX = 0), a lone small sphere (YMAX = 1), a comb tree whose leaves must be
tested in order (the lean build of variant 4).  Each renders two frames of 40 x 24 in one launch, must equal the per-pixel kernel's
(variant 2) image bit for bit, and must report its own row through mi3pt_debug_last_launch / MI3PT_OPT_LAST_BUILD."""
import importlib.util
import os

import pytest

import ptcommon as pc
import route_table
from mi3pt_host import capi, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES = 40, 24, 2
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE


class Case:
    """a scene in the reference's layouts with the view the rows render"""

    def __init__(self, nodes, triangles, materials, direction, **camera):
        self.nodes, self.triangles, self.materials, self.direction, self.camera = nodes, triangles, materials, direction, camera
        self.compile = capi.host_scene_compile(nodes, triangles, want_eight_wide=True)
        self.reference = None           # variant 2's image, rendered once

    def camera_direction(self):
        return self.direction


@pytest.fixture(scope="module")
def cases(built, demo):
    ball = scenes.flatten_mesh(scenes.sphere_geometry(0.05, 96, 64), scenes.compose_matrix(position=(0.0, 0.4, 0.0)), 0)
    sphere = scenes.Scene(ball[0], ball[1], ball[2], [scenes.WHITE], "small sphere")
    sphere.build_bvh()
    spec = importlib.util.spec_from_file_location("culling_scenes", os.path.join(ROOT, "tests", "test_gpu_culling.py"))
    cull = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cull)
    comb_tris, comb_mats, comb_nodes = cull._comb_scene(40)
    lens = dict(focalDistance=1.0, aperture=0.0)
    return {"demo": Case(demo.nodes, demo.triangles, demo.material_bytes, demo.camera_direction(), position=demo.camera["position"], fov=demo.camera["fov"], **lens),
            "sphere": Case(sphere.nodes, sphere.triangles, sphere.material_bytes, (0.0, 0.0, -1.0), position=(0.0, 0.4, 0.3), fov=45.0, **lens),     # aimed at the sphere
            "comb": Case(comb_nodes, comb_tris, comb_mats, (0.0, 0.0, -1.0), position=(0.0, 0.0, 5.0), fov=3.0, **lens)}


def _render(ctx, case, variant):
    ctx.set_kernel_variant(variant)
    ctx.reset()
    ctx.reset_counters()
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(case, W, H, frame=2, bounces=4).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, 2).tobytes())
    ctx.submit_frames(MASK, FRAMES)
    return ctx.read_texture(capi.TEX_ACCUMULATION)


@pytest.mark.parametrize("row", list(route_table.RELEASE_BUILDS))
def test_release_build_runs_and_reports_itself(gpu_ctx, cases, env, row):
    ctx = gpu_ctx
    b = dict(zip(capi.ROUTE_BUILD, route_table.RELEASE_BUILDS[row]))
    variant = 14 if b["w8"] else 13 if b["cw"] else 10 if b["wide"] else 9 if b["cull"] else 7 if b["defer"] else 4
    case = cases["comb" if variant == 4 else "sphere" if b["ymax"] else "demo"]
    # what leads the launch to this row, from the host's compile of the scene
    c = case.compile
    assert c["analysed"] and c["cull_stack_ok"] and c["wide_ok"] and c["cwide_ok"] and c["cw8_ok"]
    assert (c["auto_wide_variant"] == 12) == bool(b["ymax"])          # (the one-axis culling condition: what `auto` = 12 means)
    assert (c["leaf_cap"] < 4) == (variant == 4)
    leaf_min = ctx.get_option(capi.OPT_LEAF_MIN)
    try:
        ctx.set_tile(0, 1, 8)
        ctx.upload_bvh(case.nodes)
        ctx.upload_triangles(case.triangles)
        ctx.upload_materials(case.materials)
        ctx.upload_environment(env)
        ctx.resize(W, H)
        if case.reference is None:
            case.reference = _render(ctx, case, 2)
            assert ctx.last_launch()["kind"] == 0
            assert 0 < ctx.counters()["hits"] < ctx.counters()["rays"]          # the view shows the scene and the sky
        ctx.set_option(capi.OPT_SIX_WAVES, int(b["waves"] == 6))
        ctx.set_option(capi.OPT_WALK_MIN, 44 if b["wmin"] == 44 else 0)
        if b["diag"]:
            ctx.set_option(capi.OPT_LEAF_MIN, 8)
        got = _render(ctx, case, 7 if variant == 4 else variant)         # (leaves that must be tested in order: 7 resolves to 4)
        assert ctx.last_launch() == dict(ctx.last_launch(), kind=1, variant=variant, lean=not b["diag"], waves_per_simd=4 if b["diag"] else b["waves"],
                                         ymax=bool(b["ymax"]), walk_min=b["wmin"])
        assert ctx.get_option(capi.OPT_LAST_BUILD) == (4 if b["diag"] else b["waves"]) | (0x100 if b["ymax"] else 0) | (b["wmin"] << 16)
        assert pc.same_bits(got, case.reference), f"{row}: " + pc.describe_diff(got, case.reference)
    finally:
        ctx.set_option(capi.OPT_SIX_WAVES, -1)
        ctx.set_option(capi.OPT_WALK_MIN, 0)
        ctx.set_option(capi.OPT_LEAF_MIN, leaf_min)
        ctx.set_kernel_variant(0)
        ctx.resize(64, 64)
