"""The scene compile (csrc/pt_host_compile.cpp: what mi3pt_upload_bvh, mi3pt_upload_triangles and a context's lazy scene analysis hand
to the device) through its host-only entry point, mi3pt_host_scene_compile, against tests/golden/scene_compile_digests.json: every scalar
the compile decides -- counts, flags, stack bounds, the walk `auto` means, the bits of cull_ka / cull_kb -- and one FNV-1a digest per device
buffer, as computed by the code of THE COMMIT BEFORE THE COMPILE MOVED OUT OF pt_context.hip: each host vector hashed at the moment it was
handed to replace_buffer, the node packets after the cull words were patched in.  Every field must be equal: these bytes decide whether
every image stays bit-identical and which kernel runs.  No GPU needed.

How the rows were recorded (profiles/scene_compile_move.log): from that commit's source text -- the bodies of tri_packet_of, child_ref,
build_packets, round_up_16, prepare_cull and the analysis halves of the two uploads, cut out of its pt_context.hip by a script and compiled
for the CPU around a stub context (read-backs = copies of the uploaded bytes, launch_patch_cull = the same assignment on the host).  They
have NOT yet been recorded from that commit's context on an MI355X host, which is what the change asked for: log2 feeds a ceil in the
grid-cell choice, so the rows could in principle differ with the host's libm.  A row that differs there is a finding about that scene
(replace it), not a reason to relax the comparison.

The scenes are small and reach every branch: the demo scene; two soups with triangles outside the weight analysis (weights +inf);
the demo tree with boxes that do not bound (nesting fails: no compressed packets, no 8-wide ones); a sphere (pole residues outside the
fast slab test's range); one- and two-triangle scenes; comb trees on both sides of the culling walks' stack bound; a
tree whose leaf names a triangle that was not uploaded (the analysis declines)."""
import importlib.util
import json
import os

import numpy as np
import pytest

from mi3pt_host import capi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_compile_digests.json")
CONFIGS = [(c, o, w) for c in (-1, 0, 1) for o in (0, 1, 2) for w in (0, 1)]       # MI3PT_OPT_COLLAPSE x MI3PT_OPT_PACKET_ORDER x variant 14 selected
COMB_DEPTHS = (40, 53, 54, 55, 56)          # the culling walks' stack: depth + 1 against SM_CULL_STACK_MAX = 56


def config_key(collapse, order, eight):
    return f"collapse{collapse}_order{order}_eight{eight}"


def scene_cases():
    """name -> (nodes, triangles), in the reference's layouts."""
    spec = importlib.util.spec_from_file_location("culling_scenes", os.path.join(ROOT, "tests", "test_gpu_culling.py"))
    cull = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cull)
    cases = {}
    demo = scenes.demo_scene()
    demo.build_bvh()
    cases["demo"] = (demo.nodes, demo.triangles)
    for name in ("tiny next to huge", "slivers"):
        sc = cull._soup(**dict(cull.SOUPS[name], n=2000))
        cases[name] = (sc.nodes, sc.triangles)
    # (test_boxes_that_do_not_bound_their_triangles_are_never_skipped)
    raw = demo.nodes.view(np.uint8).reshape(len(demo.nodes), 48).copy()
    f = raw.view(np.float32).reshape(len(demo.nodes), 12)
    rng = np.random.default_rng(5)
    pick = rng.choice(np.arange(1, len(demo.nodes)), 400, replace=False)
    f[pick, 0:3] += rng.uniform(0.0, 0.05, (400, 3)).astype(np.float32)
    f[pick, 4:7] += rng.uniform(-0.02, 0.05, (400, 3)).astype(np.float32)
    cases["boxes that do not bound"] = (raw.view(demo.nodes.dtype).reshape(len(demo.nodes)), demo.triangles)
    ball = scenes.flatten_mesh(scenes.sphere_geometry(0.4, 24, 16), scenes.compose_matrix(position=(0.0, 0.4, 0.0)), 0)
    sphere = scenes.Scene(ball[0], ball[1], ball[2], [scenes.WHITE], "sphere")
    sphere.build_bvh()
    cases["sphere"] = (sphere.nodes, sphere.triangles)
    rng = np.random.default_rng(8)
    for n in (1, 2):
        sc = scenes.Scene(rng.normal(size=(n, 3, 3)), np.tile(np.array([0.0, 0.0, 1.0]), (n, 3, 1)), np.zeros(n, int), [scenes.WHITE], f"soup-{n}")
        sc.build_bvh()
        cases[f"{n} triangle{'s' if n > 1 else ''}"] = (sc.nodes, sc.triangles)
    for depth in COMB_DEPTHS:
        tris, _, nodes = cull._comb_scene(depth)
        cases[f"comb {depth}"] = (nodes, tris)
    beyond = demo.nodes.copy()
    leaf = int(np.flatnonzero(beyond["isLeaf"] == 1)[7])
    beyond["triangleIndex"][leaf] = len(demo.triangles) + 5
    cases["leaf beyond the triangles"] = (beyond, demo.triangles)
    return cases


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_scene_compile_equals_the_recorded_context(built, golden):
    assert golden["fields"] == list(capi.SCENE_COMPILE_FIELDS)
    cases = scene_cases()
    assert sorted(golden["cases"]) == sorted(cases)
    seen = {k: set() for k in ("analysed", "wide_ok", "cwide_ok", "cw8_ok", "cull_stack_ok", "auto_wide_variant")}
    for name, (nodes, tris) in cases.items():
        assert sorted(golden["cases"][name]) == sorted(config_key(*c) for c in CONFIGS)
        for collapse, order, eight in CONFIGS:
            got = capi.host_scene_compile(nodes, tris, collapse, order, bool(eight))
            want = dict(zip(golden["fields"], golden["cases"][name][config_key(collapse, order, eight)]))
            diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
            assert not diff, f"{name} {config_key(collapse, order, eight)}: (got, recorded) {diff}"
            for k in seen:
                seen[k].add(got[k])
    # the scenes do reach both sides of every decision
    for k in ("analysed", "wide_ok", "cwide_ok", "cw8_ok", "cull_stack_ok"):
        assert seen[k] == {0, 1}, (k, seen[k])
    assert len(seen["auto_wide_variant"]) > 1


def test_scene_compile_refuses_what_an_upload_refuses(built):
    demo = scenes.demo_scene()
    demo.build_bvh()
    bad = demo.nodes.copy()
    bad["left"][0] = 0
    with pytest.raises(capi.Mi3ptError, match="BVH child index must be greater than its parent's"):
        capi.host_scene_compile(bad, demo.triangles)
    bad = demo.nodes.copy()
    bad["triangleIndex"][int(np.flatnonzero(bad["isLeaf"] == 1)[0])] = -2
    with pytest.raises(capi.Mi3ptError, match="leaf node with negative triangleIndex"):
        capi.host_scene_compile(bad, demo.triangles)
    tris = demo.triangles.copy()
    tris["materialIndex"][3] = -1
    with pytest.raises(capi.Mi3ptError, match="triangle with negative materialIndex"):
        capi.host_scene_compile(demo.nodes, tris)
    with pytest.raises(capi.Mi3ptError, match="bad argument"):
        capi.host_scene_compile(demo.nodes, demo.triangles, collapse=2)
