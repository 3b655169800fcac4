"""First-hit feature images (mi3pt_render_aovs) on the GPU against the oracle: every comparison is bit for bit
(ptcommon.same_bits on the float images, array_equal on the ids) -- no tolerance anywhere.  The reference is
tests/aov_reference.py (pt_oracle.camera_ray + pt_oracle.ray_scene per texel); the conditions that keep a case from passing
vacuously (shares of hits and misses, ties, aborted rays) are asserted on the reference, never on the device's output."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import aov_reference as ar
import ptcommon as pc
from mi3pt_host import capi, layout, scenes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-pathtracer_amd", "js")
NAMES = capi.AOV_NAMES


def _read_all(ctx):
    return {name: ctx.read_aov(k) for k, name in enumerate(NAMES)}


def _render(ctx, u, w, h, mask=capi.AOV_ALL, tile=(0, 1, 8)):
    ctx.set_tile(*tile)
    ctx.resize(w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, u if isinstance(u, bytes) else u.tobytes())
    ctx.render_aovs(mask)


def _shares(ref):
    inside = ref["computed"] & ref["inside"]
    n = int(inside.sum())
    hits = int((ref["hit"] & inside).sum())
    return n, hits, n - hits


def _same(a, b):
    return all(a[n].tobytes() == b[n].tobytes() for n in NAMES)


def _neg0(demo, axis):
    p = [float(v) for v in demo.camera["position"]]
    p[axis] = -0.0
    return p


# name, (w, h), rt_uniforms keywords, (least share of hits, least share of misses, least number of hits) asserted on the reference
DEMO_CASES = [
    ("64x64", (64, 64), {}, (0.15, 0.15, 0)),
    ("100x52-ragged", (100, 52), {}, (0.15, 0.15, 0)),
    ("1x1", (1, 1), {}, (0.0, 0.0, 0)),
    ("256x256", (256, 256), {}, (0.15, 0.15, 0)),
    ("64x64-resolution-31.75x47.5", (64, 64), {"res": (31.75, 47.5)}, (0.15, 0.15, 0)),
    ("64x48-looking-down", (64, 48), {"position": (0.0, 9.0, 0.0), "direction": (0.0, -1.0, 0.0)}, (0.15, 0.15, 0)),
    ("96x64-x-minus-zero", (96, 64), {"neg0": 0}, (0.15, 0.15, 0)),
    ("96x64-y-minus-zero", (96, 64), {"neg0": 1}, (0.0, 0.0, 50)),
    ("96x64-z-minus-zero", (96, 64), {"neg0": 2}, (0.0, 0.05, 0)),
]
# Both materials of the demo scene occur among the oracle's hits of every whole-image case but two, where the input itself does not
# allow it: with the eye ON the floor plane (y = -0.0) the oracle's 93 hits are all on the model (material 1), and from z = -0.0,
# inside the model's footprint, its 5 564 hits all have material 0.
ONE_MATERIAL = {"96x64-y-minus-zero": {1}, "96x64-z-minus-zero": {0}}


def _demo_uniforms(demo, w, h, kw):
    kw = dict(kw)
    if "neg0" in kw:
        kw["position"] = _neg0(demo, kw.pop("neg0"))
    u = pc.rt_uniforms(demo, w, h, **kw)
    if "position" in kw:          # (-0.0 must have survived the uniform block)
        assert np.frombuffer(u.tobytes(), np.float32, 3, 32).tobytes() == np.array(kw["position"], np.float32).tobytes()
    return u.tobytes()


@pytest.mark.parametrize("case", DEMO_CASES, ids=[c[0] for c in DEMO_CASES])
def test_demo_scene_images_match_the_oracle(gpu_ctx, orc, demo, env, case):
    """1. All four images, whole, against the helper; each mask bit alone renders the same image as all four together."""
    name, (w, h), kw, (min_hits, min_misses, min_nhits) = case
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    pc.upload_scene(ctx, demo, env)
    u = _demo_uniforms(demo, w, h, kw)
    osc = pc.oracle_scene(orc, demo, env)
    ref = ar.reference(orc, osc, u, w, h)
    n, hits, misses = _shares(ref)
    print(f"demo {name}: {n} texels inside, {hits} hits (oracle)")
    assert ref["computed"].all()
    assert hits >= min_hits * n and misses >= min_misses * n and hits >= min_nhits
    if n > 1:
        assert set(np.unique(ref["ids"][..., 1][ref["hit"]])) == ONE_MATERIAL.get(name, {0, 1}), "materials among the oracle's hits"
    _render(ctx, u, w, h)
    got = _read_all(ctx)
    ar.assert_images(pc, got, ref, name)
    ar.check_ids(orc, osc, u, got["ids"], ref, h)
    for k, nm in enumerate(NAMES):
        ctx.resize(w, h)                                  # (nothing rendered survives a resize)
        ctx.render_aovs(1 << k)
        assert ctx.read_aov(k).tobytes() == got[nm].tobytes(), f"{name}: {nm} rendered alone"
        for other in range(capi.AOV_COUNT):
            if other != k:
                with pytest.raises(capi.Mi3ptError) as e:
                    ctx.read_aov(other)
                assert e.value.code == 4


def test_sample_settings_do_not_enter(gpu_ctx, orc, demo, env):
    """2. frame, maxBounces, samplesPerFrame, aperture, focalDistance, envMapIntensity (and the rotation) changed: the same bits."""
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    pc.upload_scene(ctx, demo, env)
    w, h = 64, 64
    _render(ctx, pc.rt_uniforms(demo, w, h), w, h)
    want = _read_all(ctx)
    ref = ar.reference(orc, pc.oracle_scene(orc, demo, env), pc.rt_uniforms(demo, w, h).tobytes(), w, h)
    ar.assert_images(pc, want, ref)
    other = pc.rt_uniforms(demo, w, h, frame=77, bounces=1, spf=5, aperture=0.3, focal=2.5, intensity=3.0, rotation=1.1)
    assert other.tobytes() != pc.rt_uniforms(demo, w, h).tobytes()
    ctx.set_uniforms(capi.PASS_RAYTRACE, other.tobytes())
    ctx.render_aovs(capi.AOV_ALL)
    assert _same(_read_all(ctx), want)
    ctx.set_storage(capi.STORAGE_F16)                     # fp32 / i32 whatever the storage
    try:
        ctx.render_aovs(capi.AOV_ALL)
        assert _same(_read_all(ctx), want)
    finally:
        ctx.set_storage(capi.STORAGE_F32)


def _coincident_sheets_scene(copies=12, segments=3):
    """The tie scene of tests/test_gpu_parity.py, built the same way: `copies` coincident subdivided quads and a second, tilted
    stack crossing the first -- every hit is a tie in t, the record says which leaf the walk visited first."""
    import math
    S = scenes
    q = S.quaternion_from_axis_angle((1.0, 0.0, 0.0), -math.pi / 2)
    parts = [S.flatten_mesh(S.plane_geometry(3, 3, segments, segments), S.compose_matrix(quaternion=q), i)
             for i in range(copies)]
    q2 = S.quaternion_from_axis_angle((0.0, 0.0, 1.0), 0.6)
    parts += [S.flatten_mesh(S.plane_geometry(2, 2, segments, segments), S.compose_matrix(position=(0, 0.3, 0), quaternion=q2), i)
              for i in range(copies)]
    mats = [dict(color=(0.2 + 0.05 * i, 0.9 - 0.06 * i, 0.5), roughness=1.0, metalness=0.0, specularColor=(1, 1, 1),
                 emissive=(0.03 * (i + 1), 0.5 / (i + 1), 0.1 * (i % 3)), emissiveIntensity=1.0) for i in range(copies)]
    sc = S.Scene(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                 np.concatenate([p[2] for p in parts]), mats, "coincident sheets")
    sc.build_bvh()
    return sc


def test_ties_keep_the_first_visited_leaf_whatever_the_context_would_run(gpu_ctx, orc, env):
    """3. The coincident-sheets scene: material and triangle ids per check_ids with the culling / wide walks on and off, in the
    debug packet layout and under every kernel variant the build has -- one set of bits."""
    sc = _coincident_sheets_scene()
    ctx = gpu_ctx
    w, h = 96, 64
    u = pc.rt_uniforms(sc, w, h).tobytes()
    osc = pc.oracle_scene(orc, sc, env)
    ref = ar.reference(orc, osc, u, w, h)
    n, hits, misses = _shares(ref)
    print(f"tie scene: {n} texels, {hits} hits, materials {sorted(set(ref['ids'][..., 1][ref['hit']].tolist()))}")
    assert hits >= 0.15 * n and misses >= 0.15 * n
    census = ar.tie_census(orc, osc, u, ref, h, stride=37)
    assert len(census) >= 50
    for same_t, meets in census:
        assert same_t >= 2 and meets == 1, "every sampled hit is a tie in t that exactly one triangle resolves"
    seen = set()

    def run(what):
        pc.upload_scene(ctx, sc, env)
        _render(ctx, u, w, h)
        got = _read_all(ctx)
        ar.assert_images(pc, got, ref, what)
        ar.check_ids(orc, osc, u, got["ids"], ref, h)
        seen.add(b"".join(got[nm].tobytes() for nm in NAMES))

    try:
        ctx.set_kernel_variant(0)
        for cull, wide in ((1, 1), (0, 1), (1, 0), (0, 0)):
            ctx.set_option(capi.OPT_CULL, cull)
            ctx.set_option(capi.OPT_WIDE, wide)
            run(f"cull {cull} wide {wide}")
        ctx.set_option(capi.OPT_CULL, 1)
        ctx.set_option(capi.OPT_WIDE, 1)
        ctx.set_packet_layout(1)
        run("packet layout 1")
        # (the layout takes effect with a raytrace submit: render a frame in it, then the images again)
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
        ctx.submit(capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE)
        ctx.sync()
        ctx.render_aovs(capi.AOV_ALL)
        got = _read_all(ctx)
        ar.assert_images(pc, got, ref, "packet layout 1, applied")
        ar.check_ids(orc, osc, u, got["ids"], ref, h)
        seen.add(b"".join(got[nm].tobytes() for nm in NAMES))
        ctx.set_packet_layout(0)
        variants = pc.variants_available(ctx, (0, 1, 2, 4, 7, 9, 10, 13))
        assert len(variants) >= 6
        for v in variants:
            ctx.set_kernel_variant(v)
            run(f"variant {v}")
    finally:
        ctx.set_option(capi.OPT_CULL, 1)
        ctx.set_option(capi.OPT_WIDE, 1)
        ctx.set_packet_layout(0)
        ctx.set_kernel_variant(0)
    assert len(seen) == 1


def _chain_scene(depth):
    """tests/test_gpu_parity.py's degenerate right-deep tree, built the same way: a chain of `depth` internal nodes whose left
    children are leaves; every box is hit, so the stack grows by one per level and the walk aborts at 64 entries."""
    ntri = depth + 1
    pos = np.zeros((ntri, 3, 3))
    for i in range(ntri):
        z = -1.0 - i
        pos[i] = [[-1, -1, z], [1, -1, z], [0, 1, z]]
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (ntri, 3, 1))
    tris = layout.pack_triangles(pos, nrm, np.zeros(ntri, int))
    nodes = np.zeros(2 * ntri - 1, layout.BVH_NODE)

    def box(lo_tri, hi_tri):
        p = pos[lo_tri:hi_tri + 1].reshape(-1, 3)
        return p.min(0), p.max(0)
    idx = 0
    for k in range(depth):
        mn, mx = box(k, depth)
        nodes[idx]["min"], nodes[idx]["max"] = mn, mx
        nodes[idx]["isLeaf"] = 0
        nodes[idx]["left"], nodes[idx]["right"] = idx + 1, idx + 2
        nodes[idx]["triangleIndex"] = -1
        mn, mx = box(k, k)
        nodes[idx + 1]["min"], nodes[idx + 1]["max"] = mn, mx
        nodes[idx + 1]["isLeaf"], nodes[idx + 1]["left"], nodes[idx + 1]["right"] = 1, -1, -1
        nodes[idx + 1]["triangleIndex"] = k
        idx += 2
    mn, mx = box(depth, depth)
    nodes[idx]["min"], nodes[idx]["max"] = mn, mx
    nodes[idx]["isLeaf"], nodes[idx]["left"], nodes[idx]["right"], nodes[idx]["triangleIndex"] = 1, -1, -1, depth
    mats = layout.pack_materials([scenes.WHITE])
    return tris, mats, nodes


class _ChainCam:
    camera = dict(position=(0.0, 0.0, 5.0), fov=30.0, focalDistance=1.0, aperture=0.0)

    @staticmethod
    def camera_direction():
        return (0.0, 0.0, -1.0)


def test_best_so_far_after_the_stack_abort(gpu_ctx, orc):
    """4. The 70-deep chain: best-so-far after the 64-entry abort equals the oracle's."""
    tris, mats, nodes = _chain_scene(70)
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    ctx.upload_bvh(nodes)
    ctx.upload_triangles(tris)
    ctx.upload_materials(mats)
    w = h = 24
    u = pc.rt_uniforms(_ChainCam, w, h).tobytes()
    osc = orc.OracleScene(tris, mats, nodes)
    ref = ar.reference(orc, osc, u, w, h)
    n, hits, _ = _shares(ref)
    print(f"chain scene: {n} texels, {hits} hits, {ref['overflows']} aborted rays")
    assert hits >= 50 and ref["overflows"] >= 1
    _render(ctx, u, w, h)
    got = _read_all(ctx)
    ar.assert_images(pc, got, ref, "chain")
    ar.check_ids(orc, osc, u, got["ids"], ref, h)


def test_images_on_a_device_built_tree(gpu_ctx, orc, demo, env):
    """5. A tree from mi3pt_device_build_bvh on the demo triangles: the images equal the helper's on that tree."""
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    pc.upload_scene(ctx, demo, env)
    nodes, _ = ctx.device_build_bvh()
    ctx.upload_bvh(nodes)
    w, h = 100, 52
    u = pc.rt_uniforms(demo, w, h).tobytes()
    osc = orc.OracleScene(demo.triangles, demo.material_bytes, nodes, env)
    ref = ar.reference(orc, osc, u, w, h)
    n, hits, misses = _shares(ref)
    assert hits >= 0.15 * n and misses >= 0.15 * n
    _render(ctx, u, w, h)
    got = _read_all(ctx)
    ar.assert_images(pc, got, ref, "device-built tree")
    ar.check_ids(orc, osc, u, got["ids"], ref, h)


def test_tile_split_and_device_group(gpu_ctx, orc, demo, env):
    """6. Each rank's compact images reassemble to the whole image; a device group's read_aov returns the whole image, gathered
    directly and staged through pinned memory."""
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    pc.upload_scene(ctx, demo, env)
    w, h = 100, 52
    u = pc.rt_uniforms(demo, w, h).tobytes()
    osc = pc.oracle_scene(orc, demo, env)
    ref = ar.reference(orc, osc, u, w, h)
    _render(ctx, u, w, h)
    whole = _read_all(ctx)
    ar.assert_images(pc, whole, ref, "whole")
    try:
        for nranks, block_rows in ((2, 8), (3, 8), (3, 4)):
            seen = np.zeros(h, int)
            for rank in range(nranks):
                _render(ctx, u, w, h, tile=(rank, nranks, block_rows))
                part = _read_all(ctx)
                rows = capi.tile_local_rows(h, rank, nranks, block_rows)
                pref = ar.reference(orc, osc, u, w, h, rank, nranks, block_rows)
                ar.assert_images(pc, part, pref, f"rank {rank} of {nranks}")
                for nm in NAMES:
                    assert part[nm].shape == (rows, w, 4)
                    for ly in range(rows):
                        gy = capi.tile_global_row(ly, rank, nranks, block_rows)
                        assert part[nm][ly].tobytes() == whole[nm][gy].tobytes(), f"{nm}: rank {rank}/{nranks} row {ly} = image row {gy}"
                for ly in range(rows):
                    seen[capi.tile_global_row(ly, rank, nranks, block_rows)] += 1
            assert (seen == 1).all()
    finally:
        ctx.set_tile(0, 1, 8)
        ctx.resize(w, h)
    with capi.Context(devices=[0, 0, 0]) as g:
        pc.upload_scene(g, demo, env)
        g.resize(w, h)
        with pytest.raises(capi.Mi3ptError) as e:
            g.read_aov(capi.AOV_ALBEDO)
        assert e.value.code == 4
        g.set_uniforms(capi.PASS_RAYTRACE, u)
        g.enable_timing(True)
        g.render_aovs(capi.AOV_ALL)
        got = _read_all(g)
        assert _same(got, whole), "device group, direct gather"
        assert g.pass_time_us(capi.PASS_AOV) > 0.0
        g.set_option(capi.OPT_GATHER_STAGED, 1)
        assert g.get_option(capi.OPT_GATHER_STAGED) == 1
        assert _same(_read_all(g), whole), "device group, staged gather"
        g.render_aovs(1 << capi.AOV_POSITION)
        assert g.read_aov(capi.AOV_POSITION).tobytes() == whole["position"].tobytes()
        ptr, nbytes = g.aov_device_ptr(capi.AOV_IDS)
        assert ptr and nbytes == w * h * 16


@pytest.mark.parametrize("variant", [7, 0], ids=["reference-counter-walk", "shipped-walk"])
def test_no_trace_in_the_sample_path(gpu_ctx, demo, env, variant):
    """7. Twelve RAYTRACE | ACCUMULATE frames, pipelining on, plain and with render_aovs + read_aov after frames 1, 5 and 9:
    accumulation image, canvas bytes, counters and the final launch identical; batch_capacity untouched by the first call.

    The counters: under kernel variant 7 (the batched state-machine kernel executing exactly the reference's tests) all eight are
    compared.  Under the default walk the box- and triangle-test counters are not compared, because they are not a function of the
    job there: what the culling walk skips depends on when a lane's parked leaves are tested, which goes by the wave's other
    lanes, and the jobs reach the waves through an atomic ticket queue.  Measured on the MI355X with NO feature-image call
    anywhere, four runs of this very job on one context: box_tests 8 894 105 / 8 895 430 / 8 894 123 / 8 895 658, tri_tests
    2 177 167 / 2 177 203 / 2 177 128 / 2 177 167, the other six counters and the image equal every time (variant 7, three runs:
    13 771 623 / 2 470 035 every time).  The six counters that ARE a function of the job are compared under both walks."""
    ctx = gpu_ctx
    w = h = 256
    frames = 12

    def job(with_aovs):
        ctx.set_kernel_variant(variant)
        pc.upload_scene(ctx, demo, env)
        ctx.set_tile(0, 1, 8)
        ctx.set_pipelining(True)
        ctx.resize(w, h)
        ctx.reset_counters()
        ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(w, h).tobytes())
        cap = [ctx.batch_capacity()]
        aov = None
        for f in range(1, frames + 1):
            ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=f, bounces=4).tobytes())
            ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, f).tobytes())
            ctx.submit(capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE)
            if with_aovs and f in (1, 5, 9):
                ctx.render_aovs(capi.AOV_ALL)
                aov = _read_all(ctx)
                cap.append(ctx.batch_capacity())
        acc = ctx.read_texture(capi.TEX_ACCUMULATION)
        launch = ctx.last_launch()
        ctx.submit(capi.SUBMIT_FULLSCREEN)
        canvas = ctx.read_canvas_rgba8()
        return acc, canvas, ctx.counters(), launch, cap, aov

    try:
        plain = job(False)
        mixed = job(True)
    finally:
        ctx.set_kernel_variant(0)
    assert plain[0].tobytes() == mixed[0].tobytes(), pc.describe_diff(mixed[0], plain[0])
    assert plain[1].tobytes() == mixed[1].tobytes()
    print(f"variant {variant}: counters plain {plain[2]} with feature images {mixed[2]}")
    compared = capi.COUNTER_NAMES if variant == 7 else tuple(k for k in capi.COUNTER_NAMES if k not in pc.WALK_COUNTERS)
    assert len(compared) == (8 if variant == 7 else 6)
    for k in compared:
        assert plain[2][k] == mixed[2][k], f"counter {k}: plain {plain[2][k]}, with feature images {mixed[2][k]}"
    assert plain[2]["pixels"] == frames * w * h
    assert plain[3] == mixed[3] and plain[3]["kind"] == 1 and plain[3]["variant"] == (7 if variant == 7 else 13)
    assert len(set(mixed[4])) == 1 and mixed[4][0] == plain[4][0]
    assert mixed[5] is not None and mixed[5]["ids"][..., 2].any()


def test_states_and_errors(gpu_ctx, orc, demo, env):
    """8. The statuses of the header, and the context renders the same bits afterwards."""
    w = h = 64
    u = pc.rt_uniforms(demo, w, h).tobytes()
    ref = ar.reference(orc, pc.oracle_scene(orc, demo, env), u, w, h)

    def code(fn, *a):
        with pytest.raises(capi.Mi3ptError) as e:
            fn(*a)
        return e.value.code

    with capi.Context(0) as ctx:
        pc.upload_scene(ctx, demo, env)
        ctx.set_uniforms(capi.PASS_RAYTRACE, u)
        assert code(ctx.render_aovs, capi.AOV_ALL) == 4                  # before resize
        assert code(ctx.aov_device_ptr, capi.AOV_ALBEDO) == 4
        ctx.resize(w, h)
        assert code(ctx.read_aov, capi.AOV_NORMAL) == 4                  # read before render
        assert code(ctx.render_aovs, 0) == 1
        assert code(ctx.render_aovs, 16) == 1
        assert code(ctx.render_aovs, 31) == 1
        assert code(ctx.set_uniforms, capi.PASS_AOV, u) == 1             # no uniform block of its own
        ctx.render_aovs(1 << capi.AOV_NORMAL)
        assert code(ctx.read_aov, capi.AOV_ALBEDO) == 4                  # not this one
        assert code(ctx.read_aov, 4) == 1
        out = np.empty((h, w, 4), np.float32)
        assert ctx.lib.mi3pt_read_aov(ctx.handle, capi.AOV_NORMAL, out.ctypes.data_as(ctypes.c_void_p), out.nbytes - 16) == 1   # wrong byte count
        assert ctx.lib.mi3pt_read_aov(ctx.handle, capi.AOV_NORMAL, None, out.nbytes) == 1
        assert code(ctx.pass_time_us, capi.PASS_AOV) == 4                # timing is off
        ctx.read_aov(capi.AOV_NORMAL)
        ctx.resize(w, h)
        assert code(ctx.read_aov, capi.AOV_NORMAL) == 4                  # read after a resize without a render
        assert code(ctx.aov_device_ptr, capi.AOV_NORMAL) == 4
        # a later upload or uniform change does not alter images already rendered
        ctx.render_aovs(capi.AOV_ALL)
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, position=(0.0, 9.0, 0.0), direction=(0.0, -1.0, 0.0)).tobytes())
        ctx.upload_materials(layout.pack_materials([scenes.RED, scenes.RED]))
        got = _read_all(ctx)
        ar.assert_images(pc, got, ref, "after the errors")
        ctx.enable_timing(True)
        ctx.upload_materials(demo.material_bytes)
        ctx.set_uniforms(capi.PASS_RAYTRACE, u)
        ctx.render_aovs(capi.AOV_ALL)
        ctx.sync()
        assert ctx.pass_time_us(capi.PASS_AOV) > 0.0
        assert _same(_read_all(ctx), got)
        # a smaller resolution at a later call leaves nothing stale
        small = pc.rt_uniforms(demo, w, h, res=(31.75, 47.5)).tobytes()
        ctx.set_uniforms(capi.PASS_RAYTRACE, small)
        ctx.render_aovs(capi.AOV_ALL)
        ar.assert_images(pc, _read_all(ctx), ar.reference(orc, pc.oracle_scene(orc, demo, env), small, w, h), "smaller resolution")


@pytest.fixture(scope="module")
def dragon(built):
    sc = scenes.dragon_class_scene()          # 869,882 triangles, the benchmark's scene and view
    sc.build_bvh()
    return sc


def test_full_hd_on_the_large_scene(gpu_ctx, orc, dragon, env):
    """9. 1920 x 1080 on the 870 k-triangle scene: 20 000 seeded random texels of each image, plus image rows 0, 539 and 1079 whole."""
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    sc = dragon
    w, h = 1920, 1080
    pc.upload_scene(ctx, sc, env)
    u = pc.rt_uniforms(sc, w, h, bounces=8).tobytes()
    _render(ctx, u, w, h)
    got = _read_all(ctx)
    osc = pc.oracle_scene(orc, sc, env)
    rng = np.random.default_rng(20261016)
    pix = sorted(set(zip(rng.integers(0, h, 20000).tolist(), rng.integers(0, w, 20000).tolist())))
    assert len(pix) >= 19800
    ref = ar.reference(orc, osc, u, w, h, pixels=pix)
    n, hits, misses = _shares(ref)
    print(f"870 k triangles, 1080p: {n} sampled texels, {hits} hits (oracle)")
    assert n == len(pix) and hits >= 0.15 * n and misses >= 0.15 * n
    ar.assert_images(pc, got, ref, "1080p sample")
    ar.check_ids(orc, osc, u, got["ids"], ref, h)
    rows = ar.reference(orc, osc, u, w, h, pixels=[(y, x) for y in (0, 539, 1079) for x in range(w)])
    assert int(rows["computed"].sum()) == 3 * w
    ar.assert_images(pc, got, rows, "1080p rows 0, 539, 1079")
    ar.check_ids(orc, osc, u, got["ids"], rows, h)


def test_device_pointer_holds_the_image(gpu_ctx, demo, env):
    """10. mi3pt_aov_device_ptr: the device memory copied back with hipMemcpy equals read_aov."""
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    pc.upload_scene(ctx, demo, env)
    w, h = 100, 52
    _render(ctx, pc.rt_uniforms(demo, w, h), w, h)
    want = _read_all(ctx)
    try:
        hip = ctypes.CDLL("libamdhip64.so")
    except OSError:
        hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    ctx.sync()
    for k, nm in enumerate(NAMES):
        ptr, nbytes = ctx.aov_device_ptr(k)
        assert ptr and nbytes == w * h * 16
        host = np.empty((h, w, 4), want[nm].dtype)
        assert hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), ptr, nbytes, 2) == 0          # hipMemcpyDeviceToHost
        assert host.tobytes() == want[nm].tobytes(), nm


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_host_writes_the_feature_images(gpu_ctx, demo, env, tmp_path):
    """11. render_demo.js --aovs at 64 x 64 under Node: the three files exist, and the raw position image equals the Python
    host's read-back byte for byte (the camera block is the JS host's own, so both hosts send the same 96 bytes)."""
    node = shutil.which("node")
    env_path = tmp_path / "env.f32"
    env_path.write_bytes(env.tobytes())
    out = str(tmp_path / "demo")
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(env_path), "--width", "64", "--height", "64",
                        "--frames", "2", "--bounces", "4", "--out", out, "--aovs"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1])["status"] == "idle"
    for suffix in ("_albedo.png", "_normal.png", "_position.f32"):
        assert os.path.getsize(out + suffix) > 0, suffix
    for suffix in ("_albedo.png", "_normal.png"):
        assert open(out + suffix, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    dump = tmp_path / "scene"
    dump.mkdir()
    r = subprocess.run([node, os.path.join(JS, "tools", "dump_demo_scene.js"), str(dump)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cam = np.frombuffer((dump / "camera.bin").read_bytes(), layout.RAYTRACE_UNIFORMS)[0]
    w = h = 64
    u = pc.rt_uniforms(demo, w, h, position=[float(v) for v in cam["camera.position"]],
                       direction=[float(v) for v in cam["camera.direction"]], fov=float(cam["camera.fov"]))
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    pc.upload_scene(ctx, demo, env)
    _render(ctx, u, w, h, mask=1 << capi.AOV_POSITION)
    want = ctx.read_aov(capi.AOV_POSITION)
    assert want[..., 3].min() < 1e19                       # something was hit
    assert open(out + "_position.f32", "rb").read() == want.tobytes()
