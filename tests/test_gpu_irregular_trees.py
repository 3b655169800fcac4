"""Irregular BVHs (tests/irregular_trees.py; tests/test_irregular_trees.py shows on the CPU that each case is what it says and can be
told from the builder's tree) ON THE DEVICE: every walk renders the oracle's bits on the oracle's paths, the context resolves every
requested walk to the one the tree's shape admits (pick_variant restated here from the flags mi3pt_host_scene_compile reports), and
nothing derived from one tree survives the upload of the next.  Per-ray probes, first-hit feature images, the sky-tile split, a device
group, a context without any BVH, and the uploads that must be refused.  No tolerance anywhere: bit for bit, counter for counter.

No tree that fails irregular_trees.precondition_violations is ever rendered."""
import numpy as np
import pytest

import aov_reference as ar
import irregular_trees as it
import ptcommon as pc
from mi3pt_host import capi

pytestmark = pytest.mark.gpu

SIZES = ((64, 48), (50, 36))            # whole tiles, and ragged in both directions
FRAMES = (2, 3)
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
VARIANTS = (0, 1, 2, 4, 7, 9, 10, 13, 14)
CASES = sorted(it.CASE_NAMES)
EXACT_WIDE = (10, 11, 12)                # the exact-packet wide walks: release builds carry 10; the experiment build picks among them by the scene
DEMO = "the builder's demo tree"
ERR_INVALID, ERR_STATE = 1, 4
NOT_SHIPPED = "would not run the shipped first-hit walk"


def scene_of(name):
    if name == DEMO:
        d = it.demo()
        return d.nodes, d.triangles, d.material_bytes, it.DEMO_VIEW
    return it.cases()[name]


@pytest.fixture(scope="module")
def flags(built):
    """(case, the 8-wide packets asked for) -> what the scene compile decides, computed once"""
    cache = {}

    def get(name, eight=False):
        if (name, eight) not in cache:
            nodes, tris, _, _ = scene_of(name)
            cache[(name, eight)] = capi.host_scene_compile(nodes, tris, want_eight_wide=eight)
        return cache[(name, eight)]
    return get


def expected_variant(requested, f):
    """pick_variant (csrc/pt_ctx_launch.hip) from the compile's flags, for a context with its default options: the walk a requested
    variant resolves to.  f: host_scene_compile's fields, with the 8-wide packets asked for when 14 is requested."""
    defer = f["leaf_cap"] >= 4                                   # leaves may be tested out of order: a proper tree, room in LDS
    cull = bool(f["cull_stack_ok"] and f["analysed"])            # the near-first walks: their stack bound holds and the analysis ran
    wide = cull and bool(f["wide_ok"])
    in_order = 7 if defer else 4
    if requested == 0:
        return (13 if f["cwide_ok"] else 10) if wide else (9 if cull else in_order)
    if requested == 14 and cull and f["cw8_ok"]:
        return 14
    if requested in (13, 14):
        return 13 if wide and f["cwide_ok"] else (10 if wide else (9 if cull else in_order))
    if requested == 10:
        return 10 if wide else (9 if cull else in_order)
    if requested == 9:
        return 9 if cull else in_order
    if requested == 7:
        return in_order
    return requested


def is_walk(ran, expected):
    """`ran` is the walk `expected` names; where that is the exact-packet wide walk, any of its three forms (the same bits)"""
    return ran in EXACT_WIDE if expected == 10 else ran == expected


@pytest.fixture(scope="module")
def want(orc, env):
    """(scene name, width, height, fp16 storage, tile split, frames) -> the oracle's running mean and summed counters, computed once"""
    cache = {}

    def get(name, w, h, f16=False, tile=(0, 1, 8), frames=FRAMES, scene=None):
        key = (name, w, h, f16, tile, tuple(frames))
        if key not in cache:
            nodes, tris, mats, cam = scene if scene is not None else scene_of(name)
            osc = orc.OracleScene(tris, mats, nodes, env)
            acc = np.zeros((capi.tile_local_rows(h, *tile), w, 4), np.float32)
            total = dict.fromkeys(capi.COUNTER_NAMES, 0)
            for f in frames:
                img, cnt = orc.raytrace(osc, it.uniforms(cam, w, h, frame=f).tobytes(), w, h, *tile, store_f16=f16)
                acc = orc.accumulate(pc.acc_uniforms(w, h, f).tobytes(), w, h, img, acc, *tile, store_f16=f16)
                for k in total:
                    total[k] += cnt[k]
            assert total["stack_overflows"] == 0 and 0 < total["hits"] < total["rays"]
            cache[key] = (acc, total)
        return cache[key]
    return get


def upload(ctx, scene, env=None):
    nodes, tris, mats, _ = scene
    ctx.upload_bvh(nodes)
    ctx.upload_triangles(tris)
    ctx.upload_materials(mats)
    if env is not None:
        ctx.upload_environment(env)


def render(ctx, cam, w, h, frames=FRAMES, per_call=None):
    """`frames` consecutive frames, batched `per_call` at a time, from a zeroed mean: (mean, counters, the last launch)"""
    ctx.reset()
    ctx.reset_counters()
    per_call = per_call or len(frames)
    for k in range(0, len(frames), per_call):
        ctx.set_uniforms(capi.PASS_RAYTRACE, it.uniforms(cam, w, h, frame=frames[k]).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, frames[k]).tobytes())
        ctx.submit_frames(MASK, min(per_call, len(frames) - k))
        ctx.flush()
    return ctx.read_texture(capi.TEX_ACCUMULATION), ctx.counters(), ctx.last_launch()


@pytest.fixture(autouse=True)
def restored(gpu_ctx):
    """whatever a test of this file changes on the session's context is put back, pass or fail"""
    try:
        yield
    finally:
        ctx = gpu_ctx
        ctx.set_kernel_variant(0)
        ctx.set_storage(capi.STORAGE_F32)
        ctx.set_tile(0, 1, 8)
        ctx.set_option(capi.OPT_SIX_WAVES, -1)
        ctx.set_option(capi.OPT_WALK_MIN, 0)
        ctx.set_option(capi.OPT_SKY_TILES, 1)
        ctx.resize(64, 64)


def check_walks(ctx, name, want, flags, w, h, f16=False, tile=(0, 1, 8)):
    _, _, _, cam = scene_of(name)
    ref, ocnt = want(name, w, h, f16, tile)
    resolved = {}
    for v in pc.variants_available(ctx, VARIANTS):
        ctx.set_kernel_variant(v)
        active = ctx.active_variant()
        assert is_walk(active, expected_variant(v, flags(name, v == 14))), f"{name}: variant {v} resolves to {active}"
        got, cnt, launch = render(ctx, cam, w, h)
        what = f"{name} {w}x{h} variant {v} -> {active}"
        assert is_walk(launch["variant"], active) and (launch["lean"] or active not in (13, 14)), f"{what}: the launch ran {launch}"
        assert pc.same_bits(got, ref), f"{what}: " + pc.describe_diff(got, ref)
        pc.check_counters(cnt, ocnt, culled=active >= 9, what=what)       # (1, 2, 4, 7: all seven counters exact)
        resolved[v] = active
    ctx.set_kernel_variant(0)
    return resolved


@pytest.mark.parametrize("name", CASES)
def test_every_walk_renders_the_oracles_bits_and_is_the_walk_the_tree_admits(gpu_ctx, env, want, flags, name):
    ctx = gpu_ctx
    upload(ctx, scene_of(name), env)
    for w, h in SIZES:
        ctx.resize(w, h)
        resolved = check_walks(ctx, name, want, flags, w, h)
    print(f"{name}: requested -> ran {resolved}")
    f = flags(name)
    if not f["tree_proper"]:
        assert set(resolved.values()) <= {1, 2, 4}            # nothing but the reference's own order
    if name == "leaf root":
        assert resolved[0] == 7                                # the one-triangle start of k_raytrace_sm
    if name in it.UNREACHABLE + it.BUILDER_MADE:
        assert resolved[0] == 13
    if name.startswith("bad boxes"):
        assert resolved[0] in EXACT_WIDE                       # the exact wide packets: no grid holds a NaN


@pytest.mark.parametrize("name", ["shared subtrees", "bad boxes", "leaf root"])
def test_fp16_storage_and_a_rank_of_a_three_way_split(gpu_ctx, env, want, flags, name):
    ctx = gpu_ctx
    upload(ctx, scene_of(name), env)
    ctx.set_storage(capi.STORAGE_F16)
    ctx.set_tile(1, 3, 8)
    for w, h in SIZES:
        ctx.resize(w, h)
        check_walks(ctx, name, want, flags, w, h, f16=True, tile=(1, 3, 8))


@pytest.mark.parametrize("six,walk_min", [(0, 0), (1, 0), (1, 44), (0, 44)], ids=["five-waves", "six-waves", "six-waves-deep-build", "five-waves-deep-build"])
def test_the_six_wave_and_deep_walk_builds_of_the_shipped_walk(gpu_ctx, env, want, flags, six, walk_min):
    ctx = gpu_ctx
    names = [n for n in CASES if expected_variant(0, flags(n)) == 13]
    assert set(it.UNREACHABLE + it.BUILDER_MADE) <= set(names)
    w, h = SIZES[0]
    for name in names:
        upload(ctx, scene_of(name), env)
        ctx.resize(w, h)
        ctx.set_option(capi.OPT_SIX_WAVES, six)
        ctx.set_option(capi.OPT_WALK_MIN, walk_min)
        got, cnt, launch = render(ctx, scene_of(name)[3], w, h)
        print(f"{name}: {launch}")
        assert launch["variant"] == 13 and launch["lean"] and launch["waves_per_simd"] == (6 if six else 5), launch
        assert launch["walk_min"] == (44 if walk_min else 32), launch
        ref, ocnt = want(name, w, h)
        assert pc.same_bits(got, ref), f"{name}: " + pc.describe_diff(got, ref)
        pc.check_counters(cnt, ocnt, culled=True, what=name)


def probe_rays(nodes, n=208, seed=3):
    """rays at the leaves' boxes: from the camera and from all around, at the centre of a leaf's box and a little beside it"""
    rng = np.random.default_rng(seed)
    leaves = np.flatnonzero(nodes["isLeaf"] == 1)
    pick = rng.choice(leaves, n, replace=len(leaves) < n)
    with np.errstate(invalid="ignore"):
        centre = (nodes["min"][pick].astype(np.float64) + nodes["max"][pick]) / 2
    bad = ~np.isfinite(centre).all(1)
    centre[bad] = rng.normal(size=(int(bad.sum()), 3)) * 0.5 + (0.0, 0.5, 0.0)
    centre = np.where(np.abs(centre) < 20.0, centre, 0.0)
    centre += rng.normal(size=(n, 3)) * 0.01 * (rng.random(n) < 0.5)[:, None]
    origin = np.tile(np.array([0.0, 1.0, 4.0]), (n, 1))
    around = rng.normal(size=(n // 2, 3))
    origin[: n // 2] = 5.0 * around / np.linalg.norm(around, axis=1)[:, None] + (0.0, 0.5, 0.0)
    d = centre - origin
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.concatenate([origin, d], 1).astype(np.float32)


def check_probe(got, hit, cnt, what, counts=True):
    bad = ~((got[:, :9].view(np.uint32) == hit.view(np.uint32)) | (np.isnan(got[:, :9]) & np.isnan(hit))).all(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(hit)} hit records differ from the oracle's; first: ray {i}, gpu {got[i, :9].tolist()} "
                             f"oracle {hit[i].tolist()}")
    if counts:
        for k, which in enumerate(("box tests", "triangle tests", "stack overflows")):
            bad = got[:, 9 + k].astype(np.uint64) != cnt[:, k]
            assert not bad.any(), f"{what}: {which} differ on {int(bad.sum())} rays, first: ray {int(np.flatnonzero(bad)[0])} " \
                                  f"gpu {got[bad][0, 9 + k]} oracle {cnt[bad][0, k]}"


def test_normalize_keeps_the_sign_of_a_zero_component(gpu_ctx):
    """The kernels' normalize keeps the sign of a zero component, as the reference's division does: a vertex normal (-0, 1, 0) is
    (-0, 1, 0) in the hit record.  mi3pt_debug_math 13 .. 15 (x / y / z of normalize(a, b, a - b)) against numpy's division, compared
    by bit pattern (== cannot tell -0 from +0)."""
    rng = np.random.default_rng(31)
    a = rng.normal(size=4096).astype(np.float32)
    b = rng.normal(size=4096).astype(np.float32)
    a[0::4] = -0.0                                       # x = -0
    b[1::4] = -0.0                                       # y = -0
    b[2::4] = a[2::4]                                    # z = +0
    a[3::8], b[3::8] = -0.0, 1.0                         # x = -0, z = -1
    c = a - b
    length = np.sqrt((a * a + b * b) + c * c)
    seen = 0
    for fn, comp in ((13, a), (14, b), (15, c)):
        want = comp / length
        got = gpu_ctx.debug_math(fn, a, b)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), fn
        seen += int((np.signbit(want) & (want == 0)).sum())
    assert seen >= 2048


@pytest.mark.parametrize("name", CASES)
def test_probes_and_feature_images(gpu_ctx, orc, env, flags, name):
    nodes, tris, mats, cam = scene_of(name)
    ctx = gpu_ctx
    upload(ctx, scene_of(name), env)
    osc = orc.OracleScene(tris, mats, nodes, env)
    rays = probe_rays(nodes)
    hit, cnt = orc.ray_scene_n(osc, rays)
    assert (hit[:, 0] == 1).sum() > 20          # aimed at leaf boxes: most rays do reach triangles
    for v in (1, 2, 4):
        ctx.set_kernel_variant(v)
        check_probe(ctx.debug_intersect(rays), hit, cnt, f"{name}: debug_intersect, variant {v}")
    ctx.set_kernel_variant(0)
    if expected_variant(0, flags(name)) == 13:
        got = ctx.debug_intersect_shipped(rays)
        check_probe(got, hit, cnt, f"{name}: debug_intersect_shipped", counts=False)
        assert (got[:, 10] <= cnt[:, 1]).all() and (got[:, 11] == 0).all()
    else:
        with pytest.raises(capi.Mi3ptError, match=NOT_SHIPPED) as e:
            ctx.debug_intersect_shipped(rays)
        assert e.value.code == ERR_STATE
    # first-hit feature images (most of these trees take k_aov's walk of the uploaded tree, not the shipped one)
    w, h = SIZES[1]
    ctx.resize(w, h)
    u = it.uniforms(cam, w, h).tobytes()
    ctx.set_uniforms(capi.PASS_RAYTRACE, u)
    ctx.render_aovs(capi.AOV_ALL)
    got = {nm: ctx.read_aov(k) for k, nm in enumerate(capi.AOV_NAMES)}
    ref = ar.reference(orc, osc, u, w, h)
    assert ref["overflows"] == 0 and w * h // 10 <= ref["hit"].sum() < w * h
    ar.assert_images(pc, got, ref, name)
    ar.check_ids(orc, osc, u, got["ids"], ref, h)


def test_the_sky_tile_split_on_equals_off(gpu_ctx, env, want, flags):
    """Tiles whose camera rays can reach no node of the tree's cut are shaded by a streaming kernel once the camera has stood still for
    a launch.  A NaN, infinite or inverted box anywhere must make the cut decline (or stay right): same bits, same paths."""
    ctx = gpu_ctx
    w, h = SIZES[0]
    frames = tuple(range(2, 8))
    proper = [n for n in CASES if flags(n)["tree_proper"]]
    assert len(proper) >= 8
    split = 0
    for name in proper:
        nodes, tris, mats, cam = scene_of(name)
        upload(ctx, scene_of(name), env)
        ctx.resize(w, h)
        ref, ocnt = want(name, w, h, frames=frames)
        runs = {}
        for on in (0, 1):
            ctx.set_option(capi.OPT_SKY_TILES, on)
            runs[on] = render(ctx, cam, w, h, frames, per_call=2)
            assert pc.same_bits(runs[on][0], ref), f"{name}, sky tiles {on}: " + pc.describe_diff(runs[on][0], ref)
            pc.check_counters(runs[on][1], ocnt, culled=runs[on][2]["variant"] >= 9, what=f"{name}, sky tiles {on}")
        empty = int(capi.host_sky_tiles(nodes, it.uniforms(cam, w, h).tobytes(), w, h).sum())
        if name.startswith("bad boxes"):
            assert empty == 0, f"{name}: {empty} tiles called empty behind boxes that are none"
        split += empty > 0 and runs[1][1]["box_tests"] < runs[0][1]["box_tests"]
    assert split >= 2            # the builder-like trees do have tiles to skip, and skipped them


def test_one_context_tree_after_tree(built, orc, env, want):
    """Every case in a fixed shuffled order on ONE context, the builder's demo tree in between; the whole scene, the tree alone, or the
    triangles alone.  Two frames after every upload: packets, leaf ranks, cull words, wide and compressed packets, the sky cut of the
    tree before must all be gone.  And an upload between two queued frames: the first is the old tree's."""
    order = list(CASES)
    np.random.default_rng(5).shuffle(order)
    sequence = []
    for k, name in enumerate(order):
        sequence.append(name)
        if k % 3 == 1:
            sequence.append(DEMO)
    d = it.demo()
    swapped = d.triangles.copy()
    swapped["materialIndex"] = 1 - swapped["materialIndex"]          # the same geometry (every tree over it stays valid), the other materials
    w, h = SIZES[1]
    with capi.Context(0) as ctx:
        ctx.upload_environment(env)
        ctx.resize(w, h)
        held = (None, None, None)
        only_tree = only_triangles = 0
        for step, name in enumerate(sequence):
            nodes, tris, mats, cam = scene_of(name)
            if tris is held[1] and mats is held[2]:
                ctx.upload_bvh(nodes)                                   # the tree alone
                only_tree += 1
            elif step % 2:
                ctx.upload_triangles(tris)
                ctx.upload_materials(mats)
                ctx.upload_bvh(nodes)
            else:
                upload(ctx, (nodes, tris, mats, cam))
            held = (nodes, tris, mats)
            got, cnt, launch = render(ctx, cam, w, h)
            ref, ocnt = want(name, w, h)
            assert pc.same_bits(got, ref), f"step {step}, {name}: " + pc.describe_diff(got, ref)
            pc.check_counters(cnt, ocnt, culled=launch["variant"] >= 9, what=f"step {step}, {name}")
            if tris is d.triangles and step % 4 == 0:
                ctx.upload_triangles(swapped)                           # the triangles alone
                only_triangles += 1
                held = (nodes, swapped, mats)
                got, cnt, launch = render(ctx, cam, w, h)
                ref, ocnt = want(name + ", materials swapped", w, h, scene=(nodes, swapped, mats, cam))
                assert pc.same_bits(got, ref), f"step {step}, {name}, materials swapped: " + pc.describe_diff(got, ref)
                pc.check_counters(cnt, ocnt, culled=launch["variant"] >= 9, what=f"step {step}, {name}, materials swapped")
        assert only_tree >= 3 and only_triangles >= 2
        # an upload between two queued frames, no read-back in between
        for first, second in ((DEMO, "missing children"), ("bad boxes", "unreachable leaves"), ("shared subtrees", DEMO)):
            upload(ctx, scene_of(first))
            cam = scene_of(first)[3]
            ctx.reset()
            ctx.set_uniforms(capi.PASS_RAYTRACE, it.uniforms(cam, w, h, frame=2).tobytes())
            ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
            ctx.submit(MASK)                                            # queued
            ctx.upload_bvh(scene_of(second)[0])
            ctx.set_uniforms(capi.PASS_RAYTRACE, it.uniforms(cam, w, h, frame=3).tobytes())
            ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 3).tobytes())
            ctx.submit(MASK)
            got = ctx.read_texture(capi.TEX_ACCUMULATION)
            acc = np.zeros((h, w, 4), np.float32)
            for f, nm in ((2, first), (3, second)):
                nodes, tris, mats, _ = scene_of(nm)
                img, _ = orc.raytrace(orc.OracleScene(tris, mats, nodes, env), it.uniforms(cam, w, h, frame=f).tobytes(), w, h)
                acc = orc.accumulate(pc.acc_uniforms(w, h, f).tobytes(), w, h, img, acc)
            assert pc.same_bits(got, acc), f"{first}, then {second}: " + pc.describe_diff(got, acc)


def test_a_two_member_group_renders_the_single_contexts_image(gpu_ctx, env, want):
    w, h = SIZES[0]
    with capi.Context(devices=[0, 0]) as group:
        group.upload_environment(env)
        group.resize(w, h)
        for name in ("missing children", "shared coincident sheets", "unreachable leaves"):
            cam = scene_of(name)[3]
            upload(group, scene_of(name))
            upload(gpu_ctx, scene_of(name), env)
            gpu_ctx.resize(w, h)
            single, _, launch = render(gpu_ctx, cam, w, h)
            got, _, glaunch = render(group, cam, w, h)
            assert glaunch["variant"] == launch["variant"], (name, glaunch, launch)
            assert pc.same_bits(got, single), f"{name}: " + pc.describe_diff(got, single)
            assert pc.same_bits(got, want(name, w, h)[0])


def test_no_bvh_at_all_every_ray_misses(built, orc, env):
    """A context that was never given a tree: the reference's walk of zero nodes (raytrace.wgsl:206-207) -- frame, feature images, probe."""
    d = it.demo()
    w, h = SIZES[1]
    osc = orc.OracleScene(d.triangles, d.material_bytes, None, env)
    with capi.Context(0) as ctx:
        ctx.upload_triangles(d.triangles)
        ctx.upload_materials(d.material_bytes)
        ctx.upload_environment(env)
        ctx.resize(w, h)
        for v in pc.variants_available(ctx, VARIANTS):
            ctx.set_kernel_variant(v)
            assert ctx.active_variant() == (v if v in (1, 2) else 4)
            got, cnt, launch = render(ctx, it.DEMO_VIEW, w, h)
            acc = np.zeros((h, w, 4), np.float32)
            total = dict.fromkeys(capi.COUNTER_NAMES, 0)
            for f in FRAMES:
                img, c = orc.raytrace(osc, it.uniforms(it.DEMO_VIEW, w, h, frame=f).tobytes(), w, h)
                acc = orc.accumulate(pc.acc_uniforms(w, h, f).tobytes(), w, h, img, acc)
                for k in total:
                    total[k] += c[k]
            assert total["hits"] == 0 and total["misses"] == total["rays"] == len(FRAMES) * w * h
            assert pc.same_bits(got, acc), f"variant {v}: " + pc.describe_diff(got, acc)
            pc.check_counters(cnt, total, what=f"no BVH, variant {v}")
        ctx.set_kernel_variant(0)
        u = it.uniforms(it.DEMO_VIEW, w, h).tobytes()
        ctx.set_uniforms(capi.PASS_RAYTRACE, u)
        ctx.render_aovs(capi.AOV_ALL)
        ref = ar.reference(orc, osc, u, w, h)
        assert not ref["hit"].any()
        ar.assert_images(pc, {nm: ctx.read_aov(k) for k, nm in enumerate(capi.AOV_NAMES)}, ref, "no BVH")
        rays = probe_rays(d.nodes)
        hit, cnt = orc.ray_scene_n(osc, rays)
        assert (hit[:, 0] == 0).all()
        for v in (1, 2, 4):
            ctx.set_kernel_variant(v)
            check_probe(ctx.debug_intersect(rays), hit, cnt, f"no BVH: debug_intersect, variant {v}")
        ctx.set_kernel_variant(0)
        with pytest.raises(capi.Mi3ptError, match=NOT_SHIPPED) as e:
            ctx.debug_intersect_shipped(rays)
        assert e.value.code == ERR_STATE


def test_refused_uploads_leave_the_scene_before_them_rendering(gpu_ctx, env, want):
    """What the upload turns away (stricter than the reference's walk: also in nodes the root never reaches) changes nothing; a leaf
    beyond the triangle buffer passes the upload and is a state error of every entry point that would walk it, before anything is
    launched."""
    ctx = gpu_ctx
    w, h = SIZES[1]
    upload(ctx, scene_of(DEMO), env)
    ctx.resize(w, h)
    ref, ocnt = want(DEMO, w, h)
    rays = probe_rays(it.demo().nodes)[:64]

    def still_renders(what):
        got, cnt, _ = render(ctx, it.DEMO_VIEW, w, h)
        assert pc.same_bits(got, ref), f"after {what}: " + pc.describe_diff(got, ref)
        pc.check_counters(cnt, ocnt, culled=True, what=f"after {what}")

    for name, (nodes, tris, message) in it.refused().items():
        if name in it.REFUSED_AT_SUBMIT:
            continue
        with pytest.raises(capi.Mi3ptError) as e:
            ctx.upload_bvh(nodes)
        assert e.value.code == ERR_INVALID and message in e.value.message, (name, e.value.message)
        still_renders(name)
    for name in it.REFUSED_AT_SUBMIT:
        nodes, tris, message = it.refused()[name]
        ctx.upload_bvh(nodes)
        ctx.reset()
        ctx.set_uniforms(capi.PASS_RAYTRACE, it.uniforms(it.DEMO_VIEW, w, h).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
        for call in (lambda: ctx.submit(MASK), lambda: ctx.submit(capi.SUBMIT_RAYTRACE), lambda: ctx.render_aovs(capi.AOV_ALL),
                     lambda: ctx.debug_intersect(rays), lambda: ctx.debug_intersect_shipped(rays), ctx.active_variant):
            with pytest.raises(capi.Mi3ptError) as e:
                call()
            assert e.value.code == ERR_STATE and message in e.value.message, (name, e.value.message)
        assert not ctx.read_texture(capi.TEX_ACCUMULATION).any()          # nothing was rendered
        ctx.upload_bvh(it.demo().nodes)
        still_renders(name)
