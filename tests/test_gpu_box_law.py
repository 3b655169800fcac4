"""The two device-side box makers -- the refit (csrc/pt_refit.hip) and the LBVH builder (csrc/pt_lbvh.hip) -- on the inputs of
tests/box_law_cases.py, where "the same box" is a question of 32-bit words: zeros of both signs, subnormals next to zeros, NaNs with
payloads, infinities; on trees whose left child has the higher index, whose chains have their leaves on the right or on alternating
sides, and whose padding words are not zero.  Every comparison is of words (refit_reference.first_difference,
lbvh_reference.first_word_difference); nothing here has a tolerance.

Together with tests/test_box_law_host.py this holds the three makers to one law, which is what the refit's promise -- on unchanged
triangles the uploaded bytes come back -- needs: host build -> upload -> refit, and device build -> upload -> refit, return their input."""
import functools

import numpy as np
import pytest

import box_law_cases as blc
import lbvh_reference as lr
import ptcommon as pc
import refit_reference as rr
import test_refit_reference as cpu
from mi3pt_host import capi, layout, scenes

pytestmark = pytest.mark.gpu

PZ, NZ = blc.PZ, blc.NZ
W, H = 48, 32
CASES = ("zeros", "subnormals", "non_finite")
SHAPES = ("built", "mirrored", "chain_right", "zigzag")


@pytest.fixture(scope="module")
def ctx(built):
    with capi.Context(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def _tree(name, shape):
    """(records as uploaded, triangles as they stand): the host-built tree (of the finite stand-in where the set is not finite: the
    tree a refit starts from was built before the vertices moved), its mirror image, or a 62-node chain over the first 63 triangles"""
    case = blc.all_cases()[name]
    if shape in ("built", "mirrored"):
        nodes = capi.host_build_bvh_f64(case.build_positions)
        return (blc.mirrored(nodes) if shape == "mirrored" else nodes), case.triangles()
    return {"chain_right": blc.chain_right, "zigzag": blc.zigzag}[shape](62), case.triangles(63)


def _refit(ctx, nodes, tris):
    ctx.upload_bvh(nodes)
    ctx.upload_triangles(tris)
    got, ms = ctx.device_refit_bvh()
    assert ms > 0 and len(got) == len(nodes)
    return got


def _same(got, want):
    diff = rr.first_difference(got, want)
    assert diff is None, diff


def _words(nodes):
    return np.ascontiguousarray(nodes).view(np.uint8).reshape(-1).view("<u4").reshape(-1, 12)


# ---------------------------------------------------------------- the refit against the law, word for word
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", CASES)
def test_refit_gives_the_laws_words(ctx, name, shape):
    """Every word of every record: zeros keep their sign, subnormals are compared as what they are, and a NaN arrives with its sign,
    payload and signalling bit -- the law only selects, so each bound is one of the words that went in."""
    nodes, tris = _tree(name, shape)
    want = rr.refit_scalar(nodes, tris)
    _same(want, rr.refit_vectorised(nodes, tris))
    got = _refit(ctx, nodes, tris)
    _same(got, want)
    if shape == "mirrored":
        inner = nodes["isLeaf"] != 1
        assert (nodes["left"][inner] > nodes["right"][inner]).any()
    box = _words(want)[:, [0, 1, 2, 4, 5, 6]]
    if name == "non_finite":
        # what the comparison above covered: every payload is in the expected leaf boxes, some reach internal nodes, and a NaN is
        # kept at some unions (it came from the left) and dropped at others (it came from the right)
        leaf = want["isLeaf"] == 1
        for payload in blc.NAN_PAYLOADS:
            assert (box[leaf] == payload).any(), hex(payload)
        assert np.isin(box[~leaf], blc.NAN_PAYLOADS).any()
        l, r = want["left"][~leaf], want["right"][~leaf]
        nan = np.isnan(want["min"])
        assert (nan[l] & ~nan[r] & nan[~leaf]).any() and (~nan[l] & nan[r] & ~nan[~leaf]).any()
        assert not (~nan[l] & nan[r] & nan[~leaf]).any()
    else:
        assert (box == PZ).any() and (box == NZ).any()
    if name == "subnormals":
        sub = (box & 0x7f800000 == 0) & (box & 0x007fffff != 0)
        assert sub.any()


def test_refit_of_the_demo_tree_with_nan_vertices(ctx):
    """tests/test_refit_reference.py's "non-finite" case on the device: the demo tree, one vertex of triangle 5 and all of triangle 40 NaN"""
    nodes, tris = cpu.cases()["non-finite"]
    want = rr.refit_vectorised(nodes, tris)
    assert np.isnan(want["min"]).any() and not np.isnan(want["min"][0]).all()
    _same(_refit(ctx, nodes, tris), want)


@pytest.mark.parametrize("shape", ("built", "zigzag"))
@pytest.mark.parametrize("name", CASES)
def test_refit_carries_the_padding_words(ctx, name, shape):
    """words 3 and 11 hold random bits in every record (mi3pt_upload_bvh takes them: the reference never reads them); they come back as
    uploaded, in leaves and in internal nodes, and the boxes are the law's"""
    plain, tris = _tree(name, shape)
    nodes = blc.stamped(plain, 7)
    got = _refit(ctx, nodes, tris)
    up, back = _words(nodes), _words(got)
    assert (back[:, [3, 7, 8, 9, 10, 11]] == up[:, [3, 7, 8, 9, 10, 11]]).all()
    for leaf in (True, False):
        sel = (nodes["isLeaf"] == 1) == leaf
        assert (back[sel][:, [3, 11]] != 0).any() and (back[sel][:, [3, 11]] == up[sel][:, [3, 11]]).all()
    _same(got, rr.refit_scalar(nodes, tris))
    assert (back[:, :3] == _words(rr.refit_scalar(plain, tris))[:, :3]).all()


@pytest.mark.parametrize("name", ("zeros", "subnormals"))
def test_host_built_tree_comes_back_unchanged(ctx, name):
    """host build -> upload -> refit: the uploaded bytes.  The host builder used to keep the first of two equal operands where the
    refit lets -0 win a minimum and +0 a maximum: on these two sets the bytes that came back were not the bytes that went in."""
    case = blc.all_cases()[name]
    nodes = capi.host_build_bvh_f64(case.positions)
    got = _refit(ctx, nodes, case.triangles())
    assert got.tobytes() == np.ascontiguousarray(nodes).tobytes(), rr.first_difference(got, nodes)
    again = _refit(ctx, got, case.triangles())
    assert again.tobytes() == got.tobytes()


# ---------------------------------------------------------------- the LBVH builder on zeros and subnormals
@pytest.mark.parametrize("name", ("zeros", "subnormals"))
def test_device_built_tree_has_the_laws_words_and_comes_back_unchanged(ctx, name):
    """device build -> word for word the CPU construction (fmin / fmax with -0 < +0: the law on everything but a NaN) -> upload ->
    refit -> the same bytes"""
    case = blc.all_cases()[name]
    tris = case.triangles()
    ctx.upload_triangles(tris)
    nodes, _ = ctx.device_build_bvh()
    lr.check_tree(nodes, tris)
    want = lr.reference_nodes(tris)
    diff = lr.first_word_difference(nodes, want)
    assert diff is None, diff
    box = _words(want)[:, [0, 1, 2, 4, 5, 6]]
    leaf = want["isLeaf"] == 1
    assert {PZ, NZ} <= set(box[leaf].ravel().tolist()) and {PZ, NZ} <= set(box[~leaf].ravel().tolist())
    _same(want, rr.refit_scalar(want, tris))                  # the CPU construction is a fixed point of the law itself
    got = _refit(ctx, nodes, tris)
    assert got.tobytes() == np.ascontiguousarray(nodes).tobytes(), rr.first_difference(got, nodes)


# ---------------------------------------------------------------- one render guard: the walks and the packet compiler read these bytes
def zeros_scene():
    """the `zeros` set as a scene, seen from a point whose x is exactly 0 -- the plane the first block lies in, so that min - o and
    max - o of its boxes are +-0 -- looking down on a cluster of the second block through a narrow lens"""
    z = blc.zeros()
    n = len(z)
    sc = scenes.Scene(z.positions, np.tile([0.0, 0.0, 1.0], (n, 3, 1)), np.zeros(n, int), [scenes.WHITE], "zeros")
    sc.build_bvh()
    target = z.positions[blc.BLOCK + 16].mean(0)               # a triangle of the second block's first pair: 0.2 across, 8.7 away
    sc.camera.update(position=(0.0, 6.0, float(target[2])), target=tuple(float(v) for v in target), fov=2.0)
    return sc


@pytest.mark.parametrize("variant", [7, 0], ids=["reference-counter-walk", "shipped-walk"])
def test_zeros_scene_renders_as_the_oracle_says(ctx, orc, env, variant):
    """48 x 32, frames 2 and 3, four bounces, the oracle on the same records: bit for bit, counters as elsewhere (variant 7 executes
    the reference's tests: all equal; the shipped walk culls)"""
    sc = zeros_scene()
    assert sc.camera["position"][0] == 0.0
    x_bounds = _words(sc.nodes)[:, [0, 4]]
    assert (x_bounds == PZ).any() and (x_bounds == NZ).any()
    osc = orc.OracleScene(sc.triangles, sc.material_bytes, sc.nodes, env)
    try:
        ctx.set_kernel_variant(variant)
        pc.upload_scene(ctx, sc, env)
        ctx.set_tile(0, 1, 8)
        ctx.resize(W, H)
        for frame in (2, 3):
            u = pc.rt_uniforms(sc, W, H, frame=frame, bounces=4)
            ctx.reset()
            ctx.reset_counters()
            pc.gpu_frame(ctx, u)
            img, cnt = ctx.read_texture(capi.TEX_OUTPUT), ctx.counters()
            want, ocnt = orc.raytrace(osc, u.tobytes(), W, H)
            assert pc.same_bits(img, want), pc.describe_diff(img, want)
            pc.check_counters(cnt, ocnt, culled=(variant == 0), what=f"zeros scene, variant {variant}, frame {frame}")
            assert cnt["stack_overflows"] == 0 and cnt["hits"] > 100 and cnt["misses"] > 100
    finally:
        ctx.set_kernel_variant(0)


# ---------------------------------------------------------------- the host's refit path on the device
def test_renderer_refits_the_unchanged_zeros_scene_to_itself(built, env):
    """renderer.refit = True and the `zeros` scene submitted twice: the second submit re-fits on the device, the cost ratio is 1.0
    exactly and the host's tree keeps the bytes it was built with"""
    from mi3pt_host import Renderer, RaytracingCamera, RaytracingScene
    sc = zeros_scene()
    built_bytes = np.ascontiguousarray(sc.nodes).tobytes()
    sc.nodes = None                                          # (the renderer builds)
    scene = RaytracingScene(sc, env)
    scene.needsUpdate = True
    cam = RaytracingCamera(2.0, position=sc.camera["position"], target=sc.camera["target"])
    with capi.Context(0) as own:
        r = Renderer(own)
        r.scalingFactor = 1
        r.presentEveryFrame = False
        r.resize(W, H)
        r.refit = True
        r.frames = 3
        r.render(scene, cam)
        assert np.ascontiguousarray(scene.content.nodes).tobytes() == built_bytes and r.lastRefitCostRatio is None
        scene.needsUpdate = True
        r.render(scene, cam)
        assert r.lastRefitCostRatio == 1.0 and r.lastRefitMs > 0
        assert np.ascontiguousarray(scene.content.nodes).tobytes() == built_bytes
