"""tests/reproject_reference.py on its own, without a device: a synthetic plane, exact single-texel cases of the definitions in
include/mi3pt.h (mi3pt_reproject, mi3pt_set_mean_by_count), the by-count law against the default law, and the use case -- a camera move
with the oracle's own renderer: the reprojected mean plus a few new frames against the same frames alone."""
import math

import numpy as np
import pytest

import aov_reference as ar
import ptcommon as pc
import reproject_reference as rr
from mi3pt_host import scenes

F = np.float32

# a camera at the origin looking down -z, fov 90, aspect 1: a point (a, b, -1) lands at fx = 2 (a + 1), fy = 2 (b + 1) of a 4 x 4 image
F0 = np.array([0, 0, 0, 1, 0, 0, -1, 1, 1, 0, 0, 1, 0, 1, 0, 0], F)
RES0 = (F(4), F(4))


def _old(rows=4, w=4):
    pos = np.zeros((rows, w, 4), F)
    pos[..., 2] = -1                      # every old texel lies in the plane z = -1 ...
    pos[..., 3] = 1
    nrm = np.zeros((rows, w, 4), F)
    nrm[..., 2] = 1                       # ... facing the camera
    ids = np.zeros((rows, w, 4), np.int32)
    ids[..., 1] = 7
    ids[..., 2] = 1
    return {"position": pos, "normal": nrm, "ids": ids}


def _new(fx, fy, rows=4, w=4):
    """a new view whose texel (0, 0) sees the point that the old view saw at (fx, fy); every other texel misses"""
    new = {"position": np.zeros((rows, w, 4), F), "normal": np.zeros((rows, w, 4), F), "ids": np.zeros((rows, w, 4), np.int32)}
    new["ids"][..., :2] = -1
    new["position"][..., 3] = 1e20
    new["position"][0, 0] = (fx / 2 - 1, fy / 2 - 1, -1, 1)
    new["normal"][0, 0] = (0, 0, 1, 0)
    new["ids"][0, 0] = (3, 7, 1, 0)
    return new


def _images(rows=4, w=4, n=8.0):
    acc = np.zeros((rows, w, 4), F)
    acc[..., 0] = np.arange(rows * w, dtype=F).reshape(rows, w)       # texel (x, y) holds 4 y + x
    acc[..., 1] = 1
    acc[..., 2] = 2
    acc[..., 3] = 1
    mo = np.zeros((rows, w, 4), F)
    mo[..., :3] = 7 * (n - 1)                                         # a per-sample variance of 7 in every channel
    mo[..., 3] = n
    return acc, mo


def _one(fx=1.25, fy=1.5, old=None, images=None, new=None, rect=(4, 4), **params):
    old = _old() if old is None else old
    acc, mo = _images() if images is None else images
    new = _new(fx, fy) if new is None else new
    a, m, info = rr.reproject(acc, mo, F0, RES0, new, old, rect, **params)
    return a[0, 0], m[0, 0], info


def test_four_taps_are_a_bilinear_mean_and_everything_else_restarts():
    a, m, info = _one()
    # fx = 1.25, fy = 1.5: taps (1, 1), (2, 1), (1, 2), (2, 2) = 5, 6, 9, 10 with 0.375, 0.125, 0.375, 0.125 -> 7.25 = 4 fy + fx
    assert a.tolist() == [7.25, 1.0, 2.0, 1.0]
    assert m.tolist() == [49.0, 49.0, 49.0, 8.0]                       # the variance 7 carried, n = min(8, 64): M2 = 7 * 7
    assert info["taps"][0, 0] == 4 and info["carried"].sum() == 1 and info["restarted"].sum() == 15
    full_a, full_m, _ = rr.reproject(*_images(), F0, RES0, _new(1.25, 1.5), _old(), (4, 4))
    assert np.all(full_a[1:] == (0, 0, 0, 1)) and np.all(full_m[1:] == 0)      # misses restart: (0, 0, 0, 1), (0, 0, 0, 0)
    assert full_a.dtype == F and full_m.dtype == F


def test_texels_outside_the_rectangle_keep_their_bits():
    acc, mo = _images()
    acc[3, 3] = (np.nan, -1, 5, 9)
    a, m, info = rr.reproject(acc, mo, F0, RES0, _new(1.25, 1.5), _old(), (3, 2))
    assert pc.same_bits(a[2:], acc[2:]) and pc.same_bits(a[:, 3:], acc[:, 3:]) and pc.same_bits(m[2:], mo[2:]) and pc.same_bits(m[:, 3:], mo[:, 3:])
    assert not info["carried"][2:].any() and not info["restarted"][2:].any() and info["restarted"][:2, :3].sum() == 5
    # ... and a tap outside the rectangle does not count: rows 2 and 3 are outside, the taps of row 2 drop out -> (5 * 0.375 + 6 * 0.125) / 0.5
    assert a[0, 0].tolist() == [5.25, 1.0, 2.0, 1.0] and info["taps"][0, 0] == 2


@pytest.mark.parametrize("rule", ["hit", "material", "n below 1", "n NaN", "normal", "plane", "zero weight", "outside the image"])
def test_each_tap_rule_alone(rule):
    """the tap (2, 1) -- value 6, weight 0.125 -- made to fail one rule: the other three renormalise, (5 * 0.375 + 9 * 0.375 + 10 * 0.125) /
    0.875; then the same tap exactly AT the rule's limit, where it still counts"""
    old, (acc, mo) = _old(), _images()
    fx, fy, want, taps = 1.25, 1.5, F(F(F(F(5 * 0.375) + F(9 * 0.375)) + F(10 * 0.125)) / F(0.875)), 3
    params = {}
    if rule == "hit":
        old["ids"][1, 2, 2] = 0
    elif rule == "material":
        old["ids"][1, 2, 1] = 8
    elif rule == "n below 1":
        mo[1, 2, 3] = 0.999
    elif rule == "n NaN":
        mo[1, 2, 3] = np.nan
    elif rule == "normal":
        old["normal"][1, 2, :3] = (0.6, 0, 0.7)                         # dot = 0.7 < 0.75
        params["normal_cos_min"] = 0.75
    elif rule == "plane":
        old["position"][1, 2, 2] = -1.5                                 # 0.5 off the new texel's plane; t1 = 1, tolerance 0.25
        params["plane_tolerance"] = 0.25
    elif rule == "zero weight":
        fx, want, taps = 1.0, F(7.0), 2                                 # tx = 0: the taps of column 2 weigh 0 and do not count -> (5 + 9) / 2
    elif rule == "outside the image":
        fx, want, taps = -0.5, F(F(F(4 * 0.25) + F(8 * 0.25)) / F(0.5)), 2      # x0 = -1: only column 0 -> (4 + 8) / 2
    a, m, info = _one(fx, fy, old=old, images=(acc, mo), **params)
    assert info["taps"][0, 0] == taps and a[0] == want and a[3] == 1
    # at the limit the tap counts
    old, (acc, mo) = _old(), _images()
    if rule == "n below 1":
        mo[1, 2, 3] = 1.0
        a, m, info = _one(old=old, images=(acc, mo))
        assert info["taps"][0, 0] == 4 and m[3] == 1.0 and a[0] == 7.25                  # n' = the smallest n of the taps
        assert m[:3].tolist() == [0.0, 0.0, 0.0]                                          # (var / ws) * (1 - 1)
    elif rule == "normal":
        old["normal"][1, 2, :3] = (0.0, 0.6, 0.75)
        assert _one(old=old, normal_cos_min=0.75)[2]["taps"][0, 0] == 4
    elif rule == "plane":
        old["position"][1, 2, 2] = -1.25
        assert _one(old=old, plane_tolerance=0.25)[2]["taps"][0, 0] == 4
        old["position"][1, 2, 2] = -0.75                                # fabsf: either side
        assert _one(old=old, plane_tolerance=0.25)[2]["taps"][0, 0] == 4


def test_the_tap_order_is_the_sums_order():
    """(0, 0), (1, 0), (0, 1), (1, 1) with weight 1 / 4 each: ((2^24 + 1) - 2^24) + 1 = 1 in fp32 in that order; any order that adds the two
    small terms first gives 2"""
    acc, mo = _images()
    acc[0, 0, 0], acc[0, 1, 0], acc[1, 0, 0], acc[1, 1, 0] = 2.0 ** 26, 4, -2.0 ** 26, 4
    a, m, info = _one(0.5, 0.5, images=(acc, mo))
    assert info["taps"][0, 0] == 4 and a.tolist() == [1.0, 1.0, 2.0, 1.0]


def test_fewer_than_two_samples_carry_no_variance():
    acc, mo = _images()
    mo[..., 3] = 1.5
    a, m, _ = _one(images=(acc, mo))
    assert a[0] == 7.25 and m.tolist() == [0.0, 0.0, 0.0, 1.5]
    acc, mo = _images()
    mo[1, 1] = (-3, np.nan, 4, 2)                                       # fmax drops a negative and a NaN quotient
    a, m, _ = _one(images=(acc, mo))
    want = F(F(0.375 * 0) + F(0.125 * 7)) + F(0.375 * 7) + F(0.125 * 7)
    assert m[0] == F(want * 1) and m[1] == F(want * 1) and m[3] == 2.0
    assert m[2] == F(F(F(F(0.375 * 4) + F(0.125 * 7)) + F(0.375 * 7)) + F(0.125 * 7))


def test_max_history_shortens_the_history_and_keeps_the_variance():
    acc, mo = _images(n=100.0)
    a, m, _ = _one(images=(acc, mo), max_history=10)
    assert a[0] == 7.25 and m.tolist() == [63.0, 63.0, 63.0, 10.0]     # 7 * (10 - 1)
    a, m, _ = _one(images=(acc, mo), max_history=256)
    assert m.tolist() == [693.0, 693.0, 693.0, 100.0]                   # the cap does not lengthen a history
    mo[2, 2, 3] = 3.0
    mo[2, 2, :3] = 14.0
    a, m, _ = _one(images=(acc, mo), max_history=64)
    assert m.tolist() == [14.0, 14.0, 14.0, 3.0]                        # the youngest tap sets n'


def test_no_tap_no_projection_no_hit_restart():
    acc, mo = _images()
    mo[..., 3] = np.nan
    a, m, info = _one(images=(acc, mo))
    assert a.tolist() == [0, 0, 0, 1] and m.tolist() == [0, 0, 0, 0] and info["restarted"][0, 0]
    for z in (0.0, 1.0):                                                # cz = 0 and cz < 0: behind the old camera
        new = _new(1.25, 1.5)
        new["position"][0, 0, 2] = z
        a, m, info = _one(new=new)
        assert a.tolist() == [0, 0, 0, 1] and m.tolist() == [0, 0, 0, 0] and info["taps"][0, 0] == 0
    new = _new(1.25, 1.5)
    new["ids"][0, 0, 2] = 0
    assert _one(new=new)[0].tolist() == [0, 0, 0, 1]
    for fx, fy in ((-1.0, 1.0), (4.0, 1.0), (1.0, -1.0), (1.0, 4.0), (np.nan, 1.0)):      # fx > -1 && fx < W, likewise fy; a NaN fails
        assert _one(fx, fy)[2]["restarted"][0, 0], (fx, fy)
    assert _one(3.5, 3.5)[2]["taps"][0, 0] == 1                         # the last texel alone, the others lie outside the image


def test_f16_storage_rounds_the_carried_mean_only():
    acc, mo = _images()
    acc[..., 1] = F(0.1)
    mo[..., :3] = F(0.1) * 7
    a, m, _ = _one(images=(acc, mo), store_f16=True)
    assert a[1] == F(np.float16(F(0.1))) and a[1] != F(0.1)
    assert m[0] == _one(images=(acc, mo))[1][0]


# ---- a synthetic plane ----
def _plane_view(position, w, h):
    """first-hit features of the 5 x 5 square y = 0 seen from `position` looking along (0, -1, -4) / |.|, fov 45: float64 rays of the frame
    the reprojection uses, positions rounded to fp32 once"""
    u = pc.rt_uniforms(scenes.demo_scene(), w, h, position=position, direction=tuple(np.array([0.0, -1.0, -4.0]) / math.sqrt(17.0)))
    f = rr.view_frame(u.tobytes()).astype(np.float64)
    pos, aspect, fwd, t, uu, r, vv = f[0:3], f[3], f[4:7], f[7], f[8:11], f[11], f[12:15]
    ys, xs = np.mgrid[0:h, 0:w]
    d = uu * (-r + 2 * r * xs[..., None] / w) + vv * (-t + 2 * t * ys[..., None] / h) + fwd * aspect
    with np.errstate(all="ignore"):
        s = -pos[1] / d[..., 1]
    P = pos + s[..., None] * d
    hit = (d[..., 1] < 0) & (np.abs(P[..., 0]) <= 2.5) & (np.abs(P[..., 2]) <= 2.5)
    feat = {"position": np.zeros((h, w, 4), F), "normal": np.zeros((h, w, 4), F), "ids": np.zeros((h, w, 4), np.int32)}
    feat["position"][..., 3] = 1e20
    feat["ids"][..., :2] = -1
    feat["position"][hit, :3] = P[hit]
    feat["position"][hit, 3] = (s * np.sqrt((d * d).sum(-1)))[hit]
    feat["normal"][hit] = (0, 1, 0, 0)
    feat["ids"][hit] = (0, 0, 1, 0)
    return u, feat, hit, P


def _linear(P):
    return np.stack([1 + 0.25 * P[..., 0], 2 + 0.125 * P[..., 2], 3 + 0.5 * P[..., 0] - 0.25 * P[..., 2]], axis=-1)


def test_a_plane_whose_mean_is_linear_in_the_world_point():
    """The mean of the old view is f(world point), f linear.  After a pure sideways move every texel carried from all of its taps that weigh (two where
    the point stays on its row: ty = 0) equals f at its
    OWN world point up to the error of bilinear interpolation of g(x, y) = f(old view's point at (x, y)) on the texel grid, which is at
    most (max |g_xx| + max |g_yy|) / 8 per channel; the second differences of the old image stand for the derivatives, and a factor 2
    covers that they are differences.  A texel carried from fewer taps (the square's edge) is a mean of neighbours: within one first
    difference.  The texels whose point lay outside the old image restart."""
    w, h = 64, 48
    u0, old, hit0, P0 = _plane_view((0.0, 1.0, 4.0), w, h)
    u1, new, hit1, P1 = _plane_view((0.5, 1.0, 4.0), w, h)
    acc = np.zeros((h, w, 4), F)
    acc[hit0, :3] = _linear(P0)[hit0]
    acc[..., 3] = 1
    mo = np.zeros((h, w, 4), F)
    mo[..., 3] = 32
    f0 = rr.view_frame(u0.tobytes())
    a, m, info = rr.reproject(acc, mo, f0, (F(w), F(h)), new, old, (w, h))
    g = np.where(hit0[..., None], _linear(P0), np.nan)
    dxx = np.abs(g[:, 2:] - 2 * g[:, 1:-1] + g[:, :-2])
    dyy = np.abs(g[2:] - 2 * g[1:-1] + g[:-2])
    bound = 2 * (np.nanmax(dxx) + np.nanmax(dyy)) / 8 + 1e-5
    first = max(np.nanmax(np.abs(np.diff(g, axis=0))), np.nanmax(np.abs(np.diff(g, axis=1)))) + 1e-5
    err = np.abs(a[..., :3].astype(np.float64) - _linear(P1)).max(axis=-1)
    four = info["carried"] & (info["taps"] == info["weighted"])
    some = info["carried"] & (info["taps"] < info["weighted"])
    print(f"plane: {int(four.sum())} texels from every weighted tap, worst error {err[four].max():.3g} (bound {bound:.3g}); {int(some.sum())} from fewer, "
          f"worst {err[some].max():.3g} (bound {first:.3g}); {int((hit1 & info['restarted']).sum())} of {int(hit1.sum())} hit texels restart")
    assert four.sum() > 0.6 * hit1.sum() and err[four].max() <= bound
    assert some.sum() > 0 and err[some].max() <= first
    assert np.all(m[info["carried"], 3] == 32) and not info["carried"][~hit1].any()
    # where the old view did not see the point -- outside its image, or off the square's edge it saw -- the texel restarts
    f = f0.astype(np.float64)
    d = P1 - f[0:3]
    fx = ((d @ f[8:11]) * f[3] / (d @ f[4:7]) + f[11]) / (2 * f[11]) * w
    left = hit1 & (fx >= w)
    assert left.sum() > 0 and info["restarted"][left].all()
    assert np.all(a[info["restarted"]] == (0, 0, 0, 1)) and np.all(m[info["restarted"]] == 0)


# ---- the by-count law ----
@pytest.mark.parametrize("store_f16", [False, True], ids=["f32", "f16"])
def test_by_count_equals_the_default_law_run_with_frames_one_to_n(store_f16):
    rng = np.random.default_rng(5)
    rows, w = 5, 7
    pa = pb = np.zeros((rows, w, 4), F)
    ma = mb = np.zeros((rows, w, 4), F)
    inside = np.ones((rows, w), bool)
    inside[:, 6] = False
    for k in range(12):
        c = (rng.random((rows, w, 4), dtype=F) * 4).astype(F)
        pa, ma = rr.by_count_step(pa, ma, c, store_f16=store_f16, inside=inside)
        pb, mb = rr.default_step(pb, mb, c, 1 + k, store_f16=store_f16, inside=inside)
        assert pc.same_bits(pa, pb) and pc.same_bits(ma, mb), k
    assert np.all(ma[:, :6, 3] == 12) and np.all(ma[:, 6] == 0) and np.all(pa[:, 6] == 0)
    # enabled != 1 restarts, as the default law's weight 1 does
    pa, ma = rr.by_count_step(pa, ma, c, enabled=0)
    assert pc.same_bits(pa[:, :, :3], c[:, :, :3]) and np.all(ma[..., 3] == 1) and np.all(ma[..., :3] == 0)


def test_a_thawed_tile_continues_as_a_sample_mean():
    """frames 1 .. 4 everywhere, 5 .. 8 with the left half frozen, 9 .. 12 everywhere, 13 .. 16 frozen again: under the count the left half
    is the mean of its twelve samples (to the rounding of twelve fp32 steps, 12 x 2^-24 relative and then some); under the default law it
    is not -- the weight 1 / frame of frame 9 takes the frozen half for a mean of eight"""
    rng = np.random.default_rng(6)
    rows, w = 4, 8
    left = np.zeros((rows, w), bool)
    left[:, :4] = True
    pa = pb = np.zeros((rows, w, 4), F)
    ma = mb = np.zeros((rows, w, 4), F)
    total = np.zeros((rows, w, 3))
    count = np.zeros((rows, w))
    for k in range(16):
        c = (1 + rng.random((rows, w, 4), dtype=F) * 4).astype(F)
        sampled = ~left if (4 <= k < 8 or k >= 12) else np.ones((rows, w), bool)
        pa, ma = rr.by_count_step(pa, ma, c, inside=sampled)
        pb, mb = rr.default_step(pb, mb, c, 1 + k, inside=sampled)
        total += np.where(sampled[..., None], c[..., :3].astype(np.float64), 0)
        count += sampled
    assert np.all(count[left] == 8) and np.all(count[~left] == 16) and np.all(ma[..., 3] == count)
    mean = total / count[..., None]
    assert np.abs(pa[..., :3] / mean - 1).max() < 1e-5
    assert pc.same_bits(pa[~left], pb[~left]) and np.abs(pb[left][:, :3] / mean[left] - 1).max() > 1e-3


# ---- the use case ----
def _tone_rmse(x, truth, sel):
    a = np.asarray(x, np.float64)[..., :3][sel]
    b = np.asarray(truth, np.float64)[..., :3][sel]
    return float(np.sqrt((((a / (1 + a)) - (b / (1 + b))) ** 2).mean()))


ORBIT_DEGREES = 2.0


def test_reprojection_beats_a_restart_after_a_camera_move(orc, demo):
    """48 x 32, four bounces, the sun-less sky of test_convergence_reference.py (under the sun a 1 024-frame yardstick is itself
    fireflies): 64 frames in view A, the camera orbits by ORBIT_DEGREES about the vertical axis through its target, then reproject + 4
    new frames against the same 4 frames alone; yardstick: a 1 024-frame mean of view B, tone-mapped RMSE over B's hit texels.
    Measured: reprojected over restarted 0.316 / 0.285 / 0.285 for maxHistory 16 / 64 / 256 (the history holds 64 samples: 256 caps
    nothing); 1 152 of 1 165 hit texels carried, 13 restart.  No ratio is asserted, only that reprojection wins."""
    w, h = 48, 32
    osc = pc.oracle_scene(orc, demo, scenes.synthetic_env(sun_radiance=0.0))
    cam = demo.camera
    pos_b, dir_b = rr.orbit(cam["position"], cam["target"], ORBIT_DEGREES)
    ua = lambda frame: pc.rt_uniforms(demo, w, h, frame=frame, bounces=4)
    ub = lambda frame: pc.rt_uniforms(demo, w, h, frame=frame, bounces=4, position=pos_b, direction=dir_b)
    mean = np.zeros((h, w, 4), F)
    moments = np.zeros((h, w, 4), F)
    for k in range(64):
        mean, moments = rr.by_count_step(mean, moments, orc.raytrace(osc, ua(2 + k).tobytes(), w, h)[0])
    truth = np.zeros((h, w, 4), np.float64)
    for f in range(1000, 2024):
        truth += orc.raytrace(osc, ub(f).tobytes(), w, h)[0]
    truth /= 1024
    feat_a = ar.reference(orc, osc, ua(0).tobytes(), w, h)
    feat_b = ar.reference(orc, osc, ub(0).tobytes(), w, h)
    hit_b = feat_b["ids"][..., 2] == 1
    new_frames = [orc.raytrace(osc, ub(66 + k).tobytes(), w, h)[0] for k in range(4)]      # (the seed offset: frames the old view never used)
    alone, alone_m = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    for c in new_frames:
        alone, alone_m = rr.by_count_step(alone, alone_m, c)
    e_alone = _tone_rmse(alone, truth, hit_b)
    f0 = rr.view_frame(ua(0).tobytes())
    ratios = {}
    for history in (16, 64, 256):
        a, m, info = rr.reproject(mean, moments, f0, (F(w), F(h)), feat_b, feat_a, (w, h), max_history=history)
        e_carried = _tone_rmse(a, truth, hit_b)
        for c in new_frames:
            a, m = rr.by_count_step(a, m, c)
        ratios[history] = _tone_rmse(a, truth, hit_b) / e_alone
        carried, restarted = int((info["carried"] & hit_b).sum()), int((info["restarted"] & hit_b).sum())
        print(f"maxHistory {history}: reprojected + 4 frames {ratios[history] * e_alone:.5f}, 4 frames alone {e_alone:.5f}, ratio {ratios[history]:.3f}; "
              f"the carried mean alone {e_carried:.5f}; {carried} of {int(hit_b.sum())} hit texels carried, {restarted} restart")
        assert ratios[history] < 1.0, history
    assert carried >= 0.5 * hit_b.sum() and restarted >= 0.01 * hit_b.sum()
    assert not info["carried"][~hit_b].any()
