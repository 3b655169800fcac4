"""tests/reproject_scene_reference.py on its own, without a device: the oracle's first-hit features of the demo scene and of moved variants
of it (tests/reproject_scene_cases.py) at 32 x 24, the definition of include/mi3pt.h (mi3pt_reproject_scene) against mi3pt_reproject's
where nothing moved, against the known answer where everything moved rigidly with the camera, and exact single-texel cases."""
import numpy as np
import pytest

import aov_reference as ar
import ptcommon as pc
import reproject_reference as rr
import reproject_scene_cases as cases
import reproject_scene_reference as rs
import test_reproject_reference as trr

F = np.float32
W, H = 32, 24


def _uniforms(sc, position=None, direction=None):
    if position is None:
        return pc.rt_uniforms(sc, W, H, frame=0, bounces=4)
    return pc.rt_uniforms(sc, W, H, frame=0, bounces=4, position=position, direction=direction)


def _features(orc, sc, u):
    feat = ar.reference(orc, pc.oracle_scene(orc, sc), u.tobytes(), W, H)
    feat["ids"] = cases.triangle_indices(orc, sc, u.tobytes(), feat, W, H)
    return feat


@pytest.fixture(scope="module")
def views(orc, demo):
    """name -> (scene, uniforms, features), computed once and left unchanged"""
    cam = demo.camera
    out = {}
    u = _uniforms(demo)
    out["old"] = (demo, u, _features(orc, demo, u))
    u = _uniforms(demo, *rr.orbit(cam["position"], cam["target"], 2.0))
    out["orbit"] = (demo, u, _features(orc, demo, u))
    sc = cases.translated(demo)
    u = _uniforms(demo, tuple(np.array(cam["position"]) + np.array(cases.TRANSLATION)), demo.camera_direction())
    out["translated"] = (sc, u, _features(orc, sc, u))
    sc = cases.box_moved(demo)
    u = _uniforms(demo)
    out["box"] = (sc, u, _features(orc, sc, u))
    return out


def _random_images(seed):
    rng = np.random.default_rng(seed)
    acc = (rng.random((H, W, 4), dtype=F) * 4).astype(F)
    acc[..., 3] = 1
    mo = (rng.random((H, W, 4), dtype=F) * 50).astype(F)
    mo[..., 3] = rng.choice(np.array([0, 1, 2, 500], F), size=(H, W), p=[0.15, 0.15, 0.2, 0.5])
    return acc, mo


def _f0(views):
    return rr.view_frame(views["old"][1].tobytes())


def test_unchanged_geometry_is_reproject_bit_for_bit(views, demo):
    acc, mo = _random_images(1)
    new, old = views["orbit"][2], views["old"][2]
    for params in ({}, dict(plane_tolerance=0.005, normal_cos_min=0.99, max_history=3)):
        want = rr.reproject(acc, mo, _f0(views), (F(W), F(H)), new, old, (W, H), **params)
        got = rs.reproject_scene(acc, mo, _f0(views), (F(W), F(H)), new, old, (W, H), demo.triangles, demo.triangles, max_history_moved=1, **params)
        assert pc.same_bits(got[0], want[0]) and pc.same_bits(got[1], want[1])
        assert np.array_equal(got[2]["carried"], want[2]["carried"]) and np.array_equal(got[2]["taps"], want[2]["taps"])
        hit = new["hit"]
        assert got[2]["static"][hit].all() and not got[2]["moved"].any() and got[2]["carried"].sum() > 0.5 * hit.sum()


@pytest.mark.parametrize("moved_history", [8, 3, 64])
def test_a_rigid_move_of_scene_and_camera_carries_every_texel_to_itself(views, demo, moved_history):
    """scene and camera moved by the same translation: every triangle moved, every hit texel's point of the kept geometry is the point the
    old view saw at the SAME texel.  With the mean A = (x / w, y / h, 0.5) the carried mean names the texel it was gathered from: within a
    quarter texel of its own -- an off-by-one tap is a whole one"""
    ys, xs = np.mgrid[0:H, 0:W]
    acc = np.stack([xs / W, ys / H, np.full((H, W), 0.5), np.ones((H, W))], axis=-1).astype(F)
    mo = np.zeros((H, W, 4), F)
    mo[..., :3] = 7
    mo[..., 3] = 8
    sc, _, new = views["translated"]
    a, m, info = rs.reproject_scene(acc, mo, _f0(views), (F(W), F(H)), new, views["old"][2], (W, H), sc.triangles, demo.triangles,
                                    max_history_moved=moved_history)
    hit = new["hit"]
    carried = info["carried"]
    print(f"translated: {int(carried.sum())} of {int(hit.sum())} hit texels carried, {int(info['moved'].sum())} moved")
    assert np.array_equal(hit, views["old"][2]["hit"]) and info["moved"][hit].all() and not info["static"].any()
    assert not carried[~hit].any() and carried.sum() >= 0.99 * hit.sum()
    assert np.abs(a[..., 0].astype(np.float64) - xs / W)[carried].max() <= 0.25 / W
    assert np.abs(a[..., 1].astype(np.float64) - ys / H)[carried].max() <= 0.25 / H
    assert np.all(m[..., 3][carried] == min(8, moved_history))


def test_a_moved_box_under_a_fixed_camera(views, demo):
    acc, mo = _random_images(2)
    mo[..., 3] = np.where(mo[..., 3] == 0, 300, mo[..., 3])          # (every old texel has a history: what restarts does so for its surface)
    sc, _, new = views["box"]
    old = views["old"][2]
    moved_history = 4
    a, m, info = rs.reproject_scene(acc, mo, _f0(views), (F(W), F(H)), new, old, (W, H), sc.triangles, demo.triangles,
                                    max_history_moved=moved_history)
    want = rr.reproject(acc, mo, _f0(views), (F(W), F(H)), new, old, (W, H))
    tri = new["ids"][..., 0]
    on_box = (tri >= cases.BOX.start) & (tri < cases.BOX.stop)
    assert np.array_equal(info["moved"], on_box) and np.array_equal(info["static"], new["hit"] & ~on_box)
    static = info["static"]
    assert static.sum() > 0 and pc.same_bits(a[static], want[0][static]) and pc.same_bits(m[static], want[1][static])
    box_carried = on_box & info["carried"]
    print(f"box: {int(on_box.sum())} box texels, {int(box_carried.sum())} carried; static reproject alone carries {int((on_box & want[2]['carried']).sum())}")
    assert box_carried.sum() >= 1 and np.all(m[..., 3][box_carried] <= moved_history) and np.all(m[..., 3][box_carried] >= 1)
    # the ground behind the box's old place: the old view saw the box there
    old_tri = old["ids"][..., 0]
    uncovered = (tri >= 0) & (tri < cases.GROUND.stop) & (old_tri >= cases.BOX.start) & (old_tri < cases.BOX.stop)
    assert (uncovered & info["restarted"]).sum() >= 1
    assert np.all(a[info["restarted"]] == (0, 0, 0, 1)) and np.all(m[info["restarted"]] == 0)


# ---- exact single-texel cases on test_reproject_reference.py's synthetic plane z = -1 (a 4 x 4 old view, fov 90 at the origin) ----
def _record(a, b, c, normal=(0, 0, 1)):
    r = np.zeros(28, F)
    r[0:3], r[4:7], r[8:11] = a, b, c
    r[12:15] = r[16:19] = r[20:23] = normal
    return r


def _one(fx, fy, rec1, rec0, tri=0, **params):
    new = trr._new(fx, fy)
    new["ids"][0, 0, 0] = tri
    acc, mo = trr._images()
    a, m, info = rs.reproject_scene(acc, mo, trr.F0, trr.RES0, new, trr._old(), (4, 4), np.stack([rec1]), np.stack([rec0]), **params)
    return a[0, 0], m[0, 0], info


def test_a_moved_triangle_is_followed_back_exactly():
    """the new triangle is the kept one moved by (-0.5, 0, 0): the new texel's point (fx 2.25 -> x = 0.125) was at x = 0.625, fx 3.25"""
    rec0 = _record((-1, -1, -1), (3, -1, -1), (-1, 3, -1))
    rec1 = _record((-1.5, -1, -1), (2.5, -1, -1), (-1.5, 3, -1))
    a, m, info = _one(2.25, 1.5, rec1, rec0, max_history_moved=5)
    # taps (3, 1), (3, 2) = 7, 11 with 0.75 * 0.5 each and the column 4 outside the image -> 9; static it would be 4 * 1.5 + 2.25 = 8.25
    assert info["moved"][0, 0] and a.tolist() == [9.0, 1.0, 2.0, 1.0] and m.tolist() == [28.0, 28.0, 28.0, 5.0]
    a, m, info = _one(2.25, 1.5, rec0, rec0, max_history_moved=5)
    assert info["static"][0, 0] and a.tolist() == [8.25, 1.0, 2.0, 1.0] and m.tolist() == [49.0, 49.0, 49.0, 8.0]
    # an interpolated normal of another length: len scales both tests, nothing else -- the same answer
    rec0_long = _record((-1, -1, -1), (3, -1, -1), (-1, 3, -1), normal=(0, 0, 4))
    assert _one(2.25, 1.5, rec1, rec0_long, max_history_moved=5)[0].tolist() == [9.0, 1.0, 2.0, 1.0]
    # ... and one that faces away fails the normal test of every tap
    rec0_back = _record((-1, -1, -1), (3, -1, -1), (-1, 3, -1), normal=(0, 0, -1))
    assert _one(2.25, 1.5, rec1, rec0_back)[2]["restarted"][0, 0]


def test_a_degenerate_triangle_a_zero_normal_and_a_bad_index_restart():
    rec0 = _record((-1, -1, -1), (3, -1, -1), (-1, 3, -1))
    needle = _record((-1, -1, -1), (3, -1, -1), (1, -1, -1))                       # three points of one line: den = 0
    a, m, info = _one(1.25, 1.5, needle, rec0)
    assert info["moved"][0, 0] and info["restarted"][0, 0] and a.tolist() == [0, 0, 0, 1] and m.tolist() == [0, 0, 0, 0]
    flat = _record((-1.5, -1, -1), (2.5, -1, -1), (-1.5, 3, -1))
    assert _one(1.25, 1.5, flat, _record((-1, -1, -1), (3, -1, -1), (-1, 3, -1), normal=(0, 0, 0)))[2]["restarted"][0, 0]      # len = 0
    assert _one(1.25, 1.5, flat, _record((-1, -1, -1), (3, -1, -1), (-1, 3, np.nan)))[2]["restarted"][0, 0]
    for tri in (-1, -2, 1, 2 ** 31 - 1):
        a, m, info = _one(1.25, 1.5, rec0, rec0, tri=tri)
        assert info["restarted"][0, 0] and not info["static"][0, 0] and not info["moved"][0, 0], tri
    assert _one(1.25, 1.5, rec0, rec0)[2]["carried"][0, 0]
