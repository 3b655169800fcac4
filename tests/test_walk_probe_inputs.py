"""The inputs of tests/test_gpu_walk_probes.py (tests/walk_probe_inputs.py) through the oracle alone: the cases the GPU tests are
about must BE there -- per family both answers of the reference, and at least one pair in each class a kernel treats specially
(the plain-division path, an unsafe box, an undecided filtered test, u / v / u + v / t / det on their limits).  No GPU needed."""
import numpy as np
import pytest

import walk_probe_inputs as wpi

f32 = np.float32


@pytest.fixture(scope="module")
def box(orc):
    out = {}
    for name, (r, mn, mx) in wpi.box_pairs().items():
        out[name] = (r, mn, mx, orc.ray_aabb_n(r, mn, mx))
    return out


@pytest.fixture(scope="module")
def tri(orc):
    return {name: (r, g, orc.ray_triangle_n(r, g)) for name, (r, g) in wpi.triangle_pairs().items()}


def _both_answers(name, hit, all_miss=()):
    share = float(np.mean(hit))
    if name in all_miss:      # all-miss by construction (up to the rounding of a constructed vertex): nothing to balance
        assert share < 0.05, f"{name}: meant to miss, {share:.3f} accepted"
    else:
        assert 0.05 <= share <= 0.95, f"{name}: {share:.3f} accepted"


def test_batched_oracle_calls_equal_the_single_ones(orc, box, tri):
    r, mn, mx, want = box["corners edges faces"]
    for i in range(0, len(r), 97):
        assert orc.ray_aabb(r[i, :3], r[i, 3:], mn[i], mx[i]) == bool(want[i])
    from mi3pt_host import layout
    r, g, want = tri["vertices and edges"]
    rec = np.zeros(1, layout.TRIANGLE)
    for i in range(0, len(r), 97):
        rec["aPosition"], rec["bPosition"], rec["cPosition"] = g[i, 0:3], g[i, 3:6], g[i, 6:9]
        one = orc.ray_triangle(r[i, :3], r[i, 3:], rec)
        assert one[0] == want[i, 0] and (one[1] == want[i, 1] or not want[i, 0])


def test_box_families_hold_both_answers_and_every_class(box):
    assert all(len(v[0]) <= 40000 for v in box.values())
    flags8 = unsafe = und = 0
    for name, (r, mn, mx, hit) in box.items():
        _both_answers(name, hit)
        flags8 += int((wpi.ray_flags(r) == 8).sum())
        unsafe += int(wpi.box_unsafe_host(mn, mx).sum())
        und += int(wpi.undecided(r, mn, mx).sum())
    assert flags8 > 0 and unsafe > 0 and und > 0
    # the family whose share of undecided pairs the GPU test bounds does stay under that bound in the replay
    r, mn, mx, _ = box[wpi.ORDINARY_BOX_FAMILY]
    assert wpi.undecided(r, mn, mx).sum() < wpi.UNDECIDED_BOUND * len(r)
    # both sides of every guard
    allr = np.concatenate([v[0] for v in box.values()])
    ad = np.abs(allr[:, 3:])
    for v in (wpi.EPS, wpi.BIG_D):
        assert (ad == v).any() and (ad == wpi._up(v)).any() and (ad == wpi._down(v)).any()
    ao = np.abs(np.concatenate([allr[:, :3]] + [v[1] for v in box.values()] + [v[2] for v in box.values()]))
    for v in (wpi.LO, wpi.HI):
        assert (ao == v).any() and (ao == wpi._up(v)).any() and (ao == wpi._down(v)).any()
    assert ((ao > 0) & (ao < f32(2.0 ** -126))).any()          # subnormals


def test_triangle_families_hold_both_answers_and_every_edge_class(tri):
    import test_cull_bound as tcb
    assert all(len(v[0]) <= 40000 for v in tri.values())
    u0 = v0 = uv1 = u1 = tnear = 0
    for name, (r, g, w) in tri.items():
        hit = w[:, 0] == 1
        _both_answers(name, hit, wpi.TRI_ALL_MISS)
        t, u, v = w[hit, 1], w[hit, 2], w[hit, 3]
        u0 += int((u == 0).sum()); v0 += int((v == 0).sum()); uv1 += int((u + v == 1).sum()); u1 += int((u == 1).sum())
        tnear += int((t <= wpi._up(wpi.EPS, 4)).sum())          # accepted within four ulp of the cut-off (t > EPSILON)
    assert min(u0, v0, uv1, u1, tnear) > 0, (u0, v0, uv1, u1, tnear)
    # the determinant ON the cut-off and on its float neighbours, both signs
    r, g, w = tri["det at the cut-off"]
    det = tcb.moller_trumbore_f32(r[:, :3], r[:, 3:], g[:, 0:3], g[:, 3:6], g[:, 6:9])[2]
    for s in (f32(1), f32(-1)):
        for v in (wpi.EPS, wpi._up(wpi.EPS), wpi._down(wpi.EPS)):
            assert (det == s * v).any(), (s, v)


def test_scene_rays_hold_both_answers(orc):
    hits = {}
    for sname, (nodes, tris, mats) in wpi.scenes().items():
        fam = wpi.scene_rays(nodes, tris)
        assert sum(len(r) for r in fam.values()) <= 12000
        osc = orc.OracleScene(tris, mats, nodes)
        for fname, r in fam.items():
            want, cnt = orc.ray_scene_n(osc, r)
            assert (cnt[:, 2] == 0).all()                       # no 64-entry abort on these trees
            hits.setdefault(fname, []).append(want[:, 0] == 1)
        if sname == wpi.TIE_SCENE:          # equal-t ties do occur there: the closest t of a ray is reached on several triangles
            r = fam["incoherent"]
            want, _ = orc.ray_scene_n(osc, r)
            r, want = r[want[:, 0] == 1][:64], want[want[:, 0] == 1][:64]
            abc = np.concatenate([tris["aPosition"], tris["bPosition"], tris["cPosition"]], 1)
            every = orc.ray_triangle_n(np.repeat(r, len(abc), 0), np.tile(abc, (len(r), 1))).reshape(len(r), len(abc), 4)
            ties = ((every[:, :, 0] == 1) & (every[:, :, 1] == want[:, 1:2])).sum(1)
            assert (ties >= 1).all() and (ties >= 2).sum() > len(r) // 2
    assert len(hits["incoherent"][0]) == 4096
    for fname, h in hits.items():
        _both_answers(fname, np.concatenate(h), wpi.SCENE_RAYS_ALL_MISS)
