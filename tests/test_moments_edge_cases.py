"""tests/moments_edge_cases.py without a device: every numpy restatement that reads the (mean, moments) pair run over the catalogue, with
the inputs the GPU tests write (same builders, sizes and seeds) and the ORACLE's feature images where the device's own are used there.
Asserted on the references alone: every value branch of each law is taken by a placed texel, the worked examples hold, the guided
filters have weights in the fp32 subnormal range that a flushing build would lose, and the non-finite cases stay mostly not-NaN, so that
the GPU comparison has something to compare.  The printout states the branch counts, the subnormal tap counts and the NaN shares."""
import numpy as np
import pytest

import aov_reference as ar
import guided_reference as gr
import history_reference as hr
import moments_edge_cases as ec
import moments_reference as mr
import ptcommon as pc
import reproject_reference as rr
import reproject_scene_cases as cases
import reproject_scene_reference as rs
import test_gpu_guided as gg
import test_gpu_guided_variance as gv
import test_gpu_history as tgh
import test_gpu_reproject as tgr

F = np.float32


# ---------------------------------------------------------------- the catalogue itself
def test_the_catalogue_holds_what_it_names_and_places_it_at_the_seams():
    counts = [v for _, v, _ in ec.COUNTS]
    assert len(counts) == 15 and np.isnan(counts[0]) and np.isinf(counts[-1]) and F(0.99999994) in counts and F(1.9999999) in counts
    assert [v for _, v, f in ec.MEANS if f][4:7] == [F(65504), F(65519.996), F(65520)]
    assert rr.store_round(F(65519.996), True) == 65504 and np.isinf(rr.store_round(F(65520), True)) and 0 < rr.store_round(F(6e-8), True) < 6.2e-5
    assert 0 < F(1e-42) < F(2.0 ** -126) and np.signbit(F(-0.0))
    for w, h, kw in ((40, 24, {}), (48, 32, {}), (50, 37, dict(linear=256)), (100, 52, dict(pitch=6))):
        for finite in (True, False):
            mean, mo, where = ec.placed(w, h, 1, finite, **kw)
            assert set(where) == {e[0] for e in ec.entries(finite)} and not ec.seam_sides(where, w, h)
            assert np.isfinite(mean).all() == finite and np.isfinite(mo).all() == finite
            edge = np.zeros((h, w), bool)
            for at in where.values():
                for y, x in at:
                    edge[y, x] = True
            # around every placed texel a radius-3 window (k_history: the lattice of three) holds other edge texels AND plain ones; a 5 x 5
            # window four apart (the guided filter's third level) holds plain ones beside its centre
            for y, x in zip(*np.nonzero(edge)):
                near = edge[max(0, y - 3):y + 4, max(0, x - 3):x + 4]
                wide = edge[np.ix_([y + 4 * k for k in range(-2, 3) if 0 <= y + 4 * k < h], [x + 4 * k for k in range(-2, 3) if 0 <= x + 4 * k < w])]
                assert (near.sum() >= 2 or "pitch" in kw) and not near.all() and wide.size > 1 and not wide.all(), (w, h, y, x)
    w, h = 50, 37
    _, _, where = ec.placed(w, h, 1, False, linear=256)
    flat = {y * w + x for at in where.values() for y, x in at}
    assert all({k - 1, k} <= flat for k in range(256, w * h, 256))          # both sides of k_accumulate_frames' block seams


# ---------------------------------------------------------------- the mean by count
def test_by_count_worked_examples_and_branches():
    for n, (mean, m2, count) in ec.BY_COUNT:
        p, m = rr.by_count_step(np.array([[[2, 2, 2, 1]]], F), np.array([[[1, 1, 1, n]]], F), np.array([[[3, 3, 3, 1]]], F))
        assert pc.same_bits(p[0, 0], [mean, mean, mean, 1]) and pc.same_bits(m[0, 0], [m2, m2, m2, count]), n
    w, h = 50, 37
    for f16 in (False, True):
        mean, mo, where = ec.placed(w, h, 5, finite=False, linear=256)
        mean = rr.store_round(mean, f16)
        n0 = mo[..., 3].copy()
        rng = np.random.default_rng(3)
        for k in range(4):
            mean, mo = rr.by_count_step(mean, mo, rng.random((h, w, 4), dtype=F) * 2, store_f16=f16)
        restart = ~(n0 >= 1)
        stuck = ~restart & (mo[..., 3] == n0)
        nan = float(np.isnan(mean).any(axis=-1).mean())
        print(f"by count, f16 {f16}: {int(restart.sum())} texels restart, {int((~restart).sum())} continue, {int(stuck.sum())} counts no longer grow, "
              f"{int((mo[..., 3] == 5.5).sum())} fractional; the mean holds a NaN in {nan:.3f} of the texels")
        assert restart.any() and (~restart).any() and stuck.any() and (mo[..., 3] == 5.5).any() and np.all(mo[..., 3][restart] == 4)
        for name in ("n=nan", "n=-1", "n=-0", "n=0", "n=0.5", "n=below 1"):
            assert all(restart[y, x] for y, x in where[name]), name
        for name in ("n=1", "n=1.5", "n=2^24", "n=inf"):
            assert not any(restart[y, x] for y, x in where[name]), name
        assert nan <= 0.5


# ---------------------------------------------------------------- the merge of a held history
def _texel(s):
    """a 1 x 1 pair from (mean.rgb, M2.rgb, n)"""
    return np.array([[[*s[0], 1]]], F), np.array([[[*s[1], s[2]]]], F)


@pytest.mark.parametrize("t", ec.THRESHOLDS, ids=[t["name"] for t in ec.THRESHOLDS])
def test_merge_worked_examples(t):
    a, m, info = hr.merge_history(*_texel(t["live"]), *_texel(t["held"]), radius=0, z_keep=t["z"][0], z_drop=t["z"][1])
    assert abs(float(info["lam"][0, 0]) - float(t["lam"])) <= 1e-9 and info["nk"][0, 0] == t["nk"]
    if t["merged"] is None:
        assert info["dropped"][0, 0] and pc.same_bits(a, _texel(t["live"])[0]) and pc.same_bits(m, _texel(t["live"])[1])
    else:
        assert info["merged"][0, 0] and (a[0, 0, 0], m[0, 0, 0], m[0, 0, 3]) == t["merged"]


@pytest.mark.parametrize("case", ec.Z_EXTREMES, ids=[c["name"] for c in ec.Z_EXTREMES])
def test_merge_parameter_extremes(case):
    """one texel with a difference of exactly 0 and one without, every sample count the same"""
    for diff, want in ((0.0, case["lam_d0"]), (0.25, case["lam"]), (1e-30, case["lam"])):
        _, _, info = hr.merge_history(*_texel(((F(1) + F(diff),) * 3, (2, 2, 2), 4)), *_texel(((1, 1, 1), (2, 2, 2), 4)), radius=0, z_keep=case["z"][0],
                                      z_drop=case["z"][1])
        if diff == 1e-30:
            assert F(1) + F(diff) == F(1) and info["lam"][0, 0] == case["lam_d0"]          # (absorbed: a difference of exactly 0 again)
        else:
            assert info["lam"][0, 0] == want, (diff, info["lam"][0, 0])
    # the images test_gpu_history.py::test_parameter_extremes merges
    held = tgh._random_pair(48, 32, 7)
    live = tgh._random_pair(48, 32, 107, near=held[0])
    _, _, info = hr.merge_history(*live, *held, radius=0, z_keep=case["z"][0], z_drop=case["z"][1])
    both = (live[1][..., 3] >= 1) & (held[1][..., 3] >= 1)
    d0 = both & (live[0][..., :3] == held[0][..., :3]).all(axis=-1)
    print(f"{case['name']}: {int(d0.sum())} of {int(both.sum())} texels with both sides have a difference of exactly 0")
    assert d0.sum() >= 20 and (both & ~d0).sum() >= 20
    assert np.all(info["lam"][d0] == case["lam_d0"]) and np.all(info["lam"][both & ~d0] == case["lam"])


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h", tgh.SIZES)
def test_merge_branches_over_the_finite_catalogue(w, h, radius):
    """the pairs of test_gpu_history.py::test_value_edges"""
    held, live = tgh.edge_pairs(w, h, 20 + radius, finite=True)
    a, m, info = hr.merge_history(*live, *held, radius=radius)
    count = tgh.describe_branches(info, live, held, f"radius {radius}, {w} x {h}")
    assert tgh._every_branch(info) and count["lam0"] and count["lam1"] and count["between"] and count["one_kept"]
    sf, sh = hr.per_sample_variance(live[1]), hr.per_sample_variance(held[1])
    for mo, var in ((live[1], sf), (held[1], sh)):          # the variance's own branches: n < 2, n >= 2, and a quotient the fmaxf clamps
        n = mo[..., 3]
        assert (n < 2).any() and (n >= 2).any() and ((n >= 2)[..., None] & (mo[..., :3] < 0) & (var == 0)).any()
    if radius == 1:
        held, live = tgh.edge_pairs(w, h, 30, finite=True)
        held, live = (rr.store_round(held[0], True), held[1]), (rr.store_round(live[0], True), live[1])
        _, _, info = hr.merge_history(*live, *held, radius=1, store_f16=True)
        assert (live[0] == 65504).any() and np.isinf(live[0]).any() and info["merged"].any()


@pytest.mark.parametrize("radius", [0, 3])
def test_merge_over_the_whole_catalogue_stays_mostly_not_nan(radius):
    """the pairs of test_gpu_history.py::test_non_finite_images.  A window with a NaN tap whose own texel is merged to something that is not
    a NaN: the fmaxf over the channels dropped it"""
    w, h = tgh.SIZES[0]
    rect = (w - 9, h - 5)
    held, live = tgh.edge_pairs(w, h, 40 + radius, finite=False)
    a, m, info = hr.merge_history(*live, *held, rect, radius=radius)
    tgh.describe_branches(info, live, held, f"non-finite, radius {radius}")
    assert tgh._every_branch(info)
    not_nan = ~np.isnan(a).any(axis=-1) & ~np.isnan(m).any(axis=-1)
    with np.errstate(all="ignore"):
        tap_nan = np.isnan(live[0][..., :3] - held[0][..., :3]).any(axis=-1) | np.isnan(hr.per_sample_variance(live[1])).any(axis=-1) \
            | np.isnan(hr.per_sample_variance(held[1])).any(axis=-1)
    pair = (live[1][..., 3] >= 1) & (held[1][..., 3] >= 1)
    ys, xs = np.mgrid[0:h, 0:w]
    tap_nan &= pair & (xs < rect[0]) & (ys < rect[1])
    window = np.zeros((h, w), bool)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            window |= gr._shift(tap_nan, dy, dx, False)
    survived = window & info["merged"] & not_nan
    print(f"non-finite, radius {radius}: {float(not_nan.mean()):.3f} of the texels without a NaN; {int(window.sum())} windows hold a NaN tap, "
          f"{int(survived.sum())} of them merge to something that is not a NaN")
    assert not_nan.mean() >= 0.5 and (survived.sum() >= 20 or radius == 0)


# ---------------------------------------------------------------- the two reprojections
@pytest.fixture(scope="module")
def views(orc, demo, env):
    """name -> (uniforms, the oracle's features) at 50 x 37: test_gpu_reproject.py's views, computed once and left unchanged"""
    w, h = tgr.SIZES[1]
    osc = pc.oracle_scene(orc, demo, env)
    out = {}
    for name in ("identical", "orbit"):
        u = tgr._uniforms(demo, w, h, None if name == "identical" else tgr._views(demo, w, h)[name])
        out[name] = (u, ar.reference(orc, osc, u.tobytes(), w, h))
    return out


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("max_history", [64, 1 << 24])
@pytest.mark.parametrize("name", ["identical", "orbit"])
def test_reproject_branches_over_the_catalogue(views, name, max_history, f16):
    """the images of test_gpu_reproject.py::test_value_edges, and the whole catalogue on top"""
    w, h = tgr.SIZES[1]
    old, new = views["identical"], views[name]
    f0 = rr.view_frame(old[0].tobytes())
    acc, mo, _ = ec.placed(w, h, 11, finite=True)
    a, m, info = rr.reproject(rr.store_round(acc, f16), mo, f0, (F(w), F(h)), new[1], old[1], (w, h), max_history=max_history, store_f16=f16)
    tgr.assert_value_branches(info, m, max_history, f"{name}, max_history {max_history}, f16 {f16}", capped=max_history == 64 or name == "identical")
    acc, mo, _ = ec.placed(w, h, 11, finite=False)
    a, m, info = rr.reproject(rr.store_round(acc, f16), mo, f0, (F(w), F(h)), new[1], old[1], (w, h), max_history=max_history, store_f16=f16)
    not_nan = float((~np.isnan(a).any(axis=-1) & ~np.isnan(m).any(axis=-1)).mean())
    print(f"the whole catalogue: {not_nan:.3f} of the texels without a NaN")
    assert not_nan >= 0.5


@pytest.mark.parametrize("max_history", [64, 1 << 24])
def test_reproject_scene_branches_over_the_catalogue(orc, demo, views, max_history):
    """the images of test_gpu_reproject_scene.py::test_value_edges: the box and the sphere moved, the camera orbited"""
    w, h = tgr.SIZES[1]
    sc = cases.box_moved_sphere_squashed(demo)
    u_old, old = views["identical"]
    u_new = views["orbit"][0]
    old = dict(old, ids=cases.triangle_indices(orc, demo, u_old.tobytes(), old, w, h))
    new = ar.reference(orc, pc.oracle_scene(orc, sc), u_new.tobytes(), w, h)
    new["ids"] = cases.triangle_indices(orc, sc, u_new.tobytes(), new, w, h)
    f0 = rr.view_frame(u_old.tobytes())
    for finite in (True, False):
        acc, mo, _ = ec.placed(w, h, 12, finite=finite)
        a, m, info = rs.reproject_scene(acc, mo, f0, (F(w), F(h)), new, old, (w, h), sc.triangles, demo.triangles, max_history=max_history,
                                        max_history_moved=8)
        if finite:
            tgr.assert_value_branches(info, m, max_history, f"scene, max_history {max_history}", capped=max_history == 64)
            n_moved = m[..., 3][info["carried"] & info["moved"]]
            assert (n_moved == 8).any() and (n_moved < 8).any()
        else:
            not_nan = float((~np.isnan(a).any(axis=-1) & ~np.isnan(m).any(axis=-1)).mean())
            print(f"the whole catalogue: {not_nan:.3f} of the texels without a NaN")
            assert not_nan >= 0.5


# ---------------------------------------------------------------- the guided filters
@pytest.fixture(scope="module")
def feat(orc, demo, env):
    w, h = gv.EDGE_SIZE
    return ar.reference(orc, pc.oracle_scene(orc, demo, env), pc.rt_uniforms(demo, w, h).tobytes(), w, h)


def _differs(a, b):
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def test_guided_weights_in_the_subnormal_range(orc, feat):
    """the images of test_gpu_guided.py::test_subnormal_weights: counted taps whose exp(...) is a subnormal, and a reference whose exp
    flushes them gives another image"""
    w, h = gg.EDGE_SIZE
    accum = gg.subnormal_accum(w, h)
    args = (feat["normal"], feat["position"], feat["albedo"], feat["ids"], gg.SUBNORMAL_LEVELS, *gg.SUBNORMAL_SIGMAS)
    want, stats = gr.guided(orc, accum, *args)
    flushed, _ = gr.guided(ec.FlushedExp(orc), accum, *args)
    changed = int(_differs(want, flushed).any(axis=-1).sum())
    print(f"plain filter: {stats['subnormal']} counted taps with a subnormal weight; flushing them changes {changed} texels")
    assert stats["subnormal"] >= 1 and changed >= 1 and np.isfinite(want).all()


def test_guided_variance_weights_in_the_subnormal_range(orc, feat):
    """the images of test_gpu_guided_variance.py::test_subnormal_weights"""
    w, h = gv.EDGE_SIZE
    accum, moments = gv.subnormal_pair(w, h)
    args = (feat["normal"], feat["position"], feat["albedo"], feat["ids"], gv.SUBNORMAL_LEVELS, *gv.SUBNORMAL_SIGMAS)
    want, var, stats = mr.guided_variance(orc, accum, moments, *args)
    flushed, _, _ = mr.guided_variance(ec.FlushedExp(orc), accum, moments, *args)
    changed = int(_differs(want, flushed).any(axis=-1).sum())
    print(f"variance filter: {stats['subnormal']} counted taps with a subnormal weight; flushing them changes {changed} texels")
    assert stats["subnormal"] >= 1 and changed >= 1 and np.isfinite(want).all()


@pytest.mark.parametrize("name", list(gv.SQUARED_SIGMAS))
def test_guided_variance_squared_weights_in_the_subnormal_range(orc, feat, name):
    """the images of test_gpu_guided_variance.py::test_subnormal_squared_weights: counted taps with a normal weight whose square is a
    subnormal, and a restatement that flushes those squares gives another variance image (and the same colour image: the squares enter
    the variance alone).  Bracketed: at ec = 40 no ring's variance is subnormal, at ec = 50 every square and every ring is exactly 0"""
    w, h = gv.EDGE_SIZE
    args = (feat["normal"], feat["position"], feat["albedo"], feat["ids"], 1, *gv.SQUARED_SIGMAS[name])
    got = {}
    for ec_value, delta in ec.SQUARED_DELTA.items():
        accum, moments, ring = gv.squared_pair(w, h, feat["ids"], delta)
        want, var, stats = mr.guided_variance(orc, accum, moments, *args)
        flushed, flushed_var, _ = mr.guided_variance(orc, accum, moments, *args, flush_squares=True)
        r = var[ring]
        got[ec_value] = (stats["squared_subnormal"], r, int(_differs(var, flushed_var)[ring].sum()))
        print(f"squared weights, {name}, ec {ec_value}: {stats['squared_subnormal']} counted taps with a normal weight and a subnormal square ("
              f"{stats['subnormal']} with a subnormal weight); of {r.size} ring texels {int((r == 0).sum())} hold 0 and {int(((r > 0) & (r < gr.TINY)).sum())} "
              f"a subnormal, the others {r[r > 0].min() if (r > 0).any() else 0:.3g} .. {r.max():.3g}; flushing the squares changes {got[ec_value][2]}")
        assert np.isfinite(want).all() and np.isfinite(var).all() and want.tobytes() == flushed.tobytes()
        assert (var[~ring] == flushed_var[~ring]).mean() > 0.99
    assert ring.sum() >= 20 * 40                                                      # twenty patches and more inside the hit classes
    stat, r, changed = got[45]
    assert stat >= got[50][0] + 1000 and changed >= 0.9 * r.size and ((r > 0) & (r < gr.TINY)).sum() >= 100
    assert ((r == 0) | (r >= F(1e-40))).all() and r.max() <= F(2e-36)
    r40 = got[40][1]
    assert not ((r40 > 0) & (r40 < gr.TINY)).any() and (r40 > 0).mean() >= 0.99
    assert not got[50][1].any() and got[50][2] == 0


def test_guided_variance_branches_and_nan_shares(orc, feat):
    """the images of test_gpu_guided_variance.py::test_count_and_m2_catalogue and ::test_non_finite_colours, and of
    test_gpu_guided.py::test_non_finite_colours"""
    w, h = gv.EDGE_SIZE
    accum, moments, where = gv.catalogue_pair(w, h)
    n, v = moments[..., 3], mr.variance_of_mean(moments)
    with np.errstate(all="ignore"):
        negative = ((moments[..., 0] + moments[..., 1]) + moments[..., 2]) / (n * (n - 1)) < 0
    print(f"variance of the mean: {int((n < 2).sum())} texels with n < 2, {int((n >= 2).sum())} with n >= 2, {int(((n >= 2) & negative).sum())} clamped, "
          f"{int(np.isnan(n).sum())} NaN counts")
    assert (n < 2).any() and (n >= 2).any() and ((n >= 2) & negative & (v == 0)).any() and np.isnan(n).any()
    assert all(v[y, x] == 0 for name in ("n=nan", "n=1.5", "n=below 2", "n=-1") for y, x in where[name])
    assert not ec.seam_sides(where, w, h)
    args = (feat["normal"], feat["position"], feat["albedo"], feat["ids"])
    want, var, stats = mr.guided_variance(orc, accum, moments, *args, 3, *gv.SIGMAS)
    shares = float(np.isnan(want).any(axis=-1).mean()), float(np.isnan(var).mean())
    print(f"count and M2 catalogue, 3 levels: a NaN in {shares[0]:.3f} of the colour's texels and {shares[1]:.3f} of the variance's")
    assert shares[0] <= 0.5 and shares[1] <= 0.5
    accum = gv.non_finite_accum(w, h)
    want, var, _ = mr.guided_variance(orc, accum, gv._random_moments(w, h), *args, 2, *gv.SIGMAS)
    plain, _ = gr.guided(orc, accum, *args, 2, *gg.ALL_ON)
    shares = float(np.isnan(want).any(axis=-1).mean()), float(np.isnan(plain).any(axis=-1).mean())
    print(f"non-finite colours, 2 levels: a NaN in {shares[0]:.3f} of the variance filter's texels and {shares[1]:.3f} of the plain filter's")
    assert 0 < shares[0] <= 0.5 and 0 < shares[1] <= 0.5
