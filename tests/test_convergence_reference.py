"""tests/convergence_reference.py on its own, without a device: exact small cases of the definition in include/mi3pt.h
(mi3pt_estimate_convergence), and its calibration against the error the project reports -- the RMSE of x / (1 + x) -- in the setting of
test_moments_reference.py::test_variance_guided_filter_wins_from_sixteen_frames_on."""
import numpy as np

import convergence_cases as cc
import convergence_reference as cr
import moments_reference as mr
import ptcommon as pc
from mi3pt_host import scenes

F = np.float32


def _images(rows, w, mean=0.0, moments=(0, 0, 0, 0)):
    acc = np.zeros((rows, w, 4), F)
    acc[..., :3] = mean
    acc[..., 3] = 1
    mo = np.zeros((rows, w, 4), F)
    mo[...] = moments
    return acc, mo


def test_a_single_texel():
    """1 x 1: M2 = (1, 2, 3), n = 4 -> v = 6 / 12; mean 1 -> d4 = 16; r = 0.5 / 16"""
    acc, mo = _images(1, 1, 1.0, (1, 2, 3, 4))
    tiles, s = cr.estimate(acc, mo, 0.5, 4)
    assert tiles.shape == (1, 1, 4) and tiles.dtype == F
    assert tiles[0, 0].tolist() == [0.03125, 0.03125, 1.0, 4.0]
    assert s == {"tiles": 1, "tiles_above": 0, "tiles_young": 0, "tiles_nonfinite": 0, "texels": 1, "worst_tile": F(0.03125),
                 "worst_texel": F(0.03125), "n_min": F(4), "threshold": F(0.5)}
    assert cr.converged(s)
    # 0.03125 <= 3 t^2 exactly at t^2 = 1 / 96: just below it the tile is above
    assert cr.summary(tiles, 0.102, 4)["tiles_above"] == 1 and cr.summary(tiles, 0.1021, 4)["tiles_above"] == 0


def test_the_sample_count_decides_what_counts_and_what_varies():
    """n = 0: not counted; n = 1 and 1.5: counted, v = 0; n = 2: v = s / 2"""
    acc, mo = _images(1, 4, 0.0)
    mo[0, :, :3] = (1, 2, 3)
    mo[0, :, 3] = (0, 1, 1.5, 2)
    counts, r = cr.texel_error(acc, mo)
    assert counts.tolist() == [[False, True, True, True]]
    assert r.tolist() == [[0.0, 0.0, 0.0, 3.0]]
    tiles, s = cr.estimate(acc, mo, 10.0, 0)
    assert tiles[0, 0].tolist() == [3.0, 3.0, 3.0, 1.0]
    assert s["texels"] == 3 and s["n_min"] == 1 and s["worst_tile"] == 1.0 and s["worst_texel"] == 3.0
    nan_n = mo.copy()
    nan_n[0, 3, 3] = np.nan                                             # a NaN n does not count
    assert cr.tile_map(acc, nan_n)[0, 0].tolist() == [0.0, 0.0, 2.0, 1.0]


def test_negative_and_nan_sums_of_squares_have_no_variance():
    acc, mo = _images(1, 2, 0.0)
    mo[0, 0] = (-1, -2, -3, 4)
    mo[0, 1] = (np.nan, 1, 1, 4)
    tiles, s = cr.estimate(acc, mo, 0.0, 0)
    assert tiles[0, 0].tolist() == [0.0, 0.0, 2.0, 4.0]
    assert cr.converged(s) and s["tiles_nonfinite"] == 0               # threshold 0: a tile without variance passes (0 <= 0)


def test_threshold_zero_keeps_any_variance_above():
    acc, mo = _images(8, 8, 0.0, (1e-30, 0, 0, 2))
    _, s = cr.estimate(acc, mo, 0.0, 0)
    assert s["tiles"] == 1 and s["tiles_above"] == 1 and s["tiles_young"] == 0 and not cr.converged(s)


def test_the_mean_enters_through_its_brightness_clamped_at_zero():
    acc, mo = _images(1, 3, 0.0, (6, 0, 0, 3))                         # v = 1
    acc[0, 0, :3] = (-5, -5, -5)                                        # a negative mean: m = 0
    acc[0, 1, :3] = (0, 1, 2)                                           # m = 1: r = 1 / 16
    acc[0, 2, :3] = (3e10, 3e10, 3e10)                                     # d4 overflows: r = 0
    _, r = cr.texel_error(acc, mo)
    assert r.tolist() == [[1.0, 0.0625, 0.0]]


def test_a_nan_mean_is_above_and_nonfinite():
    acc, mo = _images(8, 16, 0.5, (3, 3, 3, 8))
    acc[3, 2, 1] = np.nan                                               # in the left tile
    tiles, s = cr.estimate(acc, mo, 100.0, 0)
    assert np.isnan(tiles[0, 0, 0]) and tiles[0, 0, 2] == 64 and np.isfinite(tiles[0, 0, 1])      # fmax drops the NaN
    assert np.isfinite(tiles[0, 1]).all()
    assert s["tiles"] == 2 and s["tiles_above"] == 1 and s["tiles_nonfinite"] == 1 and s["tiles_young"] == 0
    assert np.isfinite(s["worst_tile"]) and s["worst_tile"] == tiles[0, 1, 0] / F(64)
    # an infinite variance over an infinite d4 is a NaN too; an infinite variance alone an infinite sum
    acc, mo = _images(1, 2, 0.0, (np.inf, 0, 0, 2))
    acc[0, 0, :3] = 3e10
    t2 = cr.tile_map(acc[:, :1], mo[:, :1])
    assert np.isnan(t2[0, 0, 0]) and t2[0, 0, 1] == 0
    t3, s3 = cr.estimate(acc[:, 1:], mo[:, 1:], 100.0, 0)
    assert np.isposinf(t3[0, 0, 0]) and s3["tiles_nonfinite"] == 1 and s3["tiles_above"] == 1 and np.isposinf(s3["worst_texel"])


def test_an_uncounted_tile_is_the_zero_record():
    acc, mo = _images(8, 16, 1.0, (1, 1, 1, 5))
    mo[:, 8:, 3] = 0                                                    # the right tile was never accumulated
    mo[:, 8:, :3] = 7
    tiles, s = cr.estimate(acc, mo, 1.0, 0)
    assert tiles[0, 1].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert s["tiles"] == 1 and s["texels"] == 64
    none, s0 = cr.estimate(acc, np.zeros_like(mo), 1.0, 0)
    assert not none.any()
    assert s0 == {"tiles": 0, "tiles_above": 0, "tiles_young": 0, "tiles_nonfinite": 0, "texels": 0, "worst_tile": F(0),
                  "worst_texel": F(0), "n_min": F(0), "threshold": F(1)}
    assert not cr.converged(s0)                                         # nothing counted is not convergence


def test_young_tiles_are_above_whatever_their_variance():
    acc, mo = _images(8, 16, 0.0, (0, 0, 0, 16))
    mo[5, 9, 3] = 15                                                    # one texel of the right tile has seen 15 frames
    _, s = cr.estimate(acc, mo, 1.0, 16)
    assert s["tiles"] == 2 and s["tiles_young"] == 1 and s["tiles_above"] == 1 and s["n_min"] == 15
    assert cr.converged(cr.estimate(acc, mo, 1.0, 15)[1])


def test_partial_tiles_and_the_fixed_tree():
    """9 x 17: 2 x 3 tiles, the edge tiles hold 1 x 8, 8 x 1 and 1 x 1 texels; the tree is not the left-to-right sum"""
    rng = np.random.default_rng(3)
    acc, mo = _images(9, 17, 0.0)
    acc[..., :3] = rng.random((9, 17, 3), dtype=F)
    mo[..., :3] = rng.random((9, 17, 3), dtype=F)
    mo[..., 3] = 7
    tiles = cr.tile_map(acc, mo)
    assert tiles.shape == (2, 3, 4)
    assert tiles[..., 2].tolist() == [[64, 64, 8], [8, 8, 1]]
    _, r = cr.texel_error(acc, mo)
    assert tiles[1, 2, 0] == r[8, 16] and tiles[1, 2, 1] == r[8, 16]
    lanes = r[:8, :8].reshape(64)
    a = lanes.copy()
    for s in (32, 16, 8, 4, 2, 1):
        a = a[:s] + a[s:2 * s]
    assert tiles[0, 0, 0] == a[0]
    assert abs(float(tiles[0, 0, 0]) - float(lanes.astype(np.float64).sum())) < 1e-4
    assert cr.tree_sum(np.arange(64, dtype=F)) == 2016


def test_a_group_combines_its_members():
    a = {"tiles": 2, "tiles_above": 1, "tiles_young": 0, "tiles_nonfinite": 0, "texels": 100, "worst_tile": F(0.5), "worst_texel": F(2),
         "n_min": F(6), "threshold": F(0.1)}
    b = dict(a, tiles=0, tiles_above=0, texels=0, worst_tile=F(0), worst_texel=F(0), n_min=F(0))       # a member without rows
    c = dict(a, tiles=3, texels=150, worst_tile=F(0.25), worst_texel=F(3), n_min=F(4))
    s = cr.combine([a, b, c])
    assert s == dict(a, tiles=5, tiles_above=2, texels=250, worst_tile=F(0.5), worst_texel=F(3), n_min=F(4))


def test_placed_extremes_move_every_field_a_dropped_record_would_lose():
    """tests/convergence_cases.py, the inputs of tests/test_gpu_convergence.py::test_summary_placed_extremes: 260 block records, more
    than the 256 one round of the fold takes; for every placed record p the one texel lies in a tile of record p and the summary differs
    from the base image's in tiles_above, tiles_young, worst_tile, worst_texel and n_min -- each decided by that tile alone"""
    assert (cc.RECORDS, cc.TILES_X * cc.TILES_Y) == (260, 4160) and cc.RECORDS > cc.FOLD_WIDTH
    assert set(cc.PLACED) >= {1, 2, 4, 8, 16, 32, 64, 128} and max(cc.PLACED) == cc.RECORDS - 1      # every stage's upper half; the last record
    assert any(cc.FOLD_WIDTH <= p < cc.RECORDS for p in cc.PLACED) and cc.FOLD_WIDTH - 1 in cc.PLACED
    base_tiles = cr.tile_map(*cc.base())
    assert np.all(base_tiles == base_tiles[0, 0]) and base_tiles[0, 0, 2] == 64 and base_tiles[0, 0, 3] == 16
    for threshold, min_frames in cc.PLACED_PARAMS:
        s0 = cr.summary(base_tiles, threshold, min_frames)
        assert (s0["tiles"], s0["tiles_above"], s0["tiles_young"], s0["tiles_nonfinite"], s0["texels"]) == (4160, 0, 0, 0, cc.W * cc.H)
        assert s0["n_min"] == 16 and s0["worst_texel"] == base_tiles[0, 0, 1] and s0["worst_tile"] == base_tiles[0, 0, 0] / F(64)
        seen = set()
        for p in cc.PLACED:
            y, x = cc.placed_texel(p)
            t = (y // 8) * cc.TILES_X + x // 8
            assert t // cc.RECORD_TILES == p
            seen.add((t % cc.RECORD_TILES, (y % 8) * 8 + x % 8))
            tiles = cr.tile_map(*cc.placed(p))
            flat = tiles.reshape(-1, 4)
            others = np.delete(flat, t, axis=0)
            assert np.all(others == base_tiles[0, 0])                        # one tile differs
            s = cr.summary(tiles, threshold, min_frames)
            assert (s["tiles"], s["tiles_above"], s["tiles_young"], s["texels"]) == (4160, 1, 1 if min_frames else 0, cc.W * cc.H)
            assert s["n_min"] == 15 == flat[t, 3] and s["n_min"] < s0["n_min"]
            assert s["worst_texel"] == flat[t, 1] > s0["worst_texel"]
            assert s["worst_tile"] == flat[t, 0] / F(64) > s0["worst_tile"]
            assert not cr.same_summary(s, s0)
        assert len(seen) == len(cc.PLACED)                                   # (another place in the record and the tile every time)


def test_the_replayed_loop_stops_where_the_estimates_say():
    say = {16: False, 32: False, 48: True, 64: True, 80: True}
    est = lambda frames: {"tiles": 1, "tiles_above": 0 if say[frames] else 1}
    assert cr.render_until(est, 80, 16, lookahead=False)[:2] == (True, 48)
    assert cr.render_until(est, 80, 16, lookahead=True)[:2] == (True, 64)          # one chunk after the estimate that said so
    assert cr.render_until(est, 32, 16, lookahead=True)[:2] == (False, 32)
    assert cr.render_until(est, 48, 16, lookahead=True)[:2] == (True, 48)          # the final estimate at the budget


def _tone_sq(x, truth):
    a = np.asarray(x, np.float64)[..., :3]
    b = np.asarray(truth, np.float64)[..., :3]
    return ((a / (1 + a) - b / (1 + b)) ** 2).sum(axis=-1)


def test_calibration_against_the_tone_mapped_error(orc, demo):
    """The demo scene at 96 x 96 under the sun-less sky, four bounces, truth = the mean of frames 1000 .. 3999.  At 8, 16, 64 and 256 frames
    the whole-image estimate sqrt(mean r / 3) over the actual RMSE of x / (1 + x) lies in [0.9, 1.2] (measured 1.069, 1.048, 1.055,
    1.011: the margin is for another libm / summation order and the truth's own noise) and the per-tile estimate correlates with the
    per-tile squared error at >= 0.85 (measured 0.925 .. 0.958)."""
    w = h = 96
    env = scenes.synthetic_env(sun_radiance=0.0)
    osc = pc.oracle_scene(orc, demo, env)
    truth = np.zeros((h, w, 4), np.float64)
    for f in range(1000, 4000):
        truth += orc.raytrace(osc, pc.rt_uniforms(demo, w, h, frame=f, bounces=4).tobytes(), w, h)[0]
    truth /= 3000
    mean = np.zeros((h, w, 4), F)
    moments = None
    for k in range(256):
        img, _ = orc.raytrace(osc, pc.rt_uniforms(demo, w, h, frame=2 + k, bounces=4).tobytes(), w, h)
        new = orc.accumulate(pc.acc_uniforms(w, h, 1 + k).tobytes(), w, h, img, mean)
        moments = mr.welford([img], [mean], [new], [1 + k], moments=moments)
        mean = new
        frames = k + 1
        if frames not in (2, 4, 8, 16, 32, 64, 128, 256):
            continue
        tiles = cr.tile_map(mean, moments)
        assert tiles.shape == (12, 12, 4) and np.all(tiles[..., 2] == 64) and np.all(tiles[..., 3] == frames)
        predicted = cr.rmse_estimate(tiles)
        sq = _tone_sq(mean, truth)
        actual = float(np.sqrt(sq.mean() / 3))
        per_tile = sq.reshape(12, 8, 12, 8).sum(axis=(1, 3))
        corr = float(np.corrcoef(tiles[..., 0].astype(np.float64).ravel(), per_tile.ravel())[0, 1])
        print(f"{frames} frames: predicted {predicted:.5f}  actual {actual:.5f}  ratio {predicted / actual:.3f}  per-tile correlation {corr:.3f}")
        if frames in (8, 16, 64, 256):
            assert 0.9 <= predicted / actual <= 1.2, frames
            assert corr >= 0.85, frames
