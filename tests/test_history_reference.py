"""The validated merge of a held history on the CPU (include/mi3pt.h: mi3pt_merge_history): tests/history_reference.py, the numpy
restatement the kernel is held to, checked rule by rule, against an independent scalar walk through the header's lines, against float64
statistics of explicit sample sets, and on the use case -- a scene that changed under a carried mean (tests/history_cases.py)."""
import numpy as np
import pytest

import history_cases as hc
import history_reference as hr
import ptcommon as pc

F = np.float32
NAN = F(np.nan)


def _texel(mean, m2, n):
    """a 1 x 1 pair: (mean, mean, mean, 1), (m2, m2, m2, n)"""
    return np.array([[[mean, mean, mean, 1]]], F), np.array([[[m2, m2, m2, n]]], F)


def _merge1(live, held, **kw):
    a, m, info = hr.merge_history(live[0], live[1], held[0], held[1], **kw)
    return a[0, 0], m[0, 0], {k: bool(v[0, 0]) for k, v in info.items() if v.dtype == bool}


# ---------------------------------------------------------------- the rules, one texel at a time
def test_a_supported_history_is_merged_exactly():
    # n = nh = 4, per-sample variance 8 on both sides: V = 8 * (1/4 + 1/4) = 4, D = -2, z2 = 4 / (4 + 1e-8) < z_keep^2: everything is kept
    live, held = _texel(1, 24, 4), _texel(3, 24, 4)
    a, m, kind = _merge1(live, held, radius=0)
    assert kind["merged"] and list(a) == [2, 2, 2, 1] and list(m) == [56, 56, 56, 8]
    # 56 = the union's sum of squared deviations: 24 + 24 + 4 * 4 * (3 - 1)^2 / 8


@pytest.mark.parametrize("n,nh,kind", [(0, 5, "only_held"), (0.5, 5, "only_held"), (NAN, 5, "only_held"), (3, 0, "dropped"), (3, NAN, "dropped"),
                                       (3, 0.5, "dropped"), (0, 0, "neither"), (NAN, NAN, "neither"), (0, NAN, "neither")])
def test_a_pair_that_fails_on_either_side(n, nh, kind):
    live, held = _texel(1.5, 2, n), _texel(1.25, 7, nh)
    a, m, kinds = _merge1(live, held, radius=1)
    assert [k for k, v in kinds.items() if v] == [kind]
    want = held if kind == "only_held" else live
    assert pc.same_bits(a, want[0][0, 0]) and pc.same_bits(m, want[1][0, 0])


def test_fewer_than_one_kept_sample_drops_the_history():
    # the means differ by ten standard errors: lam = 0
    live, held = _texel(0, 3, 4), _texel(10, 63, 64)
    a, m, kind = _merge1(live, held, radius=0)
    assert kind["dropped"] and pc.same_bits(a, live[0][0, 0]) and pc.same_bits(m, live[1][0, 0])
    # one held sample: V = 1 * (1/4 + 1) = 1.25, D^2 = 11.25, z2 = 9 of z 2 / 4: lam = 7 / 12, and floor(1 * lam) = 0
    live, held = _texel(0, 3, 4), _texel(3.3541, 0, 1)
    a, m, info = hr.merge_history(*live, *held, radius=0)
    assert 0.5 < info["lam"][0, 0] < 0.6 and info["dropped"][0, 0] and info["nk"][0, 0] == 0
    assert pc.same_bits(a, live[0]) and pc.same_bits(m, live[1])
    # 64 held samples at a score in between: V = 1/4 + 1/64, D^2 = 2.25, z2 = 8.47, lam = 0.627: floor(64 * lam) = 40 are kept
    live, held = _texel(0, 3, 4), _texel(1.5, 0, 64)
    a, m, info = hr.merge_history(*live, *held, radius=0)
    assert info["merged"][0, 0] and info["nk"][0, 0] == 40 and m[0, 0, 3] == 44
    assert a[0, 0, 0] == F(0) + F(1.5) * (F(40) / F(44)) and m[0, 0, 0] == (F(3) + F(0) * F(39)) + F(2.25) * (F(4) * (F(40) / F(44)))


def test_outside_the_rectangle_nothing_changes_and_nothing_counts():
    # texel 1 disagrees violently; at radius 1 it pools with texel 0 -- unless the rectangle ends between them
    A = np.array([[[1, 1, 1, 1], [0, 0, 0, 1]]], F)
    M = np.array([[[24, 24, 24, 4], [3, 3, 3, 4]]], F)
    Ah = np.array([[[3, 3, 3, 1], [900, 900, 900, 1]]], F)
    Mh = np.array([[[24, 24, 24, 4], [3, 3, 3, 4]]], F)
    a, m, info = hr.merge_history(A, M, Ah, Mh, None, radius=1)
    assert info["dropped"].all() and pc.same_bits(a, A) and pc.same_bits(m, M)
    a, m, info = hr.merge_history(A, M, Ah, Mh, (1, 1), radius=1)
    assert info["merged"][0, 0] and list(a[0, 0]) == [2, 2, 2, 1] and list(m[0, 0]) == [56, 56, 56, 8]
    assert pc.same_bits(a[0, 1], A[0, 1]) and pc.same_bits(m[0, 1], M[0, 1]) and not any(v[0, 1] for v in info.values() if v.dtype == bool)


def _scalar_law(A, M, Ah, Mh, rect, r, z_keep, z_drop, f16):
    """the header's lines for one texel after the other, numpy fp32 scalars, no arrays: independent of history_reference's canvas"""
    rows, w = A.shape[:2]
    res_w, res_h = rect
    eps, one, zero = F(1e-8), F(1), F(0)

    def var(m2, n):
        return np.fmax(m2 / (n - one), zero) if n >= F(2) else zero

    def pair(qx, qy):
        return 0 <= qx < w and 0 <= qy < rows and qx < res_w and qy < res_h and M[qy, qx, 3] >= one and Mh[qy, qx, 3] >= one

    out_a, out_m = A.copy(), M.copy()
    with np.errstate(all="ignore"):
        for y in range(min(rows, res_h)):
            for x in range(min(w, res_w)):
                n, nh = M[y, x, 3], Mh[y, x, 3]
                if not n >= one:
                    if nh >= one:
                        out_a[y, x], out_m[y, x] = Ah[y, x], Mh[y, x]
                    continue
                if not nh >= one:
                    continue
                D, V = [zero] * 3, [zero] * 3
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        qx, qy = x + dx, y + dy
                        if not pair(qx, qy):
                            continue
                        wq = one / M[qy, qx, 3] + one / Mh[qy, qx, 3]
                        for k in range(3):
                            D[k] = D[k] + (A[qy, qx, k] - Ah[qy, qx, k])
                            V[k] = V[k] + np.fmax(var(M[qy, qx, k], M[qy, qx, 3]), var(Mh[qy, qx, k], Mh[qy, qx, 3])) * wq
                z = [(D[k] * D[k]) / (V[k] + eps) for k in range(3)]
                z2 = np.fmax(np.fmax(z[0], z[1]), z[2])
                drop2, keep2 = F(z_drop) * F(z_drop), F(z_keep) * F(z_keep)
                lam = np.fmin(np.fmax((drop2 - z2) / (drop2 - keep2), zero), one)
                nk = np.floor(nh * lam)
                if not nk >= one:
                    continue
                N = n + nk
                f = nk / N
                for k in range(3):
                    d = Ah[y, x, k] - A[y, x, k]
                    v = A[y, x, k] + d * f
                    out_a[y, x, k] = F(np.float16(v)) if f16 else v
                    out_m[y, x, k] = (M[y, x, k] + var(Mh[y, x, k], nh) * (nk - one)) + (d * d) * (n * f)
                out_a[y, x, 3] = one
                out_m[y, x, 3] = N
    return out_a, out_m


def _random_pair(rng, w, h, near=None):
    acc = (rng.random((h, w, 4), dtype=F) * 4).astype(F)
    acc[..., 3] = 1
    mo = rng.random((h, w, 4), dtype=F)
    mo[..., 3] = rng.choice(np.array([0, 1, 2, 500, np.nan], F), size=(h, w), p=[0.12, 0.15, 0.2, 0.5, 0.03])
    mo[..., :3] *= np.fmax(mo[..., 3:], F(1))
    if near is not None:
        step = (rng.random((h, w, 3), dtype=F) - F(0.5)) * rng.choice(np.array([0.0, 0.05, 0.5], F), size=(h, w, 1))
        acc[..., :3] = np.where(rng.random((h, w, 1)) < 0.7, near[..., :3] + step, acc[..., :3])
    return acc, mo


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
def test_the_window_clipped_by_image_and_rectangle_equals_a_scalar_walk(radius):
    """7 x 5 (radius 3: most windows leave the image), the whole image and a rectangle, F32 and F16; F16 rounds the mean only"""
    rng = np.random.default_rng(40 + radius)
    w, h = 7, 5
    held = _random_pair(rng, w, h)
    live = _random_pair(rng, w, h, near=held[0])
    live[1][1, 1, 3], held[1][1, 1, 3] = 0, NAN          # (35 texels: one without samples on either side is planted)
    seen = set()
    for rect in ((w, h), (w - 2, h - 1)):
        plain = hr.merge_history(*live, *held, rect, radius)
        want = _scalar_law(*live, *held, rect, radius, 2.0, 4.0, False)
        assert pc.same_bits(plain[0], want[0]) and pc.same_bits(plain[1], want[1]), rect
        half = hr.merge_history(*live, *held, rect, radius, store_f16=True)
        want = _scalar_law(*live, *held, rect, radius, 2.0, 4.0, True)
        assert pc.same_bits(half[0], want[0]) and pc.same_bits(half[1], want[1]), rect
        merged = plain[2]["merged"]
        assert pc.same_bits(half[1], plain[1])                       # the moments do not see the rounding
        assert pc.same_bits(half[0][~merged], plain[0][~merged])     # ... and neither does a texel that only keeps or takes bits
        assert pc.same_bits(half[0][merged][:, :3], plain[0][merged][:, :3].astype(np.float16).astype(F))
        assert not pc.same_bits(half[0][merged], plain[0][merged])
        seen |= {k for k in ("merged", "dropped", "only_held", "neither") if plain[2][k].any()}
        ys, xs = np.mgrid[0:h, 0:w]
        outside = (xs >= rect[0]) | (ys >= rect[1])
        assert pc.same_bits(plain[0][outside], live[0][outside]) and pc.same_bits(plain[1][outside], live[1][outside])
    assert seen == {"merged", "dropped", "only_held", "neither"}


# ---------------------------------------------------------------- against float64 statistics of explicit samples
def test_keeping_everything_is_the_union_of_the_two_sample_sets():
    rng = np.random.default_rng(7)
    w, h, n, nh = 6, 5, 5, 20
    fresh = rng.normal(1.0, 0.5, (n, h, w, 3))
    carried = rng.normal(1.4, 0.8, (nh, h, w, 3))

    def pair(samples):
        mean = samples.mean(axis=0)
        m2 = ((samples - mean) ** 2).sum(axis=0)
        count = np.full((h, w, 1), len(samples))
        return np.concatenate([mean, np.ones((h, w, 1))], axis=-1).astype(F), np.concatenate([m2, count], axis=-1).astype(F)

    a, m, info = hr.merge_history(*pair(fresh), *pair(carried), radius=1, z_keep=1e6, z_drop=2e6)
    union = np.concatenate([fresh, carried])
    mean = union.mean(axis=0)
    m2 = ((union - mean) ** 2).sum(axis=0)
    assert info["merged"].all() and np.all(m[..., 3] == n + nh) and np.all(info["nk"] == nh)
    assert np.abs(a[..., :3] / mean - 1).max() <= 1e-5 and np.abs(m[..., :3] / m2 - 1).max() <= 1e-5


@pytest.mark.parametrize("seed", [1])
def test_gaussian_samples_keep_an_unchanged_half_and_drop_a_shifted_one(seed):
    """48 x 32, 4 fresh and 64 carried samples per texel and channel of N(1, 0.5^2); the carried samples of the right half shifted by one
    sigma.  Radius 2, z 2 / 4; measured radius + 1 away from the borders and the seam.  Issue's conditions: left: kept >= 0.95 and the
    validated RMSE <= 1.05 x merging at once; right: kept <= 0.02 and the validated RMSE <= 1.05 x the fresh samples' own"""
    rng = np.random.default_rng(seed)
    w, h, n, nh, r = 48, 32, 4, 64, 2
    fresh = rng.normal(1.0, 0.5, (n, h, w, 3))
    carried = rng.normal(1.0, 0.5, (nh, h, w, 3))
    carried[:, :, w // 2:] += 0.5

    def pair(samples):
        mean = samples.mean(axis=0)
        m2 = ((samples - mean) ** 2).sum(axis=0)
        count = np.full((h, w, 1), len(samples))
        return np.concatenate([mean, np.ones((h, w, 1))], axis=-1).astype(F), np.concatenate([m2, count], axis=-1).astype(F)

    live, held = pair(fresh), pair(carried)
    a, m, _ = hr.merge_history(*live, *held, radius=r, z_keep=2.0, z_drop=4.0)
    at_once = (n * live[0].astype(np.float64) + nh * held[0].astype(np.float64)) / (n + nh)
    ys, xs = np.mgrid[0:h, 0:w]
    rows = (ys >= r + 1) & (ys < h - r - 1)
    left = rows & (xs >= r + 1) & (xs < w // 2 - r - 1)
    right = rows & (xs >= w // 2 + r + 1) & (xs < w - r - 1)
    rmse = lambda img, sel: float(np.sqrt(((np.asarray(img, np.float64)[..., :3][sel] - 1.0) ** 2).mean()))
    kept_l, kept_r = hr.kept_share(live[1], m, held[1], left), hr.kept_share(live[1], m, held[1], right)
    print(f"seed {seed}: left: kept {kept_l:.4f}, validated {rmse(a, left):.5f}, at once {rmse(at_once, left):.5f}, fresh {rmse(live[0], left):.5f}; "
          f"right: kept {kept_r:.4f}, validated {rmse(a, right):.5f}, at once {rmse(at_once, right):.5f}, fresh {rmse(live[0], right):.5f}")
    assert kept_l >= 0.95 and rmse(a, left) <= 1.05 * rmse(at_once, left)
    assert kept_r <= 0.02 and rmse(a, right) <= 1.05 * rmse(live[0], right)


# ---------------------------------------------------------------- the use case
@pytest.fixture(scope="module")
def use_case(orc, demo):
    return hc.UseCase(orc, demo)


@pytest.mark.parametrize("change", hc.CHANGES)
def test_a_validated_history_beats_merging_at_once_and_a_restart(use_case, change):
    """Demo scene, 48 x 32, four bounces, the sun-less sky, fixed camera: 64 frames, the change, reproject_scene's reference with its
    defaults, K = 4 fresh frames, radius 1, z 2 / 4; yardstick: 1 024 frames of the new scene, tone-mapped RMSE over its hit texels.
    Measured (fresh alone / merged at once / validated, kept share): nothing 0.0411 / 0.0104 / 0.0104, 0.996; repaint 0.0396 / 0.0916 /
    0.0269, 0.709; slide 0.0454 / 0.0368 / 0.0355, 0.951; dimmed 0.0282 / 0.1175 / 0.0282, 0.000.  Only orderings are asserted."""
    row = use_case.measure(change, frames=4, radius=1)
    print(f"{change}: 4 frames alone {row['alone']:.5f}, merged at once {row['at_once']:.5f}, held / validated / merged {row['validated']:.5f}, "
          f"kept share {row['kept']:.4f}")
    if change == "nothing":
        assert row["validated"] < row["alone"] and row["kept"] >= 0.95
    elif change in ("repaint", "slide"):
        assert row["validated"] < row["at_once"] and row["validated"] < row["alone"]
    else:
        assert row["validated"] <= 1.02 * row["alone"] and row["kept"] <= 0.02
