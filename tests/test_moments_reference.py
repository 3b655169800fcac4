"""tests/moments_reference.py held to what the moments image and the variance-guided filter are FOR, on the CPU alone: exact small cases
of Welford's update, its agreement with the two-pass float64 sample variance of the oracle's frames, and the quality ordering the
variance mode was built for.  (tests/test_gpu_moments.py and tests/test_gpu_guided_variance.py hold the device to that reference bit
for bit.)"""
import numpy as np
import pytest

import aov_reference as ar
import guided_reference as gr
import moments_reference as mr
import ptcommon as pc
from mi3pt_host import scenes


def _run_means(values, acc_frames, enabled=1, shape=(2, 3)):
    """scalar radiance values, one per step, through the reference's mean (mix(prev, c, 1 / frame)) in fp32 -> welford's arguments"""
    frames, before, after = [], [], []
    mean = np.zeros(shape + (4,), np.float32)
    en = list(enabled) if np.ndim(enabled) else [enabled] * len(values)
    for v, f, e in zip(values, acc_frames, en):
        c = np.full(shape + (4,), v, np.float32)
        f32 = int(f) & 0xFFFFFFFF
        wgt = np.float32(1) if (f32 == 0 or e != 1) else np.float32(1) / np.float32(f32)
        new = mean * (np.float32(1) - wgt) + c * wgt
        frames.append(c); before.append(mean); after.append(new)
        mean = new
    return frames, before, after


def test_constant_sequence_has_no_spread():
    fr, b, a = _run_means([1.5] * 7, range(1, 8))
    m = mr.welford(fr, b, a, range(1, 8))
    assert np.all(m[..., :3] == 0) and np.all(m[..., 3] == 7)


def test_two_frames_zero_and_two():
    fr, b, a = _run_means([0.0, 2.0], [1, 2])
    m = mr.welford(fr, b, a, [1, 2])
    assert np.all(m[..., :3] == 2) and np.all(m[..., 3] == 2)          # (2 - 0) * (2 - 1); sample variance 2 / (2 - 1) = 2


@pytest.mark.parametrize("name,acc_frames,enabled,want_n", [
    ("frame 0", [1, 2, 0], 1, 1), ("frame 1", [1, 2, 3, 1], 1, 1), ("restart and go on", [1, 2, 3, 1, 2], 1, 2),
    ("enabled 0", [1, 2, 3], [1, 1, 0], 1), ("enabled 2", [1, 2, 3], [1, 1, 2], 1),
    ("wrap through 2^32", [0xFFFFFFFE, 0xFFFFFFFF, 0x100000000, 0x100000001, 0x100000002], 1, 2),
    ("no restart", [5, 6, 7], 1, 3)])
def test_every_restart_condition(name, acc_frames, enabled, want_n):
    values = [0.25 * (k + 1) * (-1) ** k for k in range(len(acc_frames))]
    fr, b, a = _run_means(values, acc_frames, enabled)
    start = np.full((2, 3, 4), 3.0, np.float32)                         # (sums from before: a restart forgets them)
    m = mr.welford(fr, b, a, acc_frames, enabled, moments=start)
    assert np.all(m[..., 3] == (want_n if name != "no restart" else 3 + 3)), name
    if want_n == 1:
        assert np.all(m[..., :3] == 0), name
    else:
        assert np.all(m[..., :3] > 0), name


def test_texels_outside_the_rectangle_are_untouched():
    fr, b, a = _run_means([0.0, 2.0, 5.0], [1, 2, 3], shape=(4, 5))
    inside = np.zeros((4, 5), bool)
    inside[:3, :2] = True
    start = np.random.default_rng(1).random((4, 5, 4), dtype=np.float32)
    m = mr.welford(fr, b, a, [1, 2, 3], moments=start, inside=inside)
    assert np.array_equal(m[~inside], start[~inside])
    assert np.all(m[inside][:, 3] == 3)


def test_variance_of_the_mean_edge_cases():
    m = np.zeros((1, 6, 4), np.float32)
    m[0, 0] = (5, 5, 5, 1)                       # n < 2
    m[0, 1] = (5, 5, 5, 0)
    m[0, 2] = (-1, -2, -3, 4)                    # a negative sum
    m[0, 3] = (np.nan, 1, 1, 4)                  # NaN
    m[0, 4] = (1, 2, 3, 4)                       # 6 / 12
    m[0, 5] = (1, 2, 3, 1.5)                     # 1 <= n < 2
    v = mr.variance_of_mean(m)
    assert v.dtype == np.float32
    assert v.tolist() == [[0.0, 0.0, 0.0, 0.0, 0.5, 0.0]]


# Measured: the largest relative gap between M2 / (n - 1) and the two-pass float64 sample variance of the same eight oracle frames, over
# the texels (x channels) whose variance is above the median: 1.33e-06 (11 ulp of fp32 after eight frames -- Welford's update does not
# cancel).  The bound is 16 x that: room for another libm or numpy summation order, nothing else.
WELFORD_GAP_MEASURED = 1.33e-06


def test_welford_against_the_two_pass_float64_variance(orc, demo, env):
    w = h = 64
    osc = pc.oracle_scene(orc, demo, env)
    steps = [(f, f, 1) for f in range(1, 9)]
    _, m, frames, _ = mr.oracle_steps(orc, osc, steps, w, h, lambda f: pc.rt_uniforms(demo, w, h, frame=f, bounces=4).tobytes(),
                                      lambda f, e: pc.acc_uniforms(w, h, f, e).tobytes())
    assert np.all(m[..., 3] == 8)
    stack = np.stack([np.asarray(f, np.float64)[..., :3] for f in frames])
    two_pass = stack.var(axis=0, ddof=1)
    got = m[..., :3].astype(np.float64) / 7.0
    sel = two_pass > np.median(two_pass)
    gap = float((np.abs(got - two_pass)[sel] / two_pass[sel]).max())
    print(f"largest relative gap of M2 / (n - 1) to the float64 two-pass variance above the median: {gap:.3g}")
    assert gap <= 16 * WELFORD_GAP_MEASURED


def _tone_rmse(x, truth):
    a = np.asarray(x, np.float64)[..., :3]
    b = np.asarray(truth, np.float64)[..., :3]
    return float(np.sqrt(np.mean((a / (1 + a) - b / (1 + b)) ** 2)))


def test_variance_guided_filter_wins_from_sixteen_frames_on(orc, demo):
    """The setting of test_guided_reference.py::test_guided_filter_beats_the_bilateral_at_low_sample_counts: the demo scene at 96 x 96
    under the sun-less sky, four bounces, RMSE of x / (1 + x) against the mean of frames 1000 .. 3999.  At 16 and 64 frames in the mean:
    variance-guided (3 levels, sigma_color 2, the other sigmas default) < guided with today's defaults (3 levels, sigma_color =
    2 / sqrt(frames)) and < un-filtered.  No number is fixed; the errors are printed (2 and 4 frames too, where nothing is asserted:
    a variance from so few samples is itself noise)."""
    w = h = 96
    env = scenes.synthetic_env(sun_radiance=0.0)
    osc = pc.oracle_scene(orc, demo, env)
    feat = ar.reference(orc, osc, pc.rt_uniforms(demo, w, h).tobytes(), w, h)
    truth = np.zeros((h, w, 4), np.float64)
    for f in range(1000, 4000):
        truth += orc.raytrace(osc, pc.rt_uniforms(demo, w, h, frame=f, bounces=4).tobytes(), w, h)[0]
    truth /= 3000
    mean = np.zeros((h, w, 4), np.float32)
    moments = None
    for k in range(64):
        img, _ = orc.raytrace(osc, pc.rt_uniforms(demo, w, h, frame=2 + k, bounces=4).tobytes(), w, h)
        new = orc.accumulate(pc.acc_uniforms(w, h, 1 + k).tobytes(), w, h, img, mean)
        moments = mr.welford([img], [mean], [new], [1 + k], moments=moments)
        mean = new
        frames = k + 1
        if frames not in (2, 4, 16, 64):
            continue
        guided, _ = gr.guided(orc, mean, feat["normal"], feat["position"], feat["albedo"], feat["ids"],
                              levels=3, sigma_color=2.0 / np.sqrt(frames), sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.05)
        by_var, _, _ = mr.guided_variance(orc, mean, moments, feat["normal"], feat["position"], feat["albedo"], feat["ids"],
                                          levels=3, sigma_color=2.0, sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.05)
        e_raw, e_gui, e_var = _tone_rmse(mean, truth), _tone_rmse(guided, truth), _tone_rmse(by_var, truth)
        print(f"{frames} frames: un-filtered {e_raw:.4f}  guided {e_gui:.4f}  variance-guided {e_var:.4f}")
        if frames >= 16:
            assert e_var < e_gui and e_var < e_raw, frames
