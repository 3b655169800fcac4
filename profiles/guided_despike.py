#!/usr/bin/env python3
"""Measures the firefly pre-pass of the guided de-noise (mi3pt_set_guided_despike; csrc/pt_guided.hip: k_guided_despike),
profiles/guided_young.py's method.
  a. (needs a GPU) 1920 x 1080, the 870 k-triangle scene and view of bench.py with the sun, the mean by count, the moments image and
     timing on, 16 frames; one process, both sides warmed up, then five rounds with the two sides alternating inside every round;
     medians and min - max of MI3PT_PASS_GUIDED at three levels with the state on against the state off -- this commit's own off
     path -- in the three modes, and the share of clamped texels.  Every mode runs under its own time limit (SIGALRM ends the
     process: a hung step starts nothing more).
  b. (--cpu: the oracle's renderer, no GPU) the table of DESIGN.md section 3: the demo scene at 96 x 64, four bounces, the
     environment with its sun (yardstick: a 3 000-frame mean) and the sun-less sky (1 024 frames), the mean by count of 1, 4, 16 and
     64 frames, three levels; tone-mapped RMSE x / (1 + x) over every texel, un-filtered and in the three modes -- fixed sigma
     (sigma_color 2 / sqrt(frames)), variance, variance + young (sigma_color 2) -- each without and with the pre-pass.
usage: python profiles/guided_despike.py [WxH] [--cpu] [--out FILE]   (prints its lines, and appends them to FILE when one is given)"""
import math
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "webgpu-pathtracer_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import ptcommon as pc  # noqa: E402
from mi3pt_host import capi, scenes  # noqa: E402

args = [a for a in sys.argv[1:]]
out_path = None
if "--out" in args:
    k = args.index("--out")
    out_path = args[k + 1]
    del args[k:k + 2]
cpu = "--cpu" in args
args = [a for a in args if a != "--cpu"]
lines = []
SIGMAS = (2.0, 0.35, 0.1, 0.05)
LEVELS = 3


def say(text):
    print(text, flush=True)
    lines.append(text)


def finish():
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


def on_the_cpu():
    import aov_reference as ar
    import guided_despike_reference as dr
    import guided_reference as gr
    import guided_young_reference as yr
    import moments_reference as mr
    import pt_oracle as orc
    import reproject_reference as rr
    F = np.float32
    demo = scenes.demo_scene()
    demo.build_bvh()
    w, h = 96, 64
    un = lambda f: pc.rt_uniforms(demo, w, h, frame=f, bounces=4).tobytes()

    def rmse(x, truth):
        a, b = np.asarray(x, np.float64)[..., :3], truth[..., :3]
        return float(np.sqrt((((a / (1 + a)) - (b / (1 + b))) ** 2).mean()))

    say(f"b. the oracle's renderer, demo scene {w} x {h}, four bounces; {LEVELS} levels, sigma {SIGMAS}, fixed mode sigma_color 2 / sqrt(N); "
        f"tone-mapped RMSE over every texel; 'pre' = behind the pre-pass")
    for name, env, yard in (("the environment with its sun", scenes.synthetic_env(), 3000), ("the sun-less sky", scenes.synthetic_env(sun_radiance=0.0), 1024)):
        osc = pc.oracle_scene(orc, demo, env)
        truth = np.zeros((h, w, 4))
        for f in range(1000, 1000 + yard):
            truth += orc.raytrace(osc, un(f), w, h)[0]
        truth /= yard
        feat = ar.reference(orc, osc, un(0), w, h)
        feats = (feat["normal"], feat["position"], feat["albedo"], feat["ids"])
        say(f"  {name}, against {yard} frames:")
        say("    N   raw      fixed    pre      ratio   variance pre      ratio   var+young pre     ratio   clamped   m == 0")
        a, m = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
        for n in range(1, 65):
            a, m = rr.by_count_step(a, m, orc.raytrace(osc, un(1 + n), w, h)[0])
            if n not in (1, 4, 16, 64):
                continue
            sc = SIGMAS[0] / math.sqrt(n)
            fixed = rmse(gr.guided(orc, a, *feats, LEVELS, sc, *SIGMAS[1:])[0], truth)
            out, _, _, st = dr.guided(orc, a, *feats, LEVELS, sc, *SIGMAS[1:])
            fixed_pre = rmse(out, truth)
            var = rmse(mr.guided_variance(orc, a, m, *feats, LEVELS, *SIGMAS)[0], truth)
            var_pre = rmse(dr.guided_variance(orc, a, m, *feats, LEVELS, *SIGMAS)[0], truth)
            young = rmse(yr.guided_variance_young(orc, a, m, *feats, LEVELS, *SIGMAS)[0], truth)
            young_pre = rmse(dr.guided_variance(orc, a, m, *feats, LEVELS, *SIGMAS, young=True)[0], truth)
            say(f"   {n:2d}   {rmse(a, truth):.4f}   {fixed:.4f}   {fixed_pre:.4f}   {fixed_pre / fixed:.3f}   {var:.4f}   {var_pre:.4f}   {var_pre / var:.3f}   "
                f"{young:.4f}    {young_pre:.4f}  {young_pre / young:.3f}   {100 * st['clamped']:5.2f} %   {100 * st['lone']:.2f} %")


if cpu:
    on_the_cpu()
    finish()
    sys.exit(0)

w, h = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
frames, bounces = 16, 8
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
MODES = (("fixed sigma", 0, SIGMAS[0] / math.sqrt(frames)), ("MI3PT_GUIDED_VARIANCE", capi.GUIDED_VARIANCE, SIGMAS[0]),
         ("MI3PT_GUIDED_VARIANCE | MI3PT_GUIDED_YOUNG", capi.GUIDED_VARIANCE | capi.GUIDED_YOUNG, SIGMAS[0]))
signal.alarm(300)          # the scene, the tree, the context, the frames
sc = scenes.dragon_class_scene()
sc.build_bvh()
env = scenes.synthetic_env()
say(f"a. {w} x {h}, {len(sc.triangles)} triangles, {bounces} bounces, the sun on, {frames} frames by count; {LEVELS} levels, sigma {SIGMAS}; "
    f"HIP events of one call, MI3PT_PASS_GUIDED; five rounds, sides alternating")
ctx = capi.Context(0)
pc.upload_scene(ctx, sc, env)
ctx.enable_timing(True)
ctx.set_moments(True)
ctx.set_mean_by_count(True)
ctx.resize(w, h)
ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2, bounces=bounces).tobytes())
ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1).tobytes())
ctx.submit_frames(MASK, frames)
ctx.flush()
ctx.render_aovs(capi.AOV_ALL)


def timed(on, flags, sigma_color):
    ctx.set_guided_despike(on)
    ctx.denoise_guided(LEVELS, sigma_color, *SIGMAS[1:], flags=flags)
    ctx.sync()
    return ctx.pass_time_us(capi.PASS_GUIDED)


for name, flags, sigma_color in MODES:
    signal.alarm(240)      # this mode's own time limit
    image = {}
    for on in (False, True):          # warm-up: code objects, the images
        timed(on, flags, sigma_color)
        image[on] = ctx.read_guided()
    clamped = ctx.read_guided_despiked()
    times = {False: [], True: []}
    for _ in range(5):
        for on in (False, True):
            times[on].append(timed(on, flags, sigma_color))
    a, b = times[False], times[True]
    say(f"  {name}: {clamped} of {w * h} texels clamped ({100.0 * clamped / (w * h):.2f} %); the filtered image "
        f"{'has the same bits' if image[False].tobytes() == image[True].tobytes() else 'differs'} with the state on")
    say(f"    state off  median {np.median(a):7.1f} us   min - max {min(a):7.1f} - {max(a):7.1f} us")
    say(f"    state on   median {np.median(b):7.1f} us   min - max {min(b):7.1f} - {max(b):7.1f} us   difference of the medians {np.median(b) - np.median(a):+.1f} us")
signal.alarm(0)
ctx.set_guided_despike(False)
ctx.close()
finish()
