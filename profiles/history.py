#!/usr/bin/env python3
"""Measures the held history (mi3pt_hold_history, mi3pt_merge_history), profiles/reproject_scene.py's method.
  a. (needs a GPU) 1920 x 1080, the 870 k-triangle scene and view of bench.py, 16 frames in the mean, timing on; one process, five
     rounds, the sides alternating inside every round; medians and min - max of
       MI3PT_PASS_REPROJECT   k_reproject after a camera orbit of 2 degrees: the yardstick for "a pass over four images"
       MI3PT_PASS_HISTORY     k_history, radius 0 .. 3, merging that reprojection's result (held) into 4 fresh frames of the new view
     with the share of carried samples kept.
  b. (--cpu: the oracle's renderer, no GPU) the table of DESIGN.md section 3 -- tests/history_cases.py: the demo scene at 48 x 32, four
     bounces, the sun-less sky, 64 frames, a change under a fixed camera, mi3pt_reproject_scene's reference, K fresh frames, radius 1 / 2 / 3;
     yardstick: a 1 024-frame mean of the new scene, tone-mapped RMSE over its hit texels.
usage: python profiles/history.py [WxH] [--cpu] [--out FILE]   (prints its lines, and appends them to FILE when one is given)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "webgpu-pathtracer_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import ptcommon as pc  # noqa: E402
import reproject_reference as rr  # noqa: E402
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


def say(text):
    print(text, flush=True)
    lines.append(text)


def finish():
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


def on_the_cpu():
    import history_cases as hc
    import pt_oracle as orc
    demo = scenes.demo_scene()
    demo.build_bvh()
    use = hc.UseCase(orc, demo)
    say(f"b. the oracle's renderer, demo scene {hc.W} x {hc.H}, four bounces, sun-less sky, a fixed camera; {hc.HISTORY_FRAMES} frames, the change, "
        f"mi3pt_reproject_scene's defaults, K fresh frames; tone-mapped RMSE over the hit texels against {hc.TRUTH_FRAMES} frames; z 2 / 4")
    say("  change   K  radius   fresh alone   merged at once   held, validated, merged   share of carried samples kept")
    for change in hc.CHANGES:
        for frames in (4, 16):
            for radius in (1, 2, 3):
                row = use.measure(change, frames, radius)
                say(f"  {change:8s} {frames:2d}  {radius}        {row['alone']:.4f}        {row['at_once']:.4f}           {row['validated']:.4f}"
                    f"                    {row['kept']:.3f}")


if cpu:
    on_the_cpu()
    finish()
    sys.exit(0)

w, h = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
frames, fresh, bounces = 16, 4, 8
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
sc = scenes.dragon_class_scene()
sc.build_bvh()
env = scenes.synthetic_env()
say(f"{w} x {h}, {len(sc.triangles)} triangles, {bounces} bounces; five rounds, sides alternating")
view_b = rr.orbit(sc.camera["position"], sc.camera["target"], 2.0)
ctx = capi.Context(0)
pc.upload_scene(ctx, sc, env)
ctx.enable_timing(True)
ctx.set_moments(True)
ctx.set_mean_by_count(True)
ctx.resize(w, h)
kept = {}


def one(radius):
    """16 frames, the orbit, mi3pt_reproject, hold, 4 frames of the new view, merge at `radius`: (reproject us, history us)"""
    ctx.reset()
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2, bounces=bounces).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1).tobytes())
    ctx.submit_frames(MASK, frames)
    ctx.flush()
    ctx.render_aovs(capi.AOV_ALL)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2 + frames, bounces=bounces, position=view_b[0], direction=view_b[1]).tobytes())
    ctx.reproject()
    ctx.sync()
    t_reproject = ctx.pass_time_us(capi.PASS_REPROJECT)
    held = float(ctx.read_moments()[..., 3].astype(np.float64).sum())
    ctx.hold_history()
    ctx.submit_frames(MASK, fresh)
    ctx.flush()
    ctx.merge_history(radius=radius)
    ctx.sync()
    t_history = ctx.pass_time_us(capi.PASS_HISTORY)
    n = ctx.read_moments()[..., 3].astype(np.float64)
    kept[radius] = (float((n - fresh).sum()) / held, held)
    return t_reproject, t_history


radii = (0, 1, 2, 3)
times = {r: [] for r in radii}
reproject = []
for r in radii:          # warm-up: code objects, the images
    one(r)
for _ in range(5):
    for r in radii:
        a, b = one(r)
        reproject.append(a)
        times[r].append(b)
say(f"a. HIP events of one call, {frames} frames in the held mean, {fresh} fresh frames")
say(f"  MI3PT_PASS_REPROJECT  k_reproject: a 2 degree orbit   median {np.median(reproject):7.1f} us   min - max {min(reproject):7.1f} - {max(reproject):7.1f} us   ({len(reproject)} calls)")
for r in radii:
    t = times[r]
    say(f"  MI3PT_PASS_HISTORY    k_history<{r}>: a {2 * r + 1} x {2 * r + 1} window      median {np.median(t):7.1f} us   min - max {min(t):7.1f} - {max(t):7.1f} us   "
        f"{100.0 * kept[r][0]:.1f} % of {kept[r][1]:.0f} carried samples kept")
ctx.close()
finish()
