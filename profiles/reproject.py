#!/usr/bin/env python3
"""Times the reprojection of the running mean (mi3pt_reproject) and the mean by count (mi3pt_set_mean_by_count).  1920 x 1080, the
870 k-triangle scene and view of bench.py; one process, five rounds, the sides alternating inside every round; medians and min - max.
  a. MI3PT_PASS_REPROJECT (the gather kernel) and MI3PT_PASS_AOV (the feature render inside the call) of one mi3pt_reproject after a
     camera orbit of 2 degrees, 16 frames in the mean, timing on; the kernel's traffic beside the estimate of 9 images x 16 B per texel;
  b. MI3PT_PASS_ACCUMULATE of a 16-frame launch with the moments twin (<true>: unchanged by the mode) and with the by-count twin
     (<true, true>), timing on.
usage: python profiles/reproject.py [WxH] [--out FILE]   (needs a GPU; prints its lines, and appends them to FILE when one is given)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "webgpu-pathtracer_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
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
w, h = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
frames, bounces = 16, 8
lines = []
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE


def say(text):
    print(text, flush=True)
    lines.append(text)


def report(title, sides, fn, unit="us"):
    times = {name: [] for name, _ in sides}
    for _, arg in sides:          # warm-up: code objects, the images
        fn(arg)
    for _ in range(5):
        for name, arg in sides:
            times[name].append(fn(arg))
    say(title)
    for name, _ in sides:
        t = times[name]
        say(f"  {name:58s} median {np.median(t):9.1f} {unit}   min - max {min(t):9.1f} - {max(t):9.1f} {unit}")
    return {name: float(np.median(t)) for name, t in times.items()}


sc = scenes.dragon_class_scene()
sc.build_bvh()
env = scenes.synthetic_env()
say(f"{w} x {h}, {len(sc.triangles)} triangles, {bounces} bounces; five rounds, sides alternating")
view_b = rr.orbit(sc.camera["position"], sc.camera["target"], 2.0)
ctx = capi.Context(0)
pc.upload_scene(ctx, sc, env)
ctx.enable_timing(True)
ctx.set_moments(True)
ctx.resize(w, h)


def sample(by_count):
    ctx.set_mean_by_count(by_count)
    ctx.reset()
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2, bounces=bounces).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1).tobytes())
    ctx.submit_frames(MASK, frames)
    ctx.flush()


def reproject(which):
    sample(True)
    ctx.render_aovs(capi.AOV_ALL)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2 + frames, bounces=bounces, position=view_b[0], direction=view_b[1]).tobytes())
    ctx.reproject()
    ctx.sync()
    return ctx.pass_time_us(which)


a = report(f"a. device time (HIP events) of one mi3pt_reproject, {frames} frames in the mean, the camera orbits by 2 degrees",
           [("MI3PT_PASS_REPROJECT (the gather kernel)", capi.PASS_REPROJECT),
            ("MI3PT_PASS_AOV (the four feature images of the new view)", capi.PASS_AOV)], reproject)
traffic = w * h * 16 * 9
t = a["MI3PT_PASS_REPROJECT (the gather kernel)"]
say(f"  traffic estimate, 7 images read and 2 written: {traffic / 1e6:.1f} MB: {traffic / t / 1e6:.2f} TB/s; the floor at 6.3 TB/s is {traffic / 6.3e6:.1f} us")
n = ctx.read_moments()[..., 3]
hit = ctx.read_aov(capi.AOV_IDS)[..., 2] == 1
say(f"  {int((n[hit] >= 1).sum())} of {int(hit.sum())} hit texels carried ({100.0 * (n[hit] >= 1).mean():.1f} %), {int((n[hit] < 1).sum())} restart")


def mean_pass(by_count):
    sample(by_count)
    ctx.sync()
    return ctx.pass_time_us(capi.PASS_ACCUMULATE)


b = report(f"b. MI3PT_PASS_ACCUMULATE of one launch of {frames} frames",
           [("k_accumulate_frames<true> (moments, the default law)", False),
            ("k_accumulate_frames<true, true> (the mean by count)", True)], mean_pass)
say(f"  by count / default = {b['k_accumulate_frames<true, true> (the mean by count)'] / b['k_accumulate_frames<true> (moments, the default law)']:.3f}")
ctx.close()
if out_path:
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
