#!/usr/bin/env python3
"""Times what the moments image and the variance-guided filter cost.  1920 x 1080, the 870 k-triangle scene and view of bench.py,
timing on; one process, five rounds, the sides alternating inside every round; medians and min - max.
  a. MI3PT_PASS_ACCUMULATE of a 16-frame batched mean (one submit_frames, one launch, one ordered mean) with moments off and on;
  b. MI3PT_PASS_GUIDED at 3 levels without and with MI3PT_GUIDED_VARIANCE (the latter includes the variance kernel).
usage: python profiles/moments.py [WxH] [--out FILE]   (needs a GPU; prints its lines, and appends them to FILE when one is given)
profiles/moments.log is put together by hand: the resource-usage diffs against the parent commit, this script's lines as its section 3, and
bench.py's headline on both commits.  A rerun does not touch it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "webgpu-pathtracer_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import ptcommon as pc  # noqa: E402
from mi3pt_host import capi, scenes  # noqa: E402

args = [a for a in sys.argv[1:]]
out_path = None
if "--out" in args:
    k = args.index("--out")
    out_path = args[k + 1]
    del args[k:k + 2]
w, h = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
frames = 16
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


sc = scenes.dragon_class_scene()
sc.build_bvh()
ctx = capi.Context(0)
pc.upload_scene(ctx, sc, scenes.synthetic_env())
ctx.enable_timing(True)
ctx.resize(w, h)
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE


def mean_of_16(moments):
    ctx.set_moments(moments)
    ctx.reset()
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=1, bounces=8).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1).tobytes())
    ctx.submit_frames(MASK, frames)
    ctx.sync()
    return ctx.pass_time_us(capi.PASS_ACCUMULATE)


def guided(flag):
    ctx.denoise_guided(3, 2.0 if flag else 2.0 / np.sqrt(frames), flags=capi.GUIDED_VARIANCE if flag else 0)
    ctx.sync()
    return ctx.pass_time_us(capi.PASS_GUIDED)


def report(title, sides, fn):
    times = {name: [] for name, _ in sides}
    for _, arg in sides:          # warm-up: code objects, the images
        fn(arg)
    for _ in range(5):
        for name, arg in sides:
            times[name].append(fn(arg))
    say(title)
    for name, _ in sides:
        t = times[name]
        say(f"  {name:42s} median {np.median(t):8.1f} us   min - max {min(t):8.1f} - {max(t):8.1f} us")
    return {name: float(np.median(t)) for name, t in times.items()}


texels = w * h
say(f"{w} x {h}, {len(sc.triangles)} triangles; device time (HIP events), five rounds, sides alternating")
a = report(f"a. MI3PT_PASS_ACCUMULATE, the ordered mean of {frames} frames in one launch",
           [("moments off", False), ("moments on", True)], mean_of_16)
# traffic: 16 radiance slots read + the mean read and written -- with moments: + the moments image read and written
off_b, on_b = texels * 16 * (frames + 2), texels * 16 * (frames + 4)
say(f"  on / off = {a['moments on'] / a['moments off']:.3f}; traffic {on_b / 1e6:.0f} MB / {off_b / 1e6:.0f} MB = {on_b / off_b:.3f}")
mean_of_16(True)                  # the mean and the moments the filter reads
ctx.render_aovs(capi.AOV_ALL)
ctx.sync()
b = report("b. MI3PT_PASS_GUIDED, 3 levels", [("without the flag (sigma_color 2 / sqrt(16))", False),
                                             ("MI3PT_GUIDED_VARIANCE (sigma_color 2)", True)], guided)
say(f"  with / without = {b['MI3PT_GUIDED_VARIANCE (sigma_color 2)'] / b['without the flag (sigma_color 2 / sqrt(16))']:.3f}")
ctx.close()
if out_path:
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
