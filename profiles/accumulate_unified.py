#!/usr/bin/env python3
"""Times the accumulate pass at its two call sites, for a comparison of two builds of the library (MI3PT_LIBRARY names the one to load).
1920 x 1080, the demo scene, timing on, moments off and on:
  a. MI3PT_PASS_ACCUMULATE of a single-frame accumulate submitted on its own (the call site of mi3pt_submit: at most 2048 blocks);
  b. MI3PT_PASS_ACCUMULATE of the last run of a 16-frame submit_frames (the batched call site: at most 4096 blocks).
Ten samples each after a warm-up; median, min - max and spread (max - min).
usage: python profiles/accumulate_unified.py LABEL [--out FILE]   (needs a GPU; prints its lines, and appends them to FILE when one is given)
profiles/accumulate_unified.log is put together by hand from this script's lines on both builds, the kernels' resource usage and bench.py's
headline on both builds."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "webgpu-pathtracer_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import ptcommon as pc  # noqa: E402
from mi3pt_host import capi, scenes  # noqa: E402

args = sys.argv[1:]
out_path = None
if "--out" in args:
    k = args.index("--out")
    out_path = args[k + 1]
    del args[k:k + 2]
label = args[0] if args else "library"
w, h, frames, samples = 1920, 1080, 16, 10
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


sc = scenes.demo_scene()
sc.build_bvh()
ctx = capi.Context(0)
pc.upload_scene(ctx, sc, scenes.synthetic_env())
ctx.enable_timing(True)
ctx.resize(w, h)
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE


def uniforms(frame):
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=frame, bounces=4).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, frame).tobytes())


def single(frame):
    uniforms(frame)
    ctx.submit(capi.SUBMIT_RAYTRACE)
    ctx.submit(capi.SUBMIT_ACCUMULATE)
    ctx.sync()
    return ctx.pass_time_us(capi.PASS_ACCUMULATE)


def batch(frame):
    uniforms(frame)
    ctx.submit_frames(MASK, frames)
    ctx.sync()
    return ctx.pass_time_us(capi.PASS_ACCUMULATE)


say(f"{label}: {w} x {h}, demo scene; MI3PT_PASS_ACCUMULATE, device time (HIP events), {samples} samples after 2 warm-up calls")
for moments in (False, True):
    ctx.set_moments(moments)
    for name, fn, step in (("a. single frame", single, 1), (f"b. last run of {frames} frames", batch, frames)):
        ctx.reset()
        t = [fn(2 + k * step) for k in range(samples + 2)][2:]
        say(f"  {name:26s} moments {'on ' if moments else 'off'}  median {np.median(t):7.1f} us   min - max {min(t):7.1f} - {max(t):7.1f}   spread {max(t) - min(t):6.1f} us")
ctx.close()
if out_path:
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
