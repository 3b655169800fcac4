#!/usr/bin/env python3
"""Times the per-tile error estimate of the running mean (mi3pt_estimate_convergence) and what sampling until converged costs beside a
fixed frame count.  1920 x 1080, the 870 k-triangle scene and view of bench.py; one process, five rounds, the sides alternating inside
every round; medians and min - max.
  a. MI3PT_PASS_CONVERGENCE (the tile kernel and the kernel that folds the summary) beside MI3PT_PASS_ACCUMULATE of the 16-frame batched mean it
     follows, timing on;
  b. the wall time of Renderer.renderUntil -- 64 frames, a check every 16, a threshold of 0 so that no check ends the run -- with lookahead
     on and off, against one mi3pt_submit_frames of the same 64 frames followed by mi3pt_sync and against the same four launches without
     the estimates, timing off.
usage: python profiles/convergence.py [WxH] [--out FILE]   (needs a GPU; prints its lines, and appends them to FILE when one is given)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "webgpu-pathtracer_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import ptcommon as pc  # noqa: E402
from mi3pt_host import RaytracingCamera, RaytracingScene, Renderer, capi, scenes  # noqa: E402

args = [a for a in sys.argv[1:]]
out_path = None
if "--out" in args:
    k = args.index("--out")
    out_path = args[k + 1]
    del args[k:k + 2]
w, h = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
frames, total, bounces = 16, 64, 8
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
        say(f"  {name:46s} median {np.median(t):9.1f} {unit}   min - max {min(t):9.1f} - {max(t):9.1f} {unit}")
    return {name: float(np.median(t)) for name, t in times.items()}


sc = scenes.dragon_class_scene()
sc.build_bvh()
env = scenes.synthetic_env()
say(f"{w} x {h}, {len(sc.triangles)} triangles, {bounces} bounces; five rounds, sides alternating")

# ---- a. device time of the estimate beside the ordered mean of the launch it follows ----
ctx = capi.Context(0)
pc.upload_scene(ctx, sc, env)
ctx.enable_timing(True)
ctx.set_moments(True)
ctx.resize(w, h)


def passes(which):
    ctx.reset()
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=1, bounces=bounces).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1).tobytes())
    ctx.submit_frames(MASK, frames)
    ctx.estimate_convergence(0.01, 16)
    ctx.sync()
    return ctx.pass_time_us(which)


a = report(f"a. device time (HIP events) after one launch of {frames} frames",
           [("MI3PT_PASS_ACCUMULATE (the ordered mean, moments on)", capi.PASS_ACCUMULATE),
            ("MI3PT_PASS_CONVERGENCE (tile kernel + summary kernel)", capi.PASS_CONVERGENCE)], passes)
traffic = w * h * 32 + ((w + 7) // 8) * ((h + 7) // 8) * 16
t_conv = a["MI3PT_PASS_CONVERGENCE (tile kernel + summary kernel)"]
say(f"  traffic {traffic / 1e6:.1f} MB: {traffic / t_conv / 1e6:.2f} TB/s; the floor at 6.3 TB/s is {traffic / 6.3e6:.1f} us")
s = ctx.read_convergence()
say(f"  the estimate after {frames} frames, threshold 0.01: {s}")
ctx.close()

# ---- b. wall time of sampling until converged beside a fixed count ----
r = Renderer.create()
r.scalingFactor = 1
r.presentEveryFrame = False
r.setUniforms("raytrace", {"maxBounces": bounces, "envMapIntensity": 1.0})
r.setUniforms("accumulate", {"enabled": 1})
r.setMoments(True)
r.resize(w, h)
scene = RaytracingScene(sc, env)
scene.needsUpdate = True
cam = RaytracingCamera(sc.camera["fov"], position=sc.camera["position"], target=sc.camera["target"])
cam.focalDistance, cam.aperture = sc.camera["focalDistance"], sc.camera["aperture"]
r.update(scene, cam)              # the scene upload, outside the timed part
r.ctx.sync()


def wall(how):
    r.frames = total
    r.reset()
    r.ctx.sync()
    t0 = time.perf_counter()
    if how == "fixed":
        r.ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2, bounces=bounces).tobytes())
        r.ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
        r.ctx.submit_frames(MASK, total)
        r.ctx.sync()
    elif how == "chunks":        # renderUntil's launches without its estimates
        for k in range(total // frames):
            r.ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2 + k * frames, bounces=bounces).tobytes())
            r.ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2 + k * frames).tobytes())
            r.ctx.submit_frames(MASK, frames)
            r.ctx.flush()
        r.ctx.sync()
    else:
        out = r.renderUntil(scene, cam, 0.0, minFrames=16, maxFrames=total, checkEvery=frames, lookahead=how == "lookahead")
        r.ctx.sync()
        assert out["frames"] == total and not out["converged"]
    return (time.perf_counter() - t0) * 1e3


b = report(f"b. wall time of {total} frames, a check every {frames} (threshold 0: every check says \"above\")",
           [("mi3pt_submit_frames(64) + mi3pt_sync", "fixed"), ("4 x (mi3pt_submit_frames(16) + mi3pt_flush) + sync", "chunks"),
            ("renderUntil, lookahead on", "lookahead"),
            ("renderUntil, lookahead off", "immediate")], wall, unit="ms")
fixed = b["mi3pt_submit_frames(64) + mi3pt_sync"]
say(f"  lookahead on / fixed = {b['renderUntil, lookahead on'] / fixed:.3f}; lookahead off / fixed = {b['renderUntil, lookahead off'] / fixed:.3f}")
r.destroy()
if out_path:
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
