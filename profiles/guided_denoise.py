#!/usr/bin/env python3
"""Times the feature-guided a-trous de-noise (mi3pt_denoise_guided) beside the fullscreen pass's 85-tap bilateral de-noiser.
1920 x 1080, the 870 k-triangle scene and view of bench.py, a mean of four frames, timing on; five rounds, the sides alternating
inside every round; medians and min - max.
usage: python profiles/guided_denoise.py [WxH]   (needs a GPU)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "webgpu-pathtracer_amd", "py"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import ptcommon as pc  # noqa: E402
from mi3pt_host import capi, scenes  # noqa: E402

w, h = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1920x1080").split("x"))
frames = 4
sc = scenes.dragon_class_scene()
sc.build_bvh()
ctx = capi.Context(0)
pc.upload_scene(ctx, sc, scenes.synthetic_env())
ctx.enable_timing(True)
ctx.resize(w, h)
for f in range(1, frames + 1):
    pc.gpu_frame(ctx, pc.rt_uniforms(sc, w, h, frame=f, bounces=8), pc.acc_uniforms(w, h, f), 3)
ctx.render_aovs(capi.AOV_ALL)
ctx.sync()
sigma_color = 2.0 / np.sqrt(frames)
sides = [("guided 1 level", 1), ("guided 3 levels", 3), ("guided 5 levels", 5), ("fullscreen denoise 1 (85-tap bilateral)", 0),
         ("fullscreen denoise 0", -1)]
times = {name: [] for name, _ in sides}


def one(levels):
    if levels > 0:
        ctx.denoise_guided(levels, sigma_color)
        ctx.sync()
        return ctx.pass_time_us(capi.PASS_GUIDED)
    ctx.set_uniforms(capi.PASS_FULLSCREEN, pc.fs_uniforms(w, h, 1.0, 1 if levels == 0 else 0, 1).tobytes())
    ctx.submit(capi.SUBMIT_FULLSCREEN)
    ctx.sync()
    return ctx.pass_time_us(capi.PASS_FULLSCREEN)


for name, levels in sides:          # warm-up: code objects, the bilateral's tap table, the filter's images
    one(levels)
for _ in range(5):
    for name, levels in sides:
        times[name].append(one(levels))
texels = w * h
print(f"{w} x {h}, {len(sc.triangles)} triangles, mean of {frames} frames, sigma_color {sigma_color:.3f}; device time (HIP events), five rounds, sides alternating")
for name, _ in sides:
    t = times[name]
    print(f"  {name:42s} median {np.median(t):8.1f} us   min - max {min(t):8.1f} - {max(t):8.1f} us")
per_level = (np.median(times["guided 5 levels"]) - np.median(times["guided 1 level"])) / 4.0
# per texel and level: colour 16 B + three 16-byte feature records read, 16 B written (the 20 x 20 halo re-reads stay in L2)
floor_us = texels * 80 / 8.0e12 * 1e6
print(f"  per level (5 levels - 1 level) / 4: {per_level:.1f} us; traffic floor {texels} texels x 80 B / 8 TB/s = {floor_us:.1f} us per level")
