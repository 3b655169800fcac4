#!/usr/bin/env python3
"""Measures the reprojection across a scene change (mi3pt_keep_geometry, mi3pt_reproject_scene), profiles/reproject.py's method.
  a. (needs a GPU) 1920 x 1080, the 870 k-triangle scene and view of bench.py, 16 frames in the mean, timing on; one process, five
     rounds, the sides alternating inside every round; medians and min - max of MI3PT_PASS_REPROJECT:
       k_reproject             mi3pt_reproject after a camera orbit of 2 degrees
       k_reproject_scene       the same orbit with the geometry kept and nothing uploaded (one buffer: no record is read twice)
       k_reproject_scene       the same orbit with the same records uploaded again (two buffers, every texel static)
       k_reproject_scene       a fixed camera, every triangle turned by 2 degrees about the vertical axis through the camera's target
     with the share of hit texels carried on every side.
  b. (--cpu: the oracle's renderer, no GPU) the demo scene at 48 x 32, four bounces, the sun-less sky: 64 frames, the box slides by 0.1
     along x under a fixed camera, then reprojected + 4 new frames against the same 4 frames alone; yardstick: a 1 024-frame mean of the
     new scene, tone-mapped RMSE over its hit texels -- all of them, and the box's alone.
usage: python profiles/reproject_scene.py [WxH] [--cpu] [--out FILE]   (prints its lines, and appends them to FILE when one is given)"""
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
F = np.float32


def say(text):
    print(text, flush=True)
    lines.append(text)


def finish():
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


def turned(sc, degrees, pivot):
    """every triangle of the scene turned about the vertical axis through `pivot`"""
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    p = np.asarray(pivot, np.float64)

    def turn(v, about):
        d = v - about
        return np.stack([c * d[..., 0] + s * d[..., 2], d[..., 1], -s * d[..., 0] + c * d[..., 2]], axis=-1) + about
    out = scenes.Scene(turn(np.asarray(sc.positions, np.float64), p), turn(np.asarray(sc.normals, np.float64), 0.0), sc.material_index, sc.materials)
    out.build_bvh()
    return out


def on_the_cpu():
    import aov_reference as ar
    import pt_oracle as orc
    import reproject_scene_cases as cases
    import reproject_scene_reference as rs
    w, h, slide = 48, 32, 0.1
    demo = scenes.demo_scene()
    demo.build_bvh()
    moved = cases.box_moved(demo, shift=(slide, 0.0, 0.0), degrees=0.0)
    sky = scenes.synthetic_env(sun_radiance=0.0)
    old_scene, new_scene = pc.oracle_scene(orc, demo, sky), pc.oracle_scene(orc, moved, sky)
    u = lambda frame: pc.rt_uniforms(demo, w, h, frame=frame, bounces=4)
    say(f"b. the oracle's renderer, demo scene {w} x {h}, four bounces, sun-less sky; 64 frames, the box slides by {slide} along x, a fixed camera")
    mean, moments = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    for k in range(64):
        mean, moments = rr.by_count_step(mean, moments, orc.raytrace(old_scene, u(2 + k).tobytes(), w, h)[0])
    truth = np.zeros((h, w, 4), np.float64)
    for f in range(1000, 2024):
        truth += orc.raytrace(new_scene, u(f).tobytes(), w, h)[0]
    truth /= 1024
    old = ar.reference(orc, old_scene, u(0).tobytes(), w, h)
    old["ids"] = cases.triangle_indices(orc, demo, u(0).tobytes(), old, w, h)
    new = ar.reference(orc, new_scene, u(0).tobytes(), w, h)
    new["ids"] = cases.triangle_indices(orc, moved, u(0).tobytes(), new, w, h)
    hit = new["hit"]
    tri = new["ids"][..., 0]
    box = hit & (tri >= cases.BOX.start) & (tri < cases.BOX.stop)
    new_frames = [orc.raytrace(new_scene, u(66 + k).tobytes(), w, h)[0] for k in range(4)]

    def rmse(x, sel):
        a, b = np.asarray(x, np.float64)[..., :3][sel], truth[..., :3][sel]
        return float(np.sqrt((((a / (1 + a)) - (b / (1 + b))) ** 2).mean()))

    def plus_frames(a, m):
        for c in new_frames:
            a, m = rr.by_count_step(a, m, c)
        return a
    alone = plus_frames(np.zeros((h, w, 4), F), np.zeros((h, w, 4), F))
    say(f"  4 frames alone: tone-mapped RMSE {rmse(alone, hit):.5f} over the {int(hit.sum())} hit texels, {rmse(alone, box):.5f} over the {int(box.sum())} box texels")
    f0 = rr.view_frame(u(0).tobytes())
    for history_moved in (1, 8, 64):
        a, m, info = rs.reproject_scene(mean, moments, f0, (F(w), F(h)), new, old, (w, h), moved.triangles, demo.triangles, max_history_moved=history_moved)
        a = plus_frames(a, m)
        say(f"  maxHistoryMoved {history_moved:2d}: reprojected + 4 frames {rmse(a, hit):.5f} (ratio {rmse(a, hit) / rmse(alone, hit):.3f}), box texels {rmse(a, box):.5f} "
            f"(ratio {rmse(a, box) / rmse(alone, box):.3f}); {int((info['carried'] & hit).sum())} of {int(hit.sum())} hit texels carried, "
            f"{int((info['carried'] & box).sum())} of {int(box.sum())} box texels")
    a, m, info = rr.reproject(mean, moments, f0, (F(w), F(h)), new, old, (w, h))
    a = plus_frames(a, m)
    say(f"  mi3pt_reproject (the scene taken as static) + 4 frames {rmse(a, hit):.5f} (ratio {rmse(a, hit) / rmse(alone, hit):.3f}), box texels {rmse(a, box):.5f} "
        f"(ratio {rmse(a, box) / rmse(alone, box):.3f}); {int((info['carried'] & box).sum())} of {int(box.sum())} box texels carried from where the box WAS")


if cpu:
    on_the_cpu()
    finish()
    sys.exit(0)

w, h = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
frames, bounces = 16, 8
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
sc = scenes.dragon_class_scene()
sc.build_bvh()
sc_turned = turned(sc, 2.0, sc.camera["target"])
env = scenes.synthetic_env()
say(f"{w} x {h}, {len(sc.triangles)} triangles, {bounces} bounces; five rounds, sides alternating")
view_a = (sc.camera["position"], sc.camera_direction())
view_b = rr.orbit(sc.camera["position"], sc.camera["target"], 2.0)
ctx = capi.Context(0)
pc.upload_scene(ctx, sc, env)
ctx.enable_timing(True)
ctx.set_moments(True)
ctx.set_mean_by_count(True)
ctx.resize(w, h)
carried = {}


def one(side):
    """side: (name, the scene uploaded after the keep or None, the new view, mi3pt_reproject instead)"""
    name, upload, view, plain = side
    ctx.reset()
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2, bounces=bounces).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 1).tobytes())
    ctx.submit_frames(MASK, frames)
    ctx.flush()
    ctx.render_aovs(capi.AOV_ALL)
    if not plain:
        ctx.keep_geometry(True)
    if upload is not None:
        pc.upload_scene(ctx, upload)
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=2 + frames, bounces=bounces, position=view[0], direction=view[1]).tobytes())
    if plain:
        ctx.reproject()
    else:
        ctx.reproject_scene()
    ctx.sync()
    t = ctx.pass_time_us(capi.PASS_REPROJECT)
    n = ctx.read_moments()[..., 3]
    hit = ctx.read_aov(capi.AOV_IDS)[..., 2] == 1
    carried[name] = (int((n[hit] >= 1).sum()), int(hit.sum()), int(((n[hit] >= 1) & (n[hit] <= 8)).sum()))
    if not plain:
        ctx.keep_geometry(False)
    if upload is not None and upload is not sc:
        pc.upload_scene(ctx, sc)
    return t


sides = [("k_reproject: a 2 degree orbit", None, view_b, True),
         ("k_reproject_scene: the orbit, geometry kept, no upload", None, view_b, False),
         ("k_reproject_scene: the orbit, the same records again", sc, view_b, False),
         ("k_reproject_scene: every triangle turned by 2 degrees", sc_turned, view_a, False)]
times = {s[0]: [] for s in sides}
for s in sides:          # warm-up: code objects, the images
    one(s)
for _ in range(5):
    for s in sides:
        times[s[0]].append(one(s))
say(f"a. MI3PT_PASS_REPROJECT (HIP events) of one call, {frames} frames in the mean")
for s in sides:
    t = times[s[0]]
    c = carried[s[0]]
    say(f"  {s[0]:56s} median {np.median(t):7.1f} us   min - max {min(t):7.1f} - {max(t):7.1f} us   {c[0]} of {c[1]} hit texels carried "
        f"({100.0 * c[0] / c[1]:.1f} %), {c[2]} with n' <= 8")
ctx.close()
finish()
