#!/usr/bin/env python3
"""Times adaptive sampling (mi3pt_set_sample_mask, Renderer.renderUntil(adaptive=True)).  1920 x 1080, the 870 k-triangle scene and view of
bench.py, 8 bounces; one process, every shape warmed, five rounds, the sides alternating inside every round; medians and min - max.
  a. the ordered mean at equal work: MI3PT_PASS_ACCUMULATE of a 16-frame launch, moments on -- k_accumulate_frames (no mask) beside
     k_accumulate_tiles under an all-ones mask;
  b. the same under partial masks: 50 %, 10 % and 1 % of the tiles sampled, scattered at random and as one contiguous band of tile rows --
     and the raytrace launch's device time beside it;
  c. what the host side of a mask change costs: mi3pt_set_sample_mask, and the enqueue (no wait) of the first launch after it -- which
     builds the tile list and copies it -- beside the enqueue of a second launch under the same mask;
  d. renderUntil adaptive (both guards) against not, with and without lookahead, at a threshold the plain run needs at least four checks
     for: wall time, frames, tile-frames sampled, and each result's RMSE of the tone-mapped mean x / (1 + x) against one long mean.
usage: python profiles/adaptive.py [WxH] [--out FILE] [--long N]   (needs a GPU; prints its lines, and appends them to FILE when one is given)"""
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


def option(name, default):
    if name in args:
        k = args.index(name)
        value = args[k + 1]
        del args[k:k + 2]
        return value
    return default


out_path = option("--out", None)
long_frames = int(option("--long", "2048"))
w, h = (int(v) for v in (args[0] if args else "1920x1080").split("x"))
frames, bounces, check_every, budget = 16, 8, 16, 512
ty, tx = (h + 7) // 8, (w + 7) // 8
lines = []
MASK = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE


def say(text):
    print(text, flush=True)
    lines.append(text)


def report(title, sides, fn, unit="us", fmt="9.1f"):
    times = {name: [] for name, _ in sides}
    for _, arg in sides:          # warm-up: code objects, the images, every mask's list
        fn(arg)
    for _ in range(5):
        for name, arg in sides:
            times[name].append(fn(arg))
    say(title)
    for name, _ in sides:
        t = np.array(times[name], np.float64)
        if t.ndim == 1:
            say(f"  {name:44s} median {np.median(t):{fmt}} {unit}   min - max {t.min():{fmt}} - {t.max():{fmt}} {unit}")
        else:
            say(f"  {name:44s} " + "   ".join(f"median {np.median(c):{fmt}} ({c.min():{fmt}} - {c.max():{fmt}}) {unit}" for c in t.T))
    return {name: np.median(np.array(t, np.float64), axis=0) for name, t in times.items()}


sc = scenes.dragon_class_scene()
sc.build_bvh()
env = scenes.synthetic_env()
say(f"{w} x {h}, {len(sc.triangles)} triangles, {bounces} bounces, {ty} x {tx} = {ty * tx} tiles; five rounds, sides alternating")

rng = np.random.default_rng(7)


def scattered(share):
    m = np.zeros(ty * tx, np.uint8)
    m[rng.choice(ty * tx, max(1, round(share * ty * tx)), replace=False)] = 1
    return m.reshape(ty, tx)


def band(share):
    m = np.zeros((ty, tx), np.uint8)
    rows = max(1, round(share * ty))
    m[(ty - rows) // 2:(ty - rows) // 2 + rows] = 1
    return m


ctx = capi.Context(0)
pc.upload_scene(ctx, sc, env)
ctx.enable_timing(True)
ctx.set_moments(True)
ctx.resize(w, h)


def launch(first=1):
    ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, w, h, frame=first, bounces=bounces).tobytes())
    ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, first).tobytes())
    ctx.submit_frames(MASK, frames)


def mean_time(mask):
    """(MI3PT_PASS_ACCUMULATE, MI3PT_PASS_RAYTRACE x frames) of one 16-frame launch under `mask`"""
    ctx.reset()
    if mask is not None:
        ctx.set_sample_mask(mask)
    launch()
    ctx.sync()
    return ctx.pass_time_us(capi.PASS_ACCUMULATE), ctx.pass_time_us(capi.PASS_RAYTRACE) * frames


# ---- a. equal work ----
a = report(f"a. MI3PT_PASS_ACCUMULATE | raytrace launch (HIP events) of one launch of {frames} frames, moments on",
           [("no mask: k_accumulate_frames", None), ("all-ones mask: k_accumulate_tiles", np.ones((ty, tx), np.uint8))], mean_time)
plain, tiles = a["no mask: k_accumulate_frames"][0], a["all-ones mask: k_accumulate_tiles"][0]
traffic = w * h * (16 * frames + 64)
say(f"  traffic {traffic / 1e6:.1f} MB ({frames} slots read, mean and moments read and written): no mask {traffic / plain / 1e6:.2f} TB/s, "
    f"all-ones mask {traffic / tiles / 1e6:.2f} TB/s; k_accumulate_tiles / k_accumulate_frames = {tiles / plain:.3f}")

# ---- b. partial masks ----
sides = [("no mask", None)]
for share in (0.5, 0.1, 0.01):
    sides.append((f"{share:.0%} of the tiles, scattered", scattered(share)))
    sides.append((f"{share:.0%} of the tiles, one band of tile rows", band(share)))
b = report("b. the same under partial masks", sides, mean_time)
for name, m in sides[1:]:
    share = float(m.mean())
    say(f"  {name:44s} sampled share {share:6.3f}: mean {b[name][0] / b['no mask'][0]:6.3f} of no mask, raytrace launch {b[name][1] / b['no mask'][1]:6.3f}")

# ---- c. the host side of a mask change ----
half = [scattered(0.5), scattered(0.5)]
flip = [0]


def host_cost(_):
    ctx.reset()
    ctx.set_sample_mask(half[flip[0]])       # (the warm-up and the previous round's list are for other masks)
    launch(1)
    ctx.sync()
    flip[0] ^= 1
    t0 = time.perf_counter()
    ctx.set_sample_mask(half[flip[0]])
    t1 = time.perf_counter()
    launch(17)
    ctx.flush()                               # enqueues; the list is built and its copy enqueued in here
    t2 = time.perf_counter()
    launch(33)
    ctx.flush()
    t3 = time.perf_counter()
    ctx.sync()
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, (t3 - t2) * 1e6


ctx.enable_timing(False)
c = report("c. host time of a mask change at 50 % scattered: mi3pt_set_sample_mask | enqueue of the first launch after it | of the next one",
           [("set | first launch | second launch", None)], host_cost)
v = c["set | first launch | second launch"]
say(f"  the list build and its copy: {v[1] - v[2]:.1f} us per mask change ({ty * tx} tiles, {int(half[0].sum()) * 4} bytes copied)")
ctx.close()

# ---- d. renderUntil, adaptive against not ----
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


def tonemapped(img):
    x = np.maximum(img[..., :3].astype(np.float64), 0.0)
    return x / (1.0 + x)


r.frames = long_frames
r.reset()
for _ in range(long_frames):
    r.render(scene, cam)
reference = tonemapped(r.readAccumulation())
# the threshold: the worst tile's estimate after each check of a plain run; 1.02 x the first one at or after the fourth check that is below
# every estimate before it, so the plain run needs that many checks
r.frames = budget
r.reset()
worst = []
for k in range(budget // check_every):
    for _ in range(check_every):
        r.render(scene, cam)
    r.estimateConvergence(0.0, 0)
    worst.append(float(np.sqrt(r.readConvergence()["worst_tile"] / 3.0)))
say("d. sqrt(worst_tile / 3) of a plain run after each check: " + ", ".join(f"{(k + 1) * check_every}: {x:.4f}" for k, x in enumerate(worst)))
pick = next((k for k in range(3, len(worst)) if worst[k] < min(worst[:k])), len(worst) - 1)
threshold = 1.02 * worst[pick]
say(f"  threshold {threshold:.5f} (1.02 x the estimate after {(pick + 1) * check_every} frames); budget {budget} frames, a check every {check_every}")
results = {}


def until(how):
    adaptive, guard, lookahead = how
    r.frames = budget
    r.reset()
    r.ctx.sync()
    t0 = time.perf_counter()
    out = r.renderUntil(scene, cam, threshold, minFrames=16, maxFrames=budget, checkEvery=check_every, lookahead=lookahead, adaptive=adaptive, guard=guard)
    r.ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3
    if how not in results:
        err = tonemapped(r.readAccumulation()) - reference
        results[how] = (out, float(np.sqrt(np.mean(err * err))))
    return ms


sides = [("plain, lookahead", (False, 1, True)), ("plain, immediate", (False, 1, False)),
         ("adaptive, guard 1, lookahead", (True, 1, True)), ("adaptive, guard 1, immediate", (True, 1, False)),
         ("adaptive, guard 0, lookahead", (True, 0, True)), ("adaptive, guard 0, immediate", (True, 0, False))]
d = report("  wall time of renderUntil", sides, until, unit="ms")
for label, how in sides:
    out, rmse = results[how]
    sampled = out.get("sampled", out["frames"] * ty * tx)
    say(f"  {label:30s} converged {out['converged']}, {out['frames']} frames, {sampled} tile-frames ({sampled / (out['frames'] * ty * tx):.3f} of "
        f"frames x tiles), RMSE of the tone-mapped mean against {long_frames} frames {rmse:.5f}, wall {float(d[label]):.1f} ms, "
        f"tiles above in the final estimate {out['summary']['tiles_above']}")
r.destroy()
if out_path:
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
