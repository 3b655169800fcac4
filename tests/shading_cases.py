"""Inputs for the shading tests (test_shading_cases.py on the CPU, test_gpu_shading.py on the device, and the
palette / forced-pixel vectors of tests/golden/make_wgsl_vectors.py): reference-legal materials, environment
texels and random draws at the ends of their ranges, and what the oracle has to show for each case so that the case
is not vacuous.  No GPU in here; the functions that need the oracle are handed its module.

The hit branch of trace() (raytrace.wgsl:380-395) mixes a diffuse and a mirror direction with the weight
isSpecular * (1 - roughness), tints the throughput with mix(color, specularColor, isSpecular) and adds
emission * throughput; the palette below has every factor of those at 0, 1, out of range, NaN, huge and tiny.
"""
import numpy as np

from mi3pt_host import layout, scenes

W, H = 64, 48                      # the common image of test_gpu_shading.py
FLOOR, BOX, SPHERE = range(0, 2), range(2, 14), range(14, 1998)       # triangle ranges of scenes.demo_scene()

PALETTE = [
    scenes.WHITE,
    dict(color=(0.9, 0.85, 0.8), roughness=0.0, metalness=1.0, specularColor=(0.95, 0.8, 0.6)),      # a perfect mirror
    dict(color=(0.7, 0.7, 0.9), roughness=0.5, metalness=0.5, specularColor=(0.6, 0.9, 0.7)),
    dict(color=(0.8, 0.8, 0.8), roughness=1.5, metalness=1.0, specularColor=(1.0, 1.0, 1.0)),        # mix weight -0.5
    dict(color=(0.8, 0.8, 0.8), roughness=-1.0, metalness=2.0, specularColor=(0.9, 0.9, 0.9)),       # mix weight 2
    dict(color=(0.6, 0.7, 0.8), roughness=0.25, metalness=0.0, specularColor=(0.0, 0.0, 0.0)),       # specular only when rand() == 0
    dict(color=(0.6, 0.7, 0.8), roughness=0.25, metalness=-1.0, specularColor=(1.0, 1.0, 1.0)),      # never specular
    dict(color=(0.6, 0.7, 0.8), roughness=0.25, metalness=float("nan"), specularColor=(1.0, 1.0, 1.0)),   # NaN >= x is false
    dict(color=(0.0, 0.0, 0.0), roughness=1.0, metalness=0.0, specularColor=(1.0, 1.0, 1.0),
         emissive=(2.0, 1.0, 0.5), emissiveIntensity=1.5),
    dict(color=(0.5, 0.5, 0.5), roughness=1.0, metalness=0.0, specularColor=(1.0, 1.0, 1.0),
         emissive=(0.2, 0.4, 0.1), emissiveIntensity=-0.25),                                         # negative radiance
    dict(color=(0.5, 0.5, 0.5), roughness=1.0, metalness=0.0, specularColor=(1.0, 1.0, 1.0),
         emissive=(7e4, 7e4, 1e3), emissiveIntensity=1.0),                                           # above binary16's 65504
    dict(color=(0.5, 0.0, 0.5), roughness=1.0, metalness=0.0, specularColor=(1.0, 1.0, 1.0),
         emissive=(1e30, 1e30, 1e30), emissiveIntensity=1e10),                                       # inf; inf * 0 in the throughput
    dict(color=(2.0, 2.0, 2.0), roughness=1.0, metalness=0.1, specularColor=(1.0, 1.0, 1.0)),        # a throughput that grows
    dict(color=(1e-20, 1e-20, 1e-20), roughness=1.0, metalness=0.0, specularColor=(1.0, 1.0, 1.0),
         emissive=(1e-30, 1e-25, 1e-38), emissiveIntensity=1e-8),                                    # underflow
]


def _demo_with(material_index, materials, name):
    base = scenes.demo_scene()
    sc = scenes.Scene(base.positions, base.normals, np.asarray(material_index, np.int64), materials, name)
    sc.build_bvh()
    return sc


def palette_scene():
    """The demo scene's geometry and camera; triangle i has material (i * 7919) % 14 of PALETTE, the floor material 0."""
    n = len(scenes.demo_scene().positions)
    index = (np.arange(n, dtype=np.int64) * 7919) % len(PALETTE)
    index[:2] = 0
    return _demo_with(index, PALETTE, "palette")


def one_material_scene(material):
    """The demo geometry with one material everywhere: the first hit of a pixel decides nothing about the shading."""
    n = len(scenes.demo_scene().positions)
    return _demo_with(np.zeros(n, np.int64), [material], "one material")


EDGE_TEXELS = np.array([1e38, np.inf, np.nan, -2.0, 1e-40, 0.0], np.float32)     # pat; 1e-40 is subnormal in binary32


def edge_env():
    """scenes.synthetic_env() with rows 180 .. 299 (the band around the horizon) in 8-texel x 4-row cells of EDGE_TEXELS."""
    env = scenes.synthetic_env().copy()
    col = np.arange(env.shape[1]) // 8
    for r in range(180, 300):
        env[r, :, :3] = EDGE_TEXELS[(col + r // 4) % 6][:, None]
    return env


# ---------------------------------------------------------------- forcing a draw of rand()

M32 = 0xFFFFFFFF
LCG_MUL, LCG_INC, HASH_MUL, FRAME_MUL, SEED0 = 747796405, 2891336453, 277803737, 719393, 123456789
LCG_MUL_INV, HASH_MUL_INV, FRAME_MUL_INV = (pow(m, -1, 1 << 32) for m in (LCG_MUL, HASH_MUL, FRAME_MUL))


def hash_output(state):
    """rand()'s output function (raytrace.wgsl:253-259) of the LCG state after the step."""
    word = (((state >> ((state >> 28) + 4)) ^ state) * HASH_MUL) & M32
    return (word >> 22) ^ word


def state_for_output(result):
    """The state that hash_output maps to `result` (the function is a bijection of u32)."""
    word = result ^ (result >> 22)                   # x ^ (x >> 22) undoes itself: 2 * 22 >= 32
    t = (word * HASH_MUL_INV) & M32
    shift = (t >> 28) + 4                            # the top four bits pass through a shift of four or more
    s = t
    for _ in range(32 // shift + 1):                 # s = t ^ (s >> shift), settled from the top bits down
        s = t ^ (s >> shift)
    assert hash_output(s) == result
    return s


def forced_frame(draw, result, index):
    """The u32 `frame` uniform with which the `draw`-th rand() (1-based) of pixel index = x + y * res_x has hash
    output `result`, i.e. returns float(result) / 2^32.  seed = index + frame * 719393 + 123456789 before the first step."""
    s = state_for_output(result & M32)
    for _ in range(draw):
        s = ((s - LCG_INC) * LCG_MUL_INV) & M32
    return ((s - SEED0 - index) * FRAME_MUL_INV) & M32


def pixel_seed(frame, index):
    return (index + frame * FRAME_MUL + SEED0) & M32


# Draw order of one sample (raytrace.wgsl:423-478, :373-411): 1-4 the two disk samples (angle, radius each); at the k-th
# hit (k = 0, 1, ..) draws 5 + 7k .. 10 + 7k are randDirection (odd offsets the angle, even ones the logarithm's
# argument) and draw 11 + 7k is the metalness test.
OUT_ZERO, OUT_ONE, OUT_ONE_LOW, OUT_BELOW_ONE = 0, M32, M32 - 127, M32 - 128       # rand() = 0.0, 1.0, 1.0, 0.99999994
INVERSION_CHECKS = [(d, r) for d in (1, 2, 6, 11, 18) for r in (OUT_ZERO, OUT_ONE, OUT_ONE_LOW, OUT_BELOW_ONE)]
INVERSION_VALUES = {OUT_ZERO: 0.0, OUT_ONE: 1.0, OUT_ONE_LOW: 1.0, OUT_BELOW_ONE: float(np.float32(0.99999994))}

FORCED_PIXEL = (32, 30)            # its un-jittered ray hits the front of the box (asserted with the oracle's ray_scene)
MIRROR_PIXEL = (32, 38)            # lower on the same face: a mirror sends the path on to the floor, so a second hit exists

ROUGH_METAL = dict(color=(0.7, 0.7, 0.9), roughness=0.5, metalness=0.5, specularColor=(0.6, 0.9, 0.7))
MIRROR = dict(color=(0.9, 0.85, 0.8), roughness=0.0, metalness=1.0, specularColor=(0.95, 0.8, 0.6))


def _glossy(metalness):
    return dict(color=(0.6, 0.7, 0.8), roughness=0.25, metalness=metalness, specularColor=(0.9, 0.5, 0.2))


# name -> (draw, hash output, pixel, material, condition on the oracle's frame F, the condition's other material)
#   "nan": the forced pixel is NaN
#   "differs": the forced pixel differs from the same frame rendered with the other material
#   None: nothing beyond equality with the oracle
FORCED_CASES = {
    "1: log(0) at draw 6": (6, OUT_ZERO, FORCED_PIXEL, ROUGH_METAL, "nan", None),
    "1: log(0) at draw 8": (8, OUT_ZERO, FORCED_PIXEL, ROUGH_METAL, "nan", None),
    "1: log(0) at draw 10": (10, OUT_ZERO, FORCED_PIXEL, ROUGH_METAL, "nan", None),
    "1: log(0) at draw 13, the second hit": (13, OUT_ZERO, MIRROR_PIXEL, MIRROR, "nan", None),
    "2: zero jitter radius at draw 2": (2, OUT_ZERO, FORCED_PIXEL, ROUGH_METAL, None, None),
    "2: jitter angle 2 pi at draw 1": (1, OUT_ONE, FORCED_PIXEL, ROUGH_METAL, None, None),
    "2: direction angle 2 pi at draw 5": (5, OUT_ONE, FORCED_PIXEL, ROUGH_METAL, None, None),
    "3: metalness 0 >= rand() 0": (11, OUT_ZERO, FORCED_PIXEL, _glossy(0.0), "differs", _glossy(-1e-30)),
    "4: metalness 1 >= rand() 1": (11, OUT_ONE, FORCED_PIXEL, _glossy(1.0), "differs", _glossy(float(np.float32(0.99999994)))),
}


def forced_case_frame(name):
    draw, result, (x, y) = FORCED_CASES[name][:3]
    return forced_frame(draw, result, x + y * W)


# ---------------------------------------------------------------- the oracle's side of every case

def _add(total, cnt):
    for k, v in cnt.items():
        total[k] = total.get(k, 0) + v
    return total


def oracle_run(orc, osc, sc, rt_frames, acc_frames=None, f16=False, enabled=1, start=None, w=W, h=H, **kw):
    """Frames `rt_frames` through the raytrace pass and, with `acc_frames`, the accumulate pass on top of `start`
    (zeros): (last image or running mean, summed counters, [(frame image, mean after it)])."""
    import ptcommon as pc
    acc = np.zeros((h, w, 4), np.float32) if start is None else start
    total, steps, img = {}, [], None
    for i, f in enumerate(rt_frames):
        img, cnt = orc.raytrace(osc, pc.rt_uniforms(sc, w, h, frame=f, **kw).tobytes(), w, h, store_f16=f16)
        _add(total, cnt)
        if acc_frames is not None:
            acc = orc.accumulate(pc.acc_uniforms(w, h, acc_frames[i], enabled).tobytes(), w, h, img, acc, store_f16=f16)
        steps.append((img, acc))
    return (acc if acc_frames is not None else img), total, steps


def image_stats(img):
    """Pixels of an image with a NaN / an infinite / a negative / a subnormal component, and finite non-zero ones."""
    rgb = np.asarray(img)[..., :3]
    tiny = np.finfo(np.float32).tiny
    return {"nan": int(np.isnan(rgb).any(-1).sum()), "inf": int(np.isinf(rgb).any(-1).sum()),
            "negative": int((rgb < 0).any(-1).sum()), "subnormal": int(((np.abs(rgb) > 0) & (np.abs(rgb) < tiny)).any(-1).sum()),
            "finite_nonzero": int((np.isfinite(rgb).all(-1) & (rgb != 0).any(-1)).sum())}


PALETTE_FRAMES, PALETTE_BOUNCES = (2, 3, 4, 5), 6


def palette_reference(orc, sc, env, f16):
    """The running mean of PALETTE_FRAMES (accumulate frame = raytrace frame) and the counters of the four frames."""
    import ptcommon as pc
    mean, cnt, _ = oracle_run(orc, pc.oracle_scene(orc, sc, env), sc, PALETTE_FRAMES, PALETTE_FRAMES, f16, bounces=PALETTE_BOUNCES)
    return mean, cnt


def check_palette_stats(f32, f16):
    """Measured: F32 1 NaN pixel, 23 with an inf; F16 1 and 52 (7e4 is above binary16's largest number)."""
    print(f"palette mean, F32 storage: {f32}\npalette mean, F16 storage: {f16}")
    assert f32["nan"] >= 1 and f16["nan"] >= 1
    assert f32["inf"] >= 10 and f16["inf"] > f32["inf"]
    assert f32["finite_nonzero"] >= 2000 and f16["finite_nonzero"] >= 2000


EDGE_FRAME, EDGE_BOUNCES = 3, 5
SKY_FRAMES, SKY_PER_LAUNCH = (3, 4, 5, 6, 7, 8), 2          # three launches of two frames: the split starts with the second
# the batched run's cameras: the issue's (the demo camera: four empty tiles in the top corners) and one that looks over the scene,
# so that most of what the streaming kernel shades comes from the edge texels
SKY_CAMERAS = {"demo camera": {}, "over the scene": dict(position=(0.0, 1.2, 4.0), direction=(0.0, 0.09950371902099893, -0.9950371902099893))}
ENV_SETTINGS = [(0.0, 0.0), (-1.5, 6.2831855), (3e38, -7.5), (1.0, 100.0)]          # (envMapIntensity, envMapRotation)
POLE_POSITION, POLE_DIRECTIONS = (0.0, 3.0, 0.0), [(0.0, 1.0, 0.0), (0.0, -1.0, 0.0)]


def check_edge_env_stats(stats):
    """Measured: 320 / 216 / 256 / 242 of 3072 pixels."""
    print(f"edge environment, frame {EDGE_FRAME}: {stats}")
    for k in ("nan", "inf", "negative", "subnormal"):
        assert stats[k] >= 100, (k, stats)


def forced_reference(orc, env, name, w=W, h=H):
    """Oracle side of FORCED_CASES[name]: dict(scene, frame F, the image of F with its counters, the mean of rt frames
    (F-1, F, F+1) under accumulate frames (1, 2, 3) with its counters); asserts the first hit and the case's condition."""
    import ptcommon as pc
    draw, result, (x, y), material, condition, other = FORCED_CASES[name]
    frame = forced_case_frame(name)
    sc = one_material_scene(material)
    osc = pc.oracle_scene(orc, sc, env)
    ray = orc.camera_ray(pc.rt_uniforms(sc, w, h).tobytes(), x / w, y / h)
    hit, _ = orc.ray_scene(osc, ray[:3], ray[3:])
    assert hit[0] == 1 and abs(hit[4] - 0.9) < 1e-5 and hit[7] == 1, (name, hit)       # the box's front face: z = 0.9, normal +z
    rand, _ = orc.rand_sequence(pixel_seed(frame, x + y * w), draw)
    assert rand[-1] == np.float32(result) / np.float32(4294967296.0)
    image, cnt, _ = oracle_run(orc, osc, sc, (frame,), bounces=PALETTE_BOUNCES, w=w, h=h)
    rt_frames = tuple((frame + d) & M32 for d in (-1, 0, 1))
    mean, mean_cnt, _ = oracle_run(orc, osc, sc, rt_frames, (1, 2, 3), bounces=PALETTE_BOUNCES, w=w, h=h)
    px = image[y, x, :3]
    line = f"forced case {name}: frame {frame:#010x} pixel ({x}, {y}) = {px}"
    if condition == "nan":
        print(line)
        assert np.isnan(px).all(), (name, px)
        assert np.isnan(mean[y, x, :3]).all()
    elif condition == "differs":
        sc2 = one_material_scene(other)
        twin, _, _ = oracle_run(orc, pc.oracle_scene(orc, sc2, env), sc2, (frame,), bounces=PALETTE_BOUNCES, w=w, h=h)
        print(line + f"; with metalness {other['metalness']!r}: {twin[y, x, :3]}")
        assert not np.array_equal(px, twin[y, x, :3]), (name, px)
    else:
        print(line)
        assert np.isfinite(px).all()
    return {"scene": sc, "frame": frame, "rt_frames": rt_frames, "image": image, "counters": cnt, "mean": mean, "mean_counters": mean_cnt}


WRAP_START = 0xFFFFFFFE
# name -> (first accumulate frame, enabled, frames): the raytrace frame starts at WRAP_START in all of them.  The step BEHIND accumulate
# frame 0 is frame 1, whose weight 1 / 1 replaces the mean once more: only a run that ENDS at frame 0 shows what frame 0 itself did.
# The first three are the issue's; the last two end at 0 -- there the mean must be that one frame, not the mean in front of it.
WRAP_CASES = {"both counters wrap": (WRAP_START, 1, 4), "a mean that restarts at 0": (0, 1, 4), "accumulation disabled": (WRAP_START, 0, 4),
              "a batch of three that ends at 0": (WRAP_START, 1, 3), "a batch of four that ends at 0": (0xFFFFFFFD, 1, 4)}
WRAP_SEED_FRAME = 7            # one frame in front, so that there is a mean to replace


def wrap_reference(orc, demo, env, name):
    """Oracle side of WRAP_CASES[name]: the mean after one seed frame and the case's frames, whose counters cross 2^32 - 1."""
    import ptcommon as pc
    first, enabled, count = WRAP_CASES[name]
    osc = pc.oracle_scene(orc, demo, env)
    seed, seed_cnt, _ = oracle_run(orc, osc, demo, (WRAP_SEED_FRAME,), (1,), bounces=4)
    rt_frames = [(WRAP_START + i) & M32 for i in range(count)]
    acc_frames = [(first + i) & M32 for i in range(count)]
    mean, cnt, steps = oracle_run(orc, osc, demo, rt_frames, acc_frames, enabled=enabled, start=seed, bounces=4)
    before = seed
    for f, (img, after) in zip(acc_frames, steps):
        if f == 0 or not enabled:
            # weight 1: the mean is replaced by the frame, whatever it held (it held something else)
            assert np.array_equal(after, img) and not np.array_equal(before, img), (name, f)
        before = after
    assert 0 in acc_frames or not enabled
    stats = image_stats(mean)
    line = f"wrap case {name}: raytrace frames {[hex(f) for f in rt_frames]}, accumulate frames {[hex(f) for f in acc_frames]}, enabled {enabled}"
    if acc_frames[-1] == 0:
        # what the device's step at frame 0 did is in the image that is compared: the last frame alone, far from any mean with weight
        # 0, 1 / 2 or 2^-32 on it (the pixels at which the last frame and the mean in front of it differ)
        last, in_front = steps[-1][0], steps[-2][1]
        moved = int((last[..., :3] != in_front[..., :3]).any(-1).sum())
        assert np.array_equal(mean, last) and moved >= 2000, (name, moved)
        line += f"; the step at 0 replaces the mean at {moved} pixels"
    print(line + f"; mean {stats}")
    return {"rt_frames": rt_frames, "acc_frames": acc_frames, "enabled": enabled, "mean": mean, "counters": _add(dict(seed_cnt), cnt)}


def check_dark_env_stats(stats):
    """envMapIntensity 0: what is left is emission -- material 9's negative one and material 13's, which underflows (measured: 7 pixels
    with a negative, 18 with a subnormal component, 49 that are not black)."""
    assert stats["negative"] >= 3 and stats["subnormal"] >= 3 and stats["finite_nonzero"] <= 200, stats
