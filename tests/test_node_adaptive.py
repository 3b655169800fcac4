"""The Node host's adaptive renderUntil against the Python host on the same inputs: render_demo.js --until --adaptive at 64 x 64, four
bounces, a check every 16 frames, both guards, with and without lookahead, then the same loop through the Python Renderer -- the frame
count at which the run stops, the tile-frames sampled, the summary, the final mask, the mean and the moments are the same."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptcommon as pc
from mi3pt_host import RaytracingScene, Renderer, layout
from test_node_convergence import CAMEL, JS, DumpedCamera

THRESHOLD = 0.08          # (the demo at 64 x 64 converges within 160 frames, tiles freezing at several checks: tests/test_gpu_adaptive.py)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
@pytest.mark.parametrize("guard,lookahead", [(1, True), (0, False)], ids=["guard-lookahead", "no-guard-immediate"])
def test_node_host_samples_what_the_python_host_samples(built, demo, env, tmp_path, guard, lookahead):
    node = shutil.which("node")
    w = h = 64
    dump = tmp_path / "scene"
    dump.mkdir()
    r = subprocess.run([node, os.path.join(JS, "tools", "dump_demo_scene.js"), str(dump)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cam = DumpedCamera(np.frombuffer((dump / "camera.bin").read_bytes(), layout.RAYTRACE_UNIFORMS)[0])
    py = Renderer.create()
    try:
        py.scalingFactor = 1
        py.presentEveryFrame = False
        py.setUniforms("raytrace", {"maxBounces": 4, "envMapIntensity": 1.0})
        py.setUniforms("accumulate", {"enabled": 1})
        py.setMoments(True)
        py.resize(w, h)
        scene = RaytracingScene(demo, env)
        scene.needsUpdate = True
        want = py.renderUntil(scene, cam, THRESHOLD, minFrames=16, maxFrames=160, checkEvery=16, lookahead=lookahead, adaptive=True, guard=guard)
        want_acc, want_moments, want_mask = py.readAccumulation(), py.readMoments(), py.readSampleMask()
    finally:
        py.destroy()
    print(f"guard {guard}, lookahead {lookahead}: the Python host stops after {want['frames']} frames, {want['sampled']} tile-frames")
    assert want["converged"] and 32 <= want["frames"] < 160 and want["sampled"] < 64 * want["frames"] // 2 and not want_mask.any()
    env_path = tmp_path / "env.f32"
    env_path.write_bytes(env.tobytes())
    out = str(tmp_path / "demo")
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(env_path), "--width", str(w), "--height", str(h),
                        "--frames", "160", "--bounces", "4", "--out", out, "--until", repr(THRESHOLD), "--min-frames", "16", "--check-every", "16",
                        "--adaptive", "--guard", str(guard)] + ([] if lookahead else ["--no-lookahead"]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    got = summary["until"]
    assert summary["status"] == "idle" and summary["frame"] == want["frames"] + 1
    assert got["converged"] is True and got["frames"] == want["frames"] and got["sampled"] == want["sampled"]
    for name, camel in CAMEL.items():
        assert got["summary"][camel] == want["summary"][name], (name, got["summary"], want["summary"])
    mask = np.frombuffer(open(out + "_mask.u8", "rb").read(), np.uint8).reshape(8, 8)
    assert np.array_equal(mask, want_mask)
    acc = np.frombuffer(open(out + ".acc.f32", "rb").read(), np.float32).reshape(h, w, 4)
    assert acc.tobytes() == want_acc.tobytes(), "the two hosts did not render the same frames: " + pc.describe_diff(acc, want_acc)
    moments = np.frombuffer(open(out + "_moments.f32", "rb").read(), np.float32).reshape(h, w, 4)
    assert moments.tobytes() == want_moments.tobytes(), pc.describe_diff(moments, want_moments)
