"""The Node host's renderUntil / readConvergence against the Python host: render_demo.js --until at 64 x 64, four bounces, a check every 16
frames, then the same loop through the Python Renderer -- the frame count at which the run stops, the summary and the mean are the same."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptcommon as pc
from mi3pt_host import RaytracingScene, Renderer, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-pathtracer_amd", "js")
CAMEL = {"tiles": "tiles", "tiles_above": "tilesAbove", "tiles_young": "tilesYoung", "tiles_nonfinite": "tilesNonfinite", "texels": "texels",
         "worst_tile": "worstTile", "worst_texel": "worstTexel", "n_min": "nMin", "threshold": "threshold"}


class DumpedCamera:
    """The Node demo's camera as dump_demo_scene.js writes it"""

    def __init__(self, cam):
        self.position = [float(v) for v in cam["camera.position"]]
        self.direction = [float(v) for v in cam["camera.direction"]]
        self.fov = float(cam["camera.fov"])
        self.focalDistance = float(cam["camera.focalDistance"])
        self.aperture = float(cam["camera.aperture"])

    def getWorldPosition(self):
        return self.position

    def getWorldDirection(self):
        return self.direction


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_host_stops_where_the_python_host_stops(built, demo, env, tmp_path):
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
        # the threshold: 1.02 x the sqrt(worst_tile / 3) of 96 frames, so the run stops inside the budget after several checks
        py.frames = 96
        for _ in range(96):
            py.render(scene, cam)
        py.estimateConvergence(0.0, 0)
        threshold = 1.02 * float(np.sqrt(py.readConvergence()["worst_tile"] / 3.0))
        py.reset()
        want = py.renderUntil(scene, cam, threshold, minFrames=16, maxFrames=256, checkEvery=16)
        want_acc = py.readAccumulation()
    finally:
        py.destroy()
    print(f"threshold {threshold!r}: the Python host stops after {want['frames']} frames: {want['summary']}")
    assert want["converged"] and 32 <= want["frames"] < 256
    env_path = tmp_path / "env.f32"
    env_path.write_bytes(env.tobytes())
    out = str(tmp_path / "demo")
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(env_path), "--width", str(w), "--height", str(h),
                        "--frames", "256", "--bounces", "4", "--out", out, "--until", repr(threshold), "--min-frames", "16", "--check-every", "16"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    got = summary["until"]
    assert summary["status"] == "idle" and summary["frame"] == want["frames"] + 1
    assert got["converged"] is True and got["frames"] == want["frames"]
    for name, camel in CAMEL.items():
        assert got["summary"][camel] == want["summary"][name], (name, got["summary"], want["summary"])
    assert "converged after %d of 256 frames" % want["frames"] in r.stderr
    acc = np.frombuffer(open(out + ".acc.f32", "rb").read(), np.float32).reshape(h, w, 4)
    assert acc.tobytes() == want_acc.tobytes(), "the two hosts did not render the same frames: " + pc.describe_diff(acc, want_acc)
