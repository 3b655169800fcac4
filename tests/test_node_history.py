"""The Node host's held history against the Python host on the same inputs: render_demo.js --slide 3 --step 0.1 --spp 4 --reproject
--validate 2 at 64 x 48, four bounces -- reprojectScene, holdHistory, two frames, mergeHistory, the remaining frames, spelled out -- then
the Python Renderer's reprojectScene(validate=2), which holds and merges on its own: every step's mean is the same, bit for bit, and so
are the final moments."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptcommon as pc
from mi3pt_host import RaytracingScene, Renderer, layout
from test_node_convergence import JS, DumpedCamera
from test_node_reproject_scene import _slid

STEPS, SPP, SLIDE, VALIDATE = 3, 4, 0.1, 2


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_host_validates_a_held_history_as_the_python_host_does(built, demo, env, tmp_path):
    node = shutil.which("node")
    w, h = 64, 48
    env_path = tmp_path / "env.f32"
    env_path.write_bytes(env.tobytes())
    out = str(tmp_path / "demo")
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(env_path), "--width", str(w), "--height", str(h),
                        "--bounces", "4", "--out", out, "--slide", str(STEPS), "--step", str(SLIDE), "--spp", str(SPP), "--reproject",
                        "--validate", str(VALIDATE), "--guided-variance"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["status"] == "idle" and summary["frame"] == SPP + 1
    kept = summary["validate"]["kept"]
    print("kept shares per step:", kept)
    assert summary["validate"]["frames"] == VALIDATE and len(kept) == STEPS - 1 and all(0.0 < k <= 1.0 for k in kept)
    blocks = [np.frombuffer(open(f"{out}_step{k}.uniforms.bin", "rb").read(), layout.RAYTRACE_UNIFORMS)[0] for k in range(STEPS)]
    py = Renderer.create()
    try:
        py.scalingFactor = 1
        py.presentEveryFrame = False
        py.frames = SPP
        py.setUniforms("raytrace", {"maxBounces": 4, "envMapIntensity": 1.0})
        py.setUniforms("accumulate", {"enabled": 1})
        py.setMeanByCount(True)
        py.resize(w, h)
        scene = RaytracingScene(demo, env)
        scene.needsUpdate = True
        cam = DumpedCamera(blocks[0])
        for k in range(STEPS):
            if k > 0:
                scene.content = _slid(demo, 0.0 + k * SLIDE)
                scene.needsUpdate = True
                assert py.reprojectScene(scene, cam, validate=VALIDATE) is True and py._validateLeft == VALIDATE
            for _ in range(SPP + 1):
                py.render(scene, cam)
            assert py._validateLeft == 0
            want = py.readAccumulation()
            got = np.frombuffer(open(f"{out}_step{k}.acc.f32", "rb").read(), np.float32).reshape(h, w, 4)
            assert got.tobytes() == want.tobytes(), f"step {k}: the two hosts did not render the same mean: " + pc.describe_diff(got, want)
        want_moments = py.readMoments()
    finally:
        py.destroy()
    moments = np.frombuffer(open(out + "_moments.f32", "rb").read(), np.float32).reshape(h, w, 4)
    assert moments.tobytes() == want_moments.tobytes(), pc.describe_diff(moments, want_moments)
    assert moments[..., 3].max() > SPP          # a history longer than one step's frames: something was kept
