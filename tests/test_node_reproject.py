"""The Node host's reprojection against the Python host on the same inputs: render_demo.js --orbit 3 --spp 4 --reproject at 64 x 48, four
bounces, then the same calls through the Python Renderer with the cameras the Node host used -- every view's mean is the same, bit for
bit, and so are the final moments."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptcommon as pc
from mi3pt_host import RaytracingScene, Renderer, layout
from test_node_convergence import JS, DumpedCamera

VIEWS, SPP = 3, 4


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_host_reprojects_what_the_python_host_reprojects(built, demo, env, tmp_path):
    node = shutil.which("node")
    w, h = 64, 48
    env_path = tmp_path / "env.f32"
    env_path.write_bytes(env.tobytes())
    out = str(tmp_path / "demo")
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(env_path), "--width", str(w), "--height", str(h),
                        "--bounces", "4", "--out", out, "--orbit", str(VIEWS), "--step", "2", "--spp", str(SPP), "--reproject",
                        "--guided-variance"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["status"] == "idle" and summary["frame"] == SPP + 1
    blocks = [np.frombuffer(open(f"{out}_view{v}.uniforms.bin", "rb").read(), layout.RAYTRACE_UNIFORMS)[0] for v in range(VIEWS)]
    assert [int(b["frame"]) for b in blocks] == [1 + SPP * (v + 1) for v in range(VIEWS)]          # the seed offset: no frame number twice
    assert len({b["camera.position"].tobytes() for b in blocks}) == VIEWS
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
        events = []
        py.on("reproject", lambda: events.append("reproject"))
        for v in range(VIEWS):
            cam = DumpedCamera(blocks[v])
            if v > 0:
                assert py.reproject(scene, cam) is True
            for _ in range(SPP + 1):
                py.render(scene, cam)
            want = py.readAccumulation()
            got = np.frombuffer(open(f"{out}_view{v}.acc.f32", "rb").read(), np.float32).reshape(h, w, 4)
            assert got.tobytes() == want.tobytes(), f"view {v}: the two hosts did not render the same mean: " + pc.describe_diff(got, want)
            assert os.path.getsize(f"{out}_view{v}.png") > 0
        assert events == ["reproject"] * (VIEWS - 1)
        want_moments = py.readMoments()
    finally:
        py.destroy()
    moments = np.frombuffer(open(out + "_moments.f32", "rb").read(), np.float32).reshape(h, w, 4)
    assert moments.tobytes() == want_moments.tobytes(), pc.describe_diff(moments, want_moments)
    assert moments[..., 3].max() > SPP          # a history longer than one view's frames: something was carried
