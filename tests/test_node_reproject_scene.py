"""The Node host's reprojection across a scene change against the Python host on the same inputs: render_demo.js --slide 3 --step 0.1
--spp 4 --reproject at 64 x 48, four bounces, then the same calls through the Python Renderer with the box where the Node host put it --
every step's mean is the same, bit for bit, and so are the final moments."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptcommon as pc
from mi3pt_host import RaytracingScene, Renderer, layout, scenes
from test_node_convergence import JS, DumpedCamera

STEPS, SPP, SLIDE = 3, 4, 0.1


def _slid(demo, x):
    """the demo scene with its box at (x, 0.4, 0.5): scenes.demo_scene's own construction, as the Node host flattens the moved mesh"""
    pos, nrm = np.array(demo.positions), np.array(demo.normals)
    box = scenes.flatten_mesh(scenes.box_geometry(0.8, 0.8, 0.8), scenes.compose_matrix(position=(x, 0.4, 0.5)), 1)
    pos[2:14], nrm[2:14] = box[0], box[1]
    return scenes.Scene(pos, nrm, demo.material_index, demo.materials)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_host_follows_the_box_as_the_python_host_does(built, demo, env, tmp_path):
    node = shutil.which("node")
    w, h = 64, 48
    env_path = tmp_path / "env.f32"
    env_path.write_bytes(env.tobytes())
    out = str(tmp_path / "demo")
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(env_path), "--width", str(w), "--height", str(h),
                        "--bounces", "4", "--out", out, "--slide", str(STEPS), "--step", str(SLIDE), "--spp", str(SPP), "--reproject",
                        "--guided-variance"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["status"] == "idle" and summary["frame"] == SPP + 1 and summary["stats"]["Triangles"] == 1998
    blocks = [np.frombuffer(open(f"{out}_step{k}.uniforms.bin", "rb").read(), layout.RAYTRACE_UNIFORMS)[0] for k in range(STEPS)]
    assert [int(b["frame"]) for b in blocks] == [1 + SPP * (k + 1) for k in range(STEPS)]          # the seed offset: no frame number twice
    assert len({b["camera.position"].tobytes() for b in blocks}) == 1                               # a fixed camera
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
        cam = DumpedCamera(blocks[0])
        for k in range(STEPS):
            if k > 0:
                scene.content = _slid(demo, 0.0 + k * SLIDE)
                scene.needsUpdate = True
                assert py.reprojectScene(scene, cam) is True
            for _ in range(SPP + 1):
                py.render(scene, cam)
            want = py.readAccumulation()
            got = np.frombuffer(open(f"{out}_step{k}.acc.f32", "rb").read(), np.float32).reshape(h, w, 4)
            assert got.tobytes() == want.tobytes(), f"step {k}: the two hosts did not render the same mean: " + pc.describe_diff(got, want)
            assert os.path.getsize(f"{out}_step{k}.png") > 0
        assert events == ["reproject"] * (STEPS - 1)
        want_moments = py.readMoments()
    finally:
        py.destroy()
    moments = np.frombuffer(open(out + "_moments.f32", "rb").read(), np.float32).reshape(h, w, 4)
    assert moments.tobytes() == want_moments.tobytes(), pc.describe_diff(moments, want_moments)
    assert moments[..., 3].max() > SPP          # a history longer than one step's frames: something was carried
