"""The Node host's denoiseGuided / readGuided against the ctypes host: render_demo.js --guided at 64 x 64, then the same filter through
capi.Context on the Node host's own accumulation image -- the filtered bytes are equal."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptcommon as pc
from mi3pt_host import capi, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-pathtracer_amd", "js")


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_host_filters_the_same_bytes(gpu_ctx, demo, env, tmp_path):
    node = shutil.which("node")
    w = h = 64
    frames = 2
    env_path = tmp_path / "env.f32"
    env_path.write_bytes(env.tobytes())
    out = str(tmp_path / "demo")
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(env_path), "--width", str(w), "--height", str(h),
                        "--frames", str(frames), "--bounces", "4", "--out", out, "--guided"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["status"] == "idle" and summary["frame"] == frames + 1
    assert open(out + "_guided.png", "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    got = np.frombuffer(open(out + "_guided.f32", "rb").read(), np.float32).reshape(h, w, 4)
    acc = np.frombuffer(open(out + ".acc.f32", "rb").read(), np.float32).reshape(h, w, 4)
    dump = tmp_path / "scene"
    dump.mkdir()
    r = subprocess.run([node, os.path.join(JS, "tools", "dump_demo_scene.js"), str(dump)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cam = np.frombuffer((dump / "camera.bin").read_bytes(), layout.RAYTRACE_UNIFORMS)[0]
    u = pc.rt_uniforms(demo, w, h, position=[float(v) for v in cam["camera.position"]],
                       direction=[float(v) for v in cam["camera.direction"]], fov=float(cam["camera.fov"]))
    ctx = gpu_ctx
    ctx.set_kernel_variant(0)
    ctx.set_tile(0, 1, 8)
    pc.upload_scene(ctx, demo, env)
    ctx.resize(w, h)
    ctx.set_uniforms(capi.PASS_RAYTRACE, u.tobytes())
    ctx.render_aovs(capi.AOV_ALL)
    ctx.write_texture(capi.TEX_ACCUMULATION, acc)
    ctx.denoise_guided(3, 2.0 / np.sqrt(float(frames)), 0.35, 0.1, 0.05)       # the hosts' defaults: sigmaColor = 2 / sqrt(frames in the mean)
    want = ctx.read_guided()
    assert acc[..., :3].max() > 0.0 and not pc.same_bits(want, acc)
    assert got.tobytes() == want.tobytes(), pc.describe_diff(got, want)
