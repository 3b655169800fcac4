"""The Node host's denoiseGuided({ variance: true, young: true }) against the ctypes host: render_demo.js --guided-variance --young at
64 x 64, two frames -- every texel holds two samples and is young --, then the same frames and the same filter through capi.Context:
the filtered image and the filtered variance are the same bytes, and not those of the variance mode without the flag."""
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
def test_node_host_sets_the_flag_and_filters_the_same_bytes(built, demo, env, tmp_path):
    node = shutil.which("node")
    w = h = 64
    frames = 2
    env_path = tmp_path / "env.f32"
    env_path.write_bytes(env.tobytes())
    out = str(tmp_path / "demo")
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(env_path), "--width", str(w), "--height", str(h),
                        "--frames", str(frames), "--bounces", "4", "--out", out, "--guided-variance", "--young"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["status"] == "idle" and summary["frame"] == frames + 1
    read = lambda name, shape: np.frombuffer(open(out + name, "rb").read(), np.float32).reshape(shape)
    acc, moments = read(".acc.f32", (h, w, 4)), read("_moments.f32", (h, w, 4))
    guided, variance = read("_guided.f32", (h, w, 4)), read("_guided_variance.f32", (h, w))
    dump = tmp_path / "scene"
    dump.mkdir()
    r = subprocess.run([node, os.path.join(JS, "tools", "dump_demo_scene.js"), str(dump)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cam = np.frombuffer((dump / "camera.bin").read_bytes(), layout.RAYTRACE_UNIFORMS)[0]
    view = dict(position=[float(v) for v in cam["camera.position"]], direction=[float(v) for v in cam["camera.direction"]],
                fov=float(cam["camera.fov"]))
    with capi.Context(0) as ctx:
        ctx.set_moments(True)
        pc.upload_scene(ctx, demo, env)
        ctx.resize(w, h)
        # Renderer.render(): the frame counter is incremented before the uniforms are written -- the first sample is frame 2
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(demo, w, h, frame=2, bounces=4, **view).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(w, h, 2).tobytes())
        ctx.submit_frames(capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE, frames)
        want_acc, want_moments = ctx.read_texture(capi.TEX_ACCUMULATION), ctx.read_moments()
        assert acc.tobytes() == want_acc.tobytes(), "the two hosts did not render the same frames: " + pc.describe_diff(acc, want_acc)
        assert np.all(want_moments[..., 3] == frames) and moments.tobytes() == want_moments.tobytes()
        ctx.render_aovs(capi.AOV_ALL)
        ctx.denoise_guided(3, 2.0, 0.35, 0.1, 0.05, flags=capi.GUIDED_VARIANCE)
        plain, plain_var = ctx.read_guided(), ctx.read_guided_variance()
        ctx.denoise_guided(3, 2.0, 0.35, 0.1, 0.05, flags=capi.GUIDED_VARIANCE | capi.GUIDED_YOUNG)
        want, want_var = ctx.read_guided(), ctx.read_guided_variance()
        assert not pc.same_bits(want, plain) and not pc.same_bits(want_var, plain_var)
        assert guided.tobytes() == want.tobytes(), pc.describe_diff(guided, want)
        assert variance.tobytes() == want_var.tobytes(), pc.describe_diff(variance, want_var)
