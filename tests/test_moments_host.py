"""Host logic of the moments image and the variance-guided filter, without a device: what setMoments and denoiseGuided(variance = True /
False / 'auto') of the Python and the Node renderer send to the C ABI -- the flag, the sigma_color defaults, the threshold of 8 frames --
over a recording stand-in for the context (the idea of tests/test_host_side.py); and the C ABI's declarations."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mi3pt_host import Renderer, RaytracingCamera, RaytracingScene, capi, layout, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-pathtracer_amd", "js")


class RecordingContext:
    """Records what a Renderer sends to the C ABI"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name,) + args)
        return record


def _renderer(monkeypatch, frames_in_mean):
    monkeypatch.setattr(capi, "host_env_cdf", lambda env: np.zeros_like(env))
    r = Renderer(RecordingContext())
    r.frames = 1000
    r.scalingFactor = 1
    r.presentEveryFrame = False
    content = scenes.demo_scene()
    content.nodes = np.zeros(1, layout.BVH_NODE)
    scene = RaytracingScene(content, scenes.synthetic_env())
    scene.needsUpdate = True
    r.resize(16, 16)
    cam = RaytracingCamera(45.0)
    for _ in range(frames_in_mean):
        r.render(scene, cam)
    assert r.frame == frames_in_mean + 1
    return r


def _sent(r):
    """(sigma_color, flags) of the last denoise_guided"""
    call = [c for c in r.ctx.calls if c[0] == "denoise_guided"][-1]
    assert call[1] == 3 and call[3:6] == (0.35, 0.1, 0.05)
    return call[2], call[6]


def test_python_renderer_variance_option(monkeypatch):
    assert capi.GUIDED_PRESENT == 1 and capi.GUIDED_VARIANCE == 2 and Renderer.VARIANCE_AUTO_FRAMES == 8
    r = _renderer(monkeypatch, 16)
    r.denoiseGuided()                                                   # the option not given: as before
    assert _sent(r) == (2.0 / math.sqrt(16), 0)
    r.denoiseGuided(variance=False, present=True)
    assert _sent(r) == (2.0 / math.sqrt(16), capi.GUIDED_PRESENT)
    r.denoiseGuided(variance=True)
    assert _sent(r) == (2.0, capi.GUIDED_VARIANCE)                      # sigmaColor defaults to 2, not 2 / sqrt(frames)
    r.denoiseGuided(variance=True, present=True, sigmaColor=1.5)
    assert _sent(r) == (1.5, capi.GUIDED_VARIANCE | capi.GUIDED_PRESENT)
    r.denoiseGuided(variance="auto")                                    # moments off: auto is False
    assert _sent(r) == (2.0 / math.sqrt(16), 0)
    r.setMoments(True)
    assert ("set_moments", True) in r.ctx.calls
    r.denoiseGuided(variance="auto")
    assert _sent(r) == (2.0, capi.GUIDED_VARIANCE)
    r.setMoments(False)
    r.denoiseGuided(variance="auto")
    assert _sent(r) == (2.0 / math.sqrt(16), 0)
    with pytest.raises(ValueError):
        r.denoiseGuided(variance="yes")
    r.readMoments()
    r.readGuidedVariance()
    assert [c[0] for c in r.ctx.calls[-2:]] == ["read_moments", "read_guided_variance"]


@pytest.mark.parametrize("frames,on", [(1, False), (7, False), (8, True), (9, True)])
def test_python_renderer_auto_threshold(monkeypatch, frames, on):
    r = _renderer(monkeypatch, frames)
    r.setMoments(True)
    r.denoiseGuided(variance="auto")
    assert _sent(r) == ((2.0, capi.GUIDED_VARIANCE) if on else (2.0 / math.sqrt(frames), 0))


NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const log = [];
const native = new Proxy({}, { get: (t, name) => (...args) => { log.push([name].concat(args.slice(1))); if (name === 'tileLocalRows') return 16;
  if (name === 'passTimeUs') return null; if (name === 'hostBuildBvhF64') return Buffer.alloc(48 * (2 * args[0].length / 9 - 1));
  if (name === 'hostEnvCdf') return new Float32Array(1024 * 512 * 4); return undefined; } });
const out = {};
for (const frames of [1, 7, 8, 9, 16]) {
  const r = new pt.Renderer({ native, handle: {}, options: {} });
  const { scene, camera } = buildDefaultScene(new Float32Array(1024 * 512 * 4));
  r.frames = 1000; r.scalingFactor = 1; r.resize(16, 16);
  for (let i = 0; i < frames; i++) r.render(scene, camera);
  const sent = () => { const c = log.filter((c) => c[0] === 'denoiseGuided').pop(); return [c[2], c[6]]; };
  const row = {};
  r.denoiseGuided(); row.plain = sent();
  r.denoiseGuided({ variance: false, present: true }); row.off = sent();
  r.denoiseGuided({ variance: true }); row.on = sent();
  r.denoiseGuided({ variance: true, present: true, sigmaColor: 1.5 }); row.onPresent = sent();
  r.denoiseGuided({ variance: 'auto' }); row.autoWithout = sent();
  r.setMoments(true); row.setMoments = log[log.length - 1];
  r.denoiseGuided({ variance: 'auto' }); row.autoWith = sent();
  r.readMoments(); r.readGuidedVariance(); row.reads = log.slice(-4).map((c) => c[0]).filter((n) => n !== 'tileLocalRows');
  let threw = false;
  try { r.denoiseGuided({ variance: 'yes' }); } catch (e) { threw = true; }
  row.threw = threw;
  out[frames] = row;
}
console.log(JSON.stringify({ threshold: pt.VARIANCE_AUTO_FRAMES, out }));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_renderer_variance_option():
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"))
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["threshold"] == 8
    for frames, row in j["out"].items():
        n = int(frames)
        plain = 2.0 / math.sqrt(n)
        assert row["plain"] == [plain, 0] and row["off"] == [plain, 1], (n, row)
        assert row["on"] == [2, 2] and row["onPresent"] == [1.5, 3], (n, row)
        assert row["autoWithout"] == [plain, 0], (n, row)
        assert row["setMoments"] == ["setMoments", 1]
        assert row["autoWith"] == ([2, 2] if n >= 8 else [plain, 0]), (n, row)
        assert row["reads"] == ["readMoments", "readGuidedVariance"] and row["threw"] is True


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.setMoments, typeof n.readMoments, typeof n.readGuidedVariance, typeof pt.Renderer.prototype.setMoments,"
              " typeof pt.Renderer.prototype.readMoments, typeof pt.Renderer.prototype.readGuidedVariance].join(' '));") % (os.path.join(JS, "mi3pt.node"), JS)
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["function"] * 6
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for name in ("setMoments(enabled: boolean)", "readMoments(): Float32Array", "readGuidedVariance(): Float32Array", "variance?: boolean | 'auto'"):
        assert name in dts, name


def test_the_c_abi_declares_and_exports_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_GUIDED_VARIANCE 2u\b", hdr) and re.search(r"#define MI3PT_GUIDED_VARIANCE_EPS 1e-8f\b", hdr)
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # added under the same number
    new = ("mi3pt_set_moments", "mi3pt_read_moments", "mi3pt_write_moments", "mi3pt_moments_device_ptr", "mi3pt_read_guided_variance")
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.mi3pt_abi_version() == 4
    for name in new:
        assert name in capi.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint %s\(mi3pt_ctx \*ctx" % name, hdr), name
    for method in ("set_moments", "read_moments", "write_moments", "moments_device_ptr", "read_guided_variance"):
        assert callable(getattr(capi.Context, method))
