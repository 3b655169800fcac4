"""Host logic of MI3PT_GUIDED_YOUNG without a device: the header's two constants under ABI 4, the ctypes constants that mirror them, and
what denoiseGuided(young = True / False) of the Python and the Node renderer send to the C ABI -- the flag, and the 'auto' rule, which
with `young` chooses the variance mode from the first frame -- over the recording stand-in of tests/test_moments_host.py."""
import json
import math
import os
import re
import shutil
import subprocess

import pytest

from mi3pt_host import capi
from test_moments_host import JS, ROOT, _renderer, _sent

BOTH = 2 | 4


def test_the_header_defines_the_flag_under_abi_4():
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_GUIDED_YOUNG 4u\b", hdr) and re.search(r"#define MI3PT_GUIDED_YOUNG_COUNT 4\.0f\b", hdr)
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # a flag added under the same number
    assert re.search(r"#define MI3PT_GUIDED_PRESENT 1u\b", hdr) and re.search(r"#define MI3PT_GUIDED_VARIANCE 2u\b", hdr)
    assert capi.GUIDED_YOUNG == 4 and capi.GUIDED_YOUNG_COUNT == 4.0
    assert capi.GUIDED_YOUNG & (capi.GUIDED_PRESENT | capi.GUIDED_VARIANCE) == 0
    # no new entry point: the flag rides in mi3pt_guided_params.flags
    assert not [name for name in capi.SYMBOLS if "young" in name]


def test_python_renderer_young_option(monkeypatch):
    r = _renderer(monkeypatch, 16)
    r.setMoments(True)
    r.denoiseGuided(variance=True)                                       # the option not given: as before
    assert _sent(r) == (2.0, capi.GUIDED_VARIANCE)
    r.denoiseGuided(variance=True, young=False)
    assert _sent(r) == (2.0, capi.GUIDED_VARIANCE)
    r.denoiseGuided(variance=True, young=True)
    assert _sent(r) == (2.0, BOTH)
    r.denoiseGuided(variance=True, young=True, present=True, sigmaColor=1.5)
    assert _sent(r) == (1.5, BOTH | capi.GUIDED_PRESENT)
    with pytest.raises(ValueError):
        r.denoiseGuided(variance=False, young=True)                      # the flag alone is MI3PT_ERR_INVALID: refused before the call
    with pytest.raises(ValueError):
        r.denoiseGuided(young=True)
    r.setMoments(False)
    r.denoiseGuided(variance="auto", young=True)                         # moments off: auto stays the fixed sigma, and no flag
    assert _sent(r) == (2.0 / math.sqrt(16), 0)


@pytest.mark.parametrize("frames", [1, 2, 3, 7, 8, 9])
def test_python_renderer_auto_rule_with_and_without_young(monkeypatch, frames):
    r = _renderer(monkeypatch, frames)
    r.setMoments(True)
    r.denoiseGuided(variance="auto")                                     # without young: the threshold of 8 frames, unchanged
    assert _sent(r) == ((2.0, capi.GUIDED_VARIANCE) if frames >= 8 else (2.0 / math.sqrt(frames), 0))
    r.denoiseGuided(variance="auto", young=False)
    assert _sent(r) == ((2.0, capi.GUIDED_VARIANCE) if frames >= 8 else (2.0 / math.sqrt(frames), 0))
    r.denoiseGuided(variance="auto", young=True)                         # with young: the variance mode from the first frame
    assert _sent(r) == (2.0, BOTH)


NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const log = [];
const native = new Proxy({}, { get: (t, name) => (...args) => { log.push([name].concat(args.slice(1))); if (name === 'tileLocalRows') return 16;
  if (name === 'passTimeUs') return null; if (name === 'hostBuildBvhF64') return Buffer.alloc(48 * (2 * args[0].length / 9 - 1));
  if (name === 'hostEnvCdf') return new Float32Array(1024 * 512 * 4); return undefined; } });
const out = {};
for (const frames of [1, 3, 7, 8, 16]) {
  const r = new pt.Renderer({ native, handle: {}, options: {} });
  const { scene, camera } = buildDefaultScene(new Float32Array(1024 * 512 * 4));
  r.frames = 1000; r.scalingFactor = 1; r.resize(16, 16);
  for (let i = 0; i < frames; i++) r.render(scene, camera);
  const sent = () => { const c = log.filter((c) => c[0] === 'denoiseGuided').pop(); return [c[2], c[6]]; };
  const threw = (o) => { try { r.denoiseGuided(o); } catch (e) { return true; } return false; };
  const row = {};
  r.denoiseGuided({ variance: 'auto', young: true }); row.autoYoungWithout = sent();
  row.aloneThrew = threw({ young: true }); row.offThrew = threw({ variance: false, young: true });
  r.setMoments(true);
  r.denoiseGuided({ variance: true }); row.on = sent();
  r.denoiseGuided({ variance: true, young: false }); row.onNotYoung = sent();
  r.denoiseGuided({ variance: true, young: true }); row.onYoung = sent();
  r.denoiseGuided({ variance: true, young: true, present: true, sigmaColor: 1.5 }); row.onYoungPresent = sent();
  r.denoiseGuided({ variance: 'auto' }); row.auto = sent();
  r.denoiseGuided({ variance: 'auto', young: true }); row.autoYoung = sent();
  out[frames] = row;
}
console.log(JSON.stringify({ out }));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_renderer_young_option():
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"))
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    for frames, row in j["out"].items():
        n = int(frames)
        plain = 2.0 / math.sqrt(n)
        assert row["autoYoungWithout"] == [plain, 0], (n, row)           # moments off: the fixed sigma, no flag
        assert row["aloneThrew"] is True and row["offThrew"] is True, (n, row)
        assert row["on"] == [2, 2] and row["onNotYoung"] == [2, 2], (n, row)
        assert row["onYoung"] == [2, 6] and row["onYoungPresent"] == [1.5, 7], (n, row)
        assert row["auto"] == ([2, 2] if n >= 8 else [plain, 0]), (n, row)
        assert row["autoYoung"] == [2, 6], (n, row)
    dts = open(os.path.join(JS, "index.d.ts")).read()
    assert "young?: boolean" in dts
    demo = open(os.path.join(JS, "tools", "render_demo.js")).read()
    assert "--young" in demo and "young })" in demo
