"""Host logic of the guided de-noise's firefly pre-pass without a device: the two entry points under ABI 4 in the header, the ctypes
table and the built library, and what denoiseGuided(despike = True / False) of the Python and the Node renderer send to the C ABI --
the state is set for the call and left as the option says, the default sends what it always sent -- over the recording stand-in of
tests/test_moments_host.py."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import pytest

from mi3pt_host import capi
from test_moments_host import JS, ROOT, _renderer, _sent


def test_the_c_abi_declares_and_exports_the_two_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # added under the same number
    assert re.search(r"\bint mi3pt_set_guided_despike\(mi3pt_ctx \*ctx, int enabled\);", hdr)
    assert re.search(r"\bint mi3pt_read_guided_despiked\(mi3pt_ctx \*ctx, uint32_t \*texels\);", hdr)
    since = hdr[hdr.index("Added since under the same number"):hdr.index("#define MI3PT_ABI_VERSION")]
    assert "mi3pt_set_guided_despike" in since and "mi3pt_read_guided_despiked" in since
    # context state, no flag bit: the flags are the three there were
    assert sorted(re.findall(r"#define (MI3PT_GUIDED_[A-Z]+) \d+u", hdr)) == ["MI3PT_GUIDED_PRESENT", "MI3PT_GUIDED_VARIANCE", "MI3PT_GUIDED_YOUNG"]
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.mi3pt_abi_version() == 4
    for name in ("mi3pt_set_guided_despike", "mi3pt_read_guided_despiked"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for method in ("set_guided_despike", "read_guided_despiked"):
        assert callable(getattr(capi.Context, method))
    # a null context is refused before anything is touched
    assert lib.mi3pt_set_guided_despike(None, 1) == 1
    assert lib.mi3pt_read_guided_despiked(None, None) == 1


def _state_calls(r):
    return [c for c in r.ctx.calls if c[0] == "set_guided_despike"]


def test_python_renderer_despike_option(monkeypatch):
    r = _renderer(monkeypatch, 16)
    plain = 2.0 / math.sqrt(16)
    r.denoiseGuided()                                                    # the option not given: what was always sent, the state untouched
    assert _sent(r) == (plain, 0) and _state_calls(r) == []
    r.denoiseGuided(despike=False)
    assert _sent(r) == (plain, 0) and _state_calls(r) == []
    r.denoiseGuided(despike=True)                                        # no flag bit: the state, set before the filter
    assert _sent(r) == (plain, 0) and _state_calls(r) == [("set_guided_despike", True)]
    names = [c[0] for c in r.ctx.calls]
    assert names.index("set_guided_despike") < len(names) - 1 - names[::-1].index("denoise_guided")
    r.denoiseGuided(despike=True, present=True)                          # left on: not sent again
    assert _sent(r) == (plain, capi.GUIDED_PRESENT) and len(_state_calls(r)) == 1
    r.readGuidedDespiked()
    assert r.ctx.calls[-1] == ("read_guided_despiked",)
    r.denoiseGuided()                                                    # the default is off: the call switches the state off again
    assert _sent(r) == (plain, 0) and _state_calls(r)[1:] == [("set_guided_despike", False)]
    r.setMoments(True)
    r.denoiseGuided(variance=True, young=True, despike=True)             # every mode
    assert _sent(r) == (2.0, capi.GUIDED_VARIANCE | capi.GUIDED_YOUNG) and _state_calls(r)[2:] == [("set_guided_despike", True)]
    r.denoiseGuided(variance="auto", despike=True)
    assert _sent(r) == (2.0, capi.GUIDED_VARIANCE) and len(_state_calls(r)) == 3


NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const log = [];
const native = new Proxy({}, { get: (t, name) => (...args) => { log.push([name].concat(args.slice(1))); if (name === 'tileLocalRows') return 16;
  if (name === 'passTimeUs') return null; if (name === 'hostBuildBvhF64') return Buffer.alloc(48 * (2 * args[0].length / 9 - 1));
  if (name === 'hostEnvCdf') return new Float32Array(1024 * 512 * 4); if (name === 'readGuidedDespiked') return 7; return undefined; } });
const r = new pt.Renderer({ native, handle: {}, options: {} });
const { scene, camera } = buildDefaultScene(new Float32Array(1024 * 512 * 4));
r.frames = 1000; r.scalingFactor = 1; r.resize(16, 16);
for (let i = 0; i < 16; i++) r.render(scene, camera);
const sent = () => { const c = log.filter((c) => c[0] === 'denoiseGuided').pop(); return [c[2], c[6]]; };
const states = () => log.filter((c) => c[0] === 'setGuidedDespike').map((c) => c[1]);
const row = {};
r.denoiseGuided(); row.plain = [sent(), states()];
r.denoiseGuided({ despike: false }); row.off = [sent(), states()];
r.denoiseGuided({ despike: true }); row.on = [sent(), states()];
row.order = log.map((c) => c[0]).filter((n) => n === 'setGuidedDespike' || n === 'denoiseGuided').slice(-2);
r.denoiseGuided({ despike: true, present: true }); row.onPresent = [sent(), states()];
row.count = r.readGuidedDespiked();
r.denoiseGuided(); row.offAgain = [sent(), states()];
r.setMoments(true);
r.denoiseGuided({ variance: true, young: true, despike: true }); row.every = [sent(), states()];
console.log(JSON.stringify(row));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_renderer_despike_option():
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"))
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    row = json.loads(r.stdout.strip().splitlines()[-1])
    plain = 2.0 / math.sqrt(16)
    assert row["plain"] == [[plain, 0], []] and row["off"] == [[plain, 0], []]
    assert row["on"] == [[plain, 0], [1]] and row["order"] == ["setGuidedDespike", "denoiseGuided"]
    assert row["onPresent"] == [[plain, 1], [1]] and row["count"] == 7
    assert row["offAgain"] == [[plain, 0], [1, 0]]
    assert row["every"] == [[2, 6], [1, 0, 1]]
    dts = open(os.path.join(JS, "index.d.ts")).read()
    assert "despike?: boolean" in dts and "readGuidedDespiked(): number" in dts
    demo = open(os.path.join(JS, "tools", "render_demo.js")).read()
    assert "--despike" in demo and "despike })" in demo


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.setGuidedDespike, typeof n.readGuidedDespiked, typeof pt.Renderer.prototype.readGuidedDespiked].join(' '));"
              ) % (os.path.join(JS, "mi3pt.node"), JS)
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["function"] * 3
