"""Host logic of adaptive sampling, without a device: the exact call sequence renderUntil(adaptive=True) of the Python and the Node renderer
sends to the C ABI over a recording stand-in for the context (the idea of tests/test_convergence_host.py, whose cases adaptive=False must
still reproduce call for call), and the C ABI's declarations."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_convergence_host as tch
from mi3pt_host import Renderer, capi

ROOT = tch.ROOT
JS = tch.JS
S = [{"tiles": 4, "tiles_above": k} for k in range(8)]        # distinguishable summaries, handed out in order


class AdaptiveContext(tch.RecordingContext):
    """... and freeze_converged answers from `left`, read_sample_mask with a 2 x 2 map of which three tiles are sampled"""

    def __init__(self, script, left):
        super().__init__(script)
        self.left = list(left)

    def __getattr__(self, name):
        record = super().__getattr__(name)

        def answer(*args):
            out = record(*args)
            if name == "freeze_converged":
                return self.left.pop(0)
            if name == "read_sample_mask":
                return np.array([[1, 1], [0, 1]], np.uint8)
            return out
        return answer


def _sequence(calls):
    """tch._sequence plus Z = freeze_converged, M = read_sample_mask"""
    letters = {"submit": "S", "flush": "F", "estimate_convergence": "E", "estimateConvergence": "E", "read_convergence": "R", "readConvergence": "R",
               "freeze_converged": "Z", "freezeConverged": "Z", "read_sample_mask": "M", "readSampleMask": "M"}
    out = []
    for c in calls:
        k = letters.get(c[0])
        if k is None:
            continue
        if out and out[-1][0] == k and k == "S":
            out[-1] = (k, out[-1][1] + 1)
        else:
            out.append((k, 1))
    return " ".join(k + (str(n) if k == "S" else "") for k, n in out)


ADAPTIVE = {
    # name: (options, tiles left after each freeze, the sequence, (converged, frames, sampled tile-frames), summaries read, events)
    "immediate": (dict(maxFrames=20, checkEvery=4, lookahead=False), [2, 0], "M S4 F E R Z S4 F E R Z", (True, 8, 4 * 3 + 4 * 2), 2,
                  ["converged", "complete"]),
    "lookahead": (dict(maxFrames=20, checkEvery=4), [2, 0], "M S4 F E S4 F R Z E S4 F R Z E R", (True, 12, 4 * 3 + 4 * 3 + 4 * 2), 3,
                  ["converged", "complete"]),
    "budget without lookahead": (dict(maxFrames=10, checkEvery=4, lookahead=False), [3, 2, 1], "M S4 F E R Z S4 F E R Z S2 F E R Z",
                                 (False, 10, 4 * 3 + 4 * 3 + 2 * 2), 3, ["complete"]),
    "budget with lookahead": (dict(maxFrames=10, checkEvery=4), [3, 1], "M S4 F E S4 F R Z E S2 F R Z E R", (False, 10, 4 * 3 + 4 * 3 + 2 * 3), 3,
                              ["complete"]),
    "converged at the budget": (dict(maxFrames=8, checkEvery=4, lookahead=False), [1, 0], "M S4 F E R Z S4 F E R Z", (True, 8, 4 * 3 + 4 * 1), 2,
                                ["complete", "converged"]),
    "guard 0": (dict(maxFrames=8, checkEvery=8, lookahead=False, guard=0), [0], "M S8 F E R Z", (True, 8, 8 * 3), 1, ["complete", "converged"]),
}


def _renderer(monkeypatch, script, left):
    r, scene, cam, events = tch._renderer(monkeypatch, script)
    r.ctx.__class__ = AdaptiveContext
    r.ctx.left = list(left)
    return r, scene, cam, events


@pytest.mark.parametrize("name", list(ADAPTIVE), ids=[n.replace(" ", "-") for n in ADAPTIVE])
def test_python_adaptive_render_until_sends(monkeypatch, name):
    options, left, sequence, (converged, frames, sampled), reads, names = ADAPTIVE[name]
    r, scene, cam, events = _renderer(monkeypatch, S, left)
    before = len(r.ctx.calls)
    out = r.renderUntil(scene, cam, 0.02, minFrames=3, adaptive=True, **options)
    calls = r.ctx.calls[before:]
    assert _sequence(calls) == sequence
    assert all(c[1:] == (0.02, 3) for c in calls if c[0] == "estimate_convergence")
    assert all(c[1:] == (options.get("guard", 1),) for c in calls if c[0] == "freeze_converged")
    assert out == {"converged": converged, "frames": frames, "summary": S[reads - 1], "sampled": sampled}
    assert out["summary"] is S[reads - 1] and r.frame == frames + 1
    assert r.status == "idle" and [e[0] for e in events] == names
    assert not r.ctx.left                                      # every scripted decision was taken


@pytest.mark.parametrize("name", list(tch.CASES), ids=[n.replace(" ", "-") for n in tch.CASES])
def test_python_adaptive_off_is_the_recorded_sequence(monkeypatch, name):
    """adaptive=False, spelled out: the sequences tests/test_convergence_host.py records, no mask call, no "sampled" """
    options, script, sequence, (converged, frames), names = tch.CASES[name]
    r, scene, cam, events = _renderer(monkeypatch, script, [])
    before = len(r.ctx.calls)
    out = r.renderUntil(scene, cam, 0.02, minFrames=3, adaptive=False, guard=0, **options)
    calls = r.ctx.calls[before:]
    assert tch._sequence(calls) == sequence and _sequence(calls) == sequence
    assert out == {"converged": converged, "frames": frames, "summary": script[-1]}
    assert [e[0] for e in events] == names


def test_python_mask_methods_forward(monkeypatch):
    r, *_ = _renderer(monkeypatch, [], [5, 6])
    mask = [[1, 0], [0, 1]]
    r.setSampleMask(mask)
    r.setSampleMask(None)
    assert r.readSampleMask().tolist() == [[1, 1], [0, 1]]
    assert r.freezeConverged() == 5 and r.freezeConverged(0) == 6
    assert r.ctx.calls[-5:] == [("set_sample_mask", mask), ("set_sample_mask", None), ("read_sample_mask",), ("freeze_converged", 1),
                                ("freeze_converged", 0)]


NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const cases = %s;
const out = {};
for (const name of Object.keys(cases)) {
  const [options, script, left] = cases[name];
  const log = [];
  const answers = script.slice(), tilesLeft = left.slice();
  const native = new Proxy({}, { get: (t, fn) => (...args) => { log.push([fn].concat(args.slice(1))); if (fn === 'tileLocalRows') return 16;
    if (fn === 'passTimeUs') return null; if (fn === 'hostBuildBvhF64') return Buffer.alloc(48 * (2 * args[0].length / 9 - 1));
    if (fn === 'hostEnvCdf') return new Float32Array(1024 * 512 * 4); if (fn === 'readConvergence') return answers.shift();
    if (fn === 'freezeConverged') return tilesLeft.shift(); if (fn === 'readSampleMask') return Uint8Array.from([1, 1, 0, 1]);
    if (fn === 'batchCapacity') return 5; return undefined; } });
  const r = new pt.Renderer({ native, handle: {}, options: { presentEveryFrame: false } });
  const { scene, camera } = buildDefaultScene(new Float32Array(1024 * 512 * 4));
  r.scalingFactor = 1;
  const events = [];
  r.on('converged', (s) => events.push(['converged', s]));
  r.on('complete', () => events.push(['complete']));
  const row = {};
  r.setMoments(true);
  r.resize(16, 16);
  if (name === 'methods') {
    const before = log.length;
    r.setSampleMask([1, 0, 0, 7]); r.setSampleMask(null);
    row.mask = Array.from(r.readSampleMask());
    row.left = [r.freezeConverged(), r.freezeConverged(0)];
    row.calls = log.slice(before).filter((c) => c[0] !== 'tileLocalRows').map((c) => c.map((v) => (v instanceof Uint8Array ? Array.from(v) : v)));
  } else {
    const before = log.length;
    row.out = r.renderUntil(scene, camera, 0.02, Object.assign({ minFrames: 3 }, options));
    row.calls = log.slice(before).filter((c) => ['submit', 'flush', 'estimateConvergence', 'readConvergence', 'freezeConverged', 'readSampleMask',
      'setSampleMask', 'batchCapacity'].includes(c[0]));
    row.frame = r.frame; row.status = r.status; row.events = events; row.left = tilesLeft.length;
  }
  out[name] = row;
}
console.log(JSON.stringify(out));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_adaptive_render_until_sends_the_same():
    camel = lambda s: {"tiles": s["tiles"], "tilesAbove": s["tiles_above"]}
    cases = {name: [dict(options, adaptive=True), [camel(s) for s in S], left] for name, (options, left, *_) in ADAPTIVE.items()}
    for name, (options, script, *_) in tch.CASES.items():
        cases["off: " + name] = [dict(options, adaptive=False, guard=0), [camel(s) for s in script], []]
    cases["methods"] = [{}, [], [5, 6]]
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"), json.dumps(cases))
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    for name, (options, left, sequence, (converged, frames, sampled), reads, names) in ADAPTIVE.items():
        row = j[name]
        assert _sequence(row["calls"]) == sequence, name
        assert all(c[1:] == [0.02, 3] for c in row["calls"] if c[0] == "estimateConvergence"), name
        assert all(c[1:] == [options.get("guard", 1)] for c in row["calls"] if c[0] == "freezeConverged"), name
        assert row["out"] == {"converged": converged, "frames": frames, "summary": camel(S[reads - 1]), "sampled": sampled}, name
        assert row["frame"] == frames + 1 and row["status"] == "idle" and row["left"] == 0, name
        assert [e[0] for e in row["events"]] == names, name
    for name, (options, script, sequence, (converged, frames), names) in tch.CASES.items():
        row = j["off: " + name]
        assert _sequence(row["calls"]) == sequence, name
        assert row["out"] == {"converged": converged, "frames": frames, "summary": camel(script[-1])}, name
    row = j["methods"]
    assert row["mask"] == [1, 1, 0, 1] and row["left"] == [5, 6]
    assert row["calls"] == [["setSampleMask", [1, 0, 0, 1]], ["setSampleMask", None], ["readSampleMask", 4], ["freezeConverged", 1], ["freezeConverged", 0]]


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.setSampleMask, typeof n.readSampleMask, typeof n.freezeConverged,"
              " typeof pt.Renderer.prototype.setSampleMask, typeof pt.Renderer.prototype.readSampleMask,"
              " typeof pt.Renderer.prototype.freezeConverged].join(' '));") % (os.path.join(JS, "mi3pt.node"), JS)
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["function"] * 6
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for name in ("setSampleMask(mask: ArrayLike<number> | null): void", "readSampleMask(): Uint8Array", "freezeConverged(guard?: 0 | 1): number",
                 "adaptive?: boolean", "guard?: 0 | 1", "sampled?: number"):
        assert name in dts, name
    demo = open(os.path.join(JS, "tools", "render_demo.js")).read()
    assert "--adaptive" in demo and "--guard" in demo and "adaptive:" in demo


def test_the_c_abi_declares_and_exports_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # added under the same number
    assert re.search(r"\bint mi3pt_set_sample_mask\(mi3pt_ctx \*ctx, const uint8_t \*tiles, size_t ntiles\);", hdr)
    assert re.search(r"\bint mi3pt_read_sample_mask\(mi3pt_ctx \*ctx, uint8_t \*dst, size_t ntiles, uint32_t \*sampled_out\);", hdr)
    assert re.search(r"\bint mi3pt_freeze_converged\(mi3pt_ctx \*ctx, int guard, uint32_t \*sampled_out\);", hdr)
    assert re.search(r"\bint mi3pt_host_freeze_tiles\(const float \*records, int tiles_x, int tiles_y, float threshold, int min_frames,\s+"
                     r"int guard, uint8_t \*mask_inout, uint32_t \*sampled_out\);", hdr)
    section = re.search(r"adaptive sampling: stop sampling the tiles that have converged.*?---- \*/", hdr, re.S).group(0)
    for phrase in ("NOT the sample mean", "NOT the image's neighbours", "keep\n * their bits", "mi3pt_resize and mi3pt_reset drop the mask",
                   "never thaws"):
        assert phrase in section, phrase
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.mi3pt_abi_version() == 4
    for name in ("mi3pt_set_sample_mask", "mi3pt_read_sample_mask", "mi3pt_freeze_converged", "mi3pt_host_freeze_tiles"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for method in ("set_sample_mask", "read_sample_mask", "freeze_converged"):
        assert callable(getattr(capi.Context, method))
    assert callable(capi.host_freeze_tiles)
    for method in ("setSampleMask", "readSampleMask", "freezeConverged", "renderUntil"):
        assert callable(getattr(Renderer, method))
