"""Host logic of sampling until converged, without a device: the exact call sequence renderUntil of the Python and the Node renderer sends
to the C ABI -- chunking, flush then read then estimate with lookahead, the immediate stop without, the final estimate at the budget, the
refusal without setMoments, the events -- over a recording stand-in for the context whose read_convergence answers from a scripted list
(the idea of tests/test_moments_host.py); and the C ABI's declarations."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mi3pt_host import Renderer, RaytracingCamera, RaytracingScene, capi, layout, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-pathtracer_amd", "js")
ABOVE = {"tiles": 4, "tiles_above": 1}
DONE = {"tiles": 4, "tiles_above": 0}
NOTHING = {"tiles": 0, "tiles_above": 0}          # nothing counted is not convergence


class RecordingContext:
    """Records what a Renderer sends to the C ABI; read_convergence answers from `script`"""

    def __init__(self, script):
        self.calls = []
        self.script = list(script)

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name,) + args)
            if name == "read_convergence":
                return self.script.pop(0)
            if name == "batch_capacity":
                return 5
        return record


def _renderer(monkeypatch, script, moments=True):
    monkeypatch.setattr(capi, "host_env_cdf", lambda env: np.zeros_like(env))
    r = Renderer(RecordingContext(script))
    r.scalingFactor = 1
    r.presentEveryFrame = False
    if moments:
        r.setMoments(True)
    content = scenes.demo_scene()
    content.nodes = np.zeros(1, layout.BVH_NODE)
    scene = RaytracingScene(content, scenes.synthetic_env())
    scene.needsUpdate = True
    r.resize(16, 16)
    events = []
    r.on("converged", lambda s: events.append(("converged", s)))
    r.on("complete", lambda: events.append(("complete",)))
    return r, scene, RaytracingCamera(45.0), events


def _sequence(calls):
    """The calls that matter, run-length encoded: S = submit, F = flush, E = estimate_convergence, R = read_convergence"""
    letters = {"submit": "S", "flush": "F", "estimate_convergence": "E", "read_convergence": "R"}
    out = []
    for c in calls:
        k = letters.get(c[0]) or letters.get({"estimateConvergence": "estimate_convergence", "readConvergence": "read_convergence"}.get(c[0]))
        if k is None:
            continue
        if out and out[-1][0] == k and k == "S":
            out[-1] = (k, out[-1][1] + 1)
        else:
            out.append((k, 1))
    return " ".join(k + (str(n) if k == "S" else "") for k, n in out)


CASES = {
    # name: (options, script, the sequence, (converged, frames), status afterwards, events)
    "lookahead": (dict(maxFrames=20, checkEvery=4), [ABOVE, DONE], "S4 F E S4 F R E S4 F R", (True, 12), ["converged", "complete"]),
    "immediate": (dict(maxFrames=20, checkEvery=4, lookahead=False), [ABOVE, DONE], "S4 F E R S4 F E R", (True, 8), ["converged", "complete"]),
    "budget with lookahead": (dict(maxFrames=10, checkEvery=4), [ABOVE, ABOVE, ABOVE], "S4 F E S4 F R E S2 F R E R", (False, 10), ["complete"]),
    "budget without lookahead": (dict(maxFrames=10, checkEvery=4, lookahead=False), [ABOVE, ABOVE, ABOVE], "S4 F E R S4 F E R S2 F E R", (False, 10),
                                 ["complete"]),
    "converged by the final estimate": (dict(maxFrames=8, checkEvery=4), [ABOVE, DONE], "S4 F E S4 F R E R", (True, 8), ["complete", "converged"]),
    "one chunk": (dict(maxFrames=3, checkEvery=4), [NOTHING], "S3 F E R", (False, 3), ["complete"]),
    "the batch capacity by default": (dict(maxFrames=7), [ABOVE, ABOVE], "S5 F E S2 F R E R", (False, 7), ["complete"]),
}


@pytest.mark.parametrize("name", list(CASES), ids=[n.replace(" ", "-") for n in CASES])
def test_python_render_until_sends(monkeypatch, name):
    options, script, sequence, (converged, frames), names = CASES[name]
    r, scene, cam, events = _renderer(monkeypatch, script)
    before = len(r.ctx.calls)
    out = r.renderUntil(scene, cam, 0.02, minFrames=3, **options)
    calls = r.ctx.calls[before:]
    assert _sequence(calls) == sequence
    assert all(c[1:] == (0.02, 3) for c in calls if c[0] == "estimate_convergence")
    assert (out["converged"], out["frames"]) == (converged, frames) and r.frame == frames + 1
    script_last = CASES[name][1][-1]
    assert out["summary"] is script_last
    assert r.status == "idle" and [e[0] for e in events] == names
    if converged:
        assert [e for e in events if e[0] == "converged"][0][1] is script_last
    assert r.frames == options["maxFrames"]
    assert ("batch_capacity",) in calls if "checkEvery" not in options else ("batch_capacity",) not in calls


def test_python_render_until_refuses_without_moments_and_has_defaults(monkeypatch):
    r, scene, cam, _ = _renderer(monkeypatch, [DONE, DONE], moments=False)
    with pytest.raises(ValueError):
        r.renderUntil(scene, cam, 0.02)
    assert not [c for c in r.ctx.calls if c[0] in ("submit", "estimate_convergence")]
    r.setMoments(True)
    r.frames = 5                                                        # maxFrames None: self.frames
    out = r.renderUntil(scene, cam, 0.5)
    assert [c for c in r.ctx.calls if c[0] == "estimate_convergence"] == [("estimate_convergence", 0.5, 16)]      # minFrames 16
    assert out == {"converged": True, "frames": 5, "summary": DONE}
    r.estimateConvergence(0.25)
    r.estimateConvergence(0.25, 4)
    r.readConvergence()
    r.readConvergenceTiles()
    assert r.ctx.calls[-4:] == [("estimate_convergence", 0.25, 16), ("estimate_convergence", 0.25, 4), ("read_convergence",),
                                ("read_convergence_tiles",)]


NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const cases = %s;
const out = {};
for (const name of Object.keys(cases)) {
  const [options, script] = cases[name];
  const log = [];
  const answers = script.slice();
  const native = new Proxy({}, { get: (t, fn) => (...args) => { log.push([fn].concat(args.slice(1))); if (fn === 'tileLocalRows') return 16;
    if (fn === 'passTimeUs') return null; if (fn === 'hostBuildBvhF64') return Buffer.alloc(48 * (2 * args[0].length / 9 - 1));
    if (fn === 'hostEnvCdf') return new Float32Array(1024 * 512 * 4); if (fn === 'readConvergence') return answers.shift();
    if (fn === 'batchCapacity') return 5; return undefined; } });
  const r = new pt.Renderer({ native, handle: {}, options: { presentEveryFrame: false } });
  const { scene, camera } = buildDefaultScene(new Float32Array(1024 * 512 * 4));
  r.scalingFactor = 1;
  const events = [];
  r.on('converged', (s) => events.push(['converged', s]));
  r.on('complete', () => events.push(['complete']));
  const row = {};
  if (name === 'refusal') {
    r.resize(16, 16);
    try { r.renderUntil(scene, camera, 0.02); row.threw = false; } catch (e) { row.threw = true; }
    row.sent = log.filter((c) => c[0] === 'submit' || c[0] === 'estimateConvergence').length;
    r.setMoments(true); r.frames = 5;
    const before = log.length;
    row.out = r.renderUntil(scene, camera, 0.5);
    row.estimates = log.slice(before).filter((c) => c[0] === 'estimateConvergence');
    r.estimateConvergence(0.25); r.estimateConvergence(0.25, 4); r.readConvergence(); r.readConvergenceTiles();
    row.last = log.slice(-5).filter((c) => c[0] !== 'tileLocalRows');
  } else {
    r.setMoments(true);
    r.resize(16, 16);
    const before = log.length;
    row.out = r.renderUntil(scene, camera, 0.02, Object.assign({ minFrames: 3 }, options));
    row.calls = log.slice(before).filter((c) => ['submit', 'flush', 'estimateConvergence', 'readConvergence', 'batchCapacity'].includes(c[0]));
    row.frame = r.frame; row.status = r.status; row.frames = r.frames; row.events = events;
  }
  out[name] = row;
}
console.log(JSON.stringify(out));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_render_until_sends_the_same():
    camel = lambda s: {"tiles": s["tiles"], "tilesAbove": s["tiles_above"]}
    cases = {name: [options, [camel(s) for s in script]] for name, (options, script, *_) in CASES.items()}
    cases["refusal"] = [{}, [camel(DONE), camel(DONE)]]
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"), json.dumps(cases))
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    for name, (options, script, sequence, (converged, frames), names) in CASES.items():
        row = j[name]
        assert _sequence(row["calls"]) == sequence, name
        assert all(c[1:] == [0.02, 3] for c in row["calls"] if c[0] == "estimateConvergence"), name
        assert row["out"] == {"converged": converged, "frames": frames, "summary": camel(script[-1])}, name
        assert row["frame"] == frames + 1 and row["status"] == "idle" and row["frames"] == options["maxFrames"], name
        assert [e[0] for e in row["events"]] == names, name
        if converged:
            assert [e for e in row["events"] if e[0] == "converged"][0][1] == camel(script[-1]), name
        assert (["batchCapacity"] in row["calls"]) == ("checkEvery" not in options), name
    row = j["refusal"]
    assert row["threw"] is True and row["sent"] == 0
    assert row["estimates"] == [["estimateConvergence", 0.5, 16]]
    assert row["out"] == {"converged": True, "frames": 5, "summary": camel(DONE)}
    assert row["last"] == [["estimateConvergence", 0.25, 16], ["estimateConvergence", 0.25, 4], ["readConvergence"], ["readConvergenceTiles", 4]]


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.estimateConvergence, typeof n.readConvergence, typeof n.readConvergenceTiles, typeof n.batchCapacity,"
              " typeof pt.Renderer.prototype.estimateConvergence, typeof pt.Renderer.prototype.readConvergence,"
              " typeof pt.Renderer.prototype.readConvergenceTiles, typeof pt.Renderer.prototype.renderUntil].join(' '));") % (os.path.join(JS, "mi3pt.node"), JS)
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["function"] * 8
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for name in ("estimateConvergence(threshold: number, minFrames?: number): void", "readConvergence(): ConvergenceSummary",
                 "readConvergenceTiles(): Float32Array", "renderUntil(scene: RaytracingScene, camera: RaytracingCamera, threshold: number",
                 "export interface ConvergenceSummary", "tilesAbove: number", "'converged'"):
        assert name in dts, name
    demo = open(os.path.join(JS, "tools", "render_demo.js")).read()
    assert "--until" in demo and "renderUntil(" in demo


def test_the_c_abi_declares_and_exports_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # added under the same number
    assert re.search(r"\bMI3PT_PASS_CONVERGENCE = 5\b", hdr) and capi.PASS_CONVERGENCE == 5
    assert re.search(r"\bint mi3pt_estimate_convergence\(mi3pt_ctx \*ctx, float threshold, int min_frames\);", hdr)
    assert re.search(r"\bint mi3pt_read_convergence\(mi3pt_ctx \*ctx, mi3pt_convergence \*out\);", hdr)
    assert re.search(r"\bint mi3pt_read_convergence_tiles\(mi3pt_ctx \*ctx, float \*dst, size_t nfloats\);", hdr)
    struct = re.search(r"typedef struct mi3pt_convergence \{(.*?)\} mi3pt_convergence;", hdr, re.S)
    assert struct
    fields = re.findall(r"\b(uint32_t|uint64_t|float)\s+([a-z_, ]+);", struct.group(1))
    names = [(t, n.strip()) for t, group in fields for n in group.split(",")]
    assert names == [("uint32_t", "tiles"), ("uint32_t", "tiles_above"), ("uint32_t", "tiles_young"), ("uint32_t", "tiles_nonfinite"),
                     ("uint64_t", "texels"), ("float", "worst_tile"), ("float", "worst_texel"), ("float", "n_min"), ("float", "threshold")]
    assert [n for n, _ in capi.Convergence._fields_] == [n for _, n in names] and ctypes.sizeof(capi.Convergence) == 40
    stream_ordered = re.search(r"STREAM ORDERED.*?\.  mi3pt_set_uniforms", hdr, re.S).group(0)
    assert "mi3pt_estimate_convergence" in stream_ordered
    blocking = re.search(r"BLOCKING, but for ONE EVENT only.*?\n \*     Three things", hdr, re.S).group(0)
    assert "mi3pt_read_convergence" in blocking and "mi3pt_read_convergence_tiles" in blocking
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.mi3pt_abi_version() == 4
    for name in ("mi3pt_estimate_convergence", "mi3pt_read_convergence", "mi3pt_read_convergence_tiles"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for method in ("estimate_convergence", "read_convergence", "read_convergence_tiles"):
        assert callable(getattr(capi.Context, method))
    for method in ("estimateConvergence", "readConvergence", "readConvergenceTiles", "renderUntil"):
        assert callable(getattr(Renderer, method))
