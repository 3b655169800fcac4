"""The host side of the held history, without a device: the C ABI's declarations and exports, the argument faults that need no device, and
the exact call sequence holdHistory / mergeHistory / reproject(validate=K) of the Python and the Node renderer send to the C ABI, over the
recording stand-ins of tests/test_reproject_host.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_reproject_host as trh
import test_reproject_scene_host as tsh
from mi3pt_host import Renderer, capi

ROOT, JS = trh.ROOT, trh.JS
F = np.float32
KEEP = ("render_aovs", "reproject", "reproject_scene", "hold_history", "merge_history", "reset", "submit", "set_moments", "set_mean_by_count")


# ---------------------------------------------------------------- declarations
def test_the_c_abi_declares_and_exports_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # added under the same number
    added = re.search(r"Added since under the same number.*?\*/", hdr, re.S).group(0)
    for name in ("mi3pt_hold_history", "mi3pt_merge_history", "struct mi3pt_history_params", "MI3PT_PASS_HISTORY (7)"):
        assert name in added, name
    assert re.search(r"\bMI3PT_PASS_HISTORY = 7\b", hdr) and capi.PASS_HISTORY == 7
    assert re.search(r"#define MI3PT_HISTORY_EPS 1e-8f\b", hdr)
    assert re.search(r"\bint mi3pt_hold_history\(mi3pt_ctx \*ctx\);", hdr)
    assert re.search(r"\bint mi3pt_merge_history\(mi3pt_ctx \*ctx, const mi3pt_history_params \*params\);", hdr)
    struct = re.search(r"typedef struct mi3pt_history_params \{(.*?)\} mi3pt_history_params;", hdr, re.S)
    fields = re.findall(r"\b(float|int|unsigned)\s+([a-z_]+);", struct.group(1))
    assert fields == [("int", "radius"), ("float", "z_keep"), ("float", "z_drop"), ("unsigned", "flags")]
    assert [n for n, _ in capi.HistoryParams._fields_] == [n for _, n in fields] and ctypes.sizeof(capi.HistoryParams) == 16
    stream_ordered = re.search(r"STREAM ORDERED.*?\.  mi3pt_set_uniforms", hdr, re.S).group(0)
    assert "mi3pt_hold_history" in stream_ordered and "mi3pt_merge_history" in stream_ordered
    assert "name other images after either call" in hdr          # the device pointers handed out earlier
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.mi3pt_abi_version() == 4
    for name in ("mi3pt_hold_history", "mi3pt_merge_history"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    for method in ("hold_history", "merge_history"):
        assert callable(getattr(capi.Context, method))
    for method in ("holdHistory", "mergeHistory"):
        assert callable(getattr(Renderer, method))
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for name in ("holdHistory(): void", "mergeHistory(options?: { radius?: number; zKeep?: number; zDrop?: number }): void", "validate?: number"):
        assert name in dts, name
    demo = open(os.path.join(JS, "tools", "render_demo.js")).read()
    assert "--validate" in demo and "holdHistory(" in demo and "mergeHistory(" in demo


def test_argument_faults_that_need_no_device(built):
    """a null context or a null parameter block is MI3PT_ERR_INVALID with or without a device, whatever the other argument holds"""
    lib = capi.load_library()
    lib.mi3pt_last_error.restype = ctypes.c_char_p
    assert lib.mi3pt_hold_history(None) == 1
    for p in (capi.HistoryParams(1, 2.0, 4.0, 0), capi.HistoryParams(7, -1.0, float("nan"), 9)):
        assert lib.mi3pt_merge_history(None, ctypes.byref(p)) == 1
        assert b"null" in lib.mi3pt_last_error()
    assert lib.mi3pt_merge_history(None, None) == 1
    out = ctypes.c_float()
    assert lib.mi3pt_pass_time_us(None, capi.PASS_HISTORY, ctypes.byref(out)) == 1


# ---------------------------------------------------------------- the Python Renderer: what it sends
def _names(calls):
    return [c[0] for c in calls if c[0] in KEEP]


def test_python_hold_and_merge_send(monkeypatch):
    r, scene, cam_a, cam_b, events = trh._renderer(monkeypatch)
    for _ in range(3):
        r.render(scene, cam_a)
    before = len(r.ctx.calls)
    r.holdHistory()
    r.render(scene, cam_a)
    r.mergeHistory()
    r.holdHistory()
    r.mergeHistory(radius=2, zKeep=1.0, zDrop=3.0)
    calls = [c for c in r.ctx.calls[before:] if c[0] in KEEP]
    assert calls == [("hold_history",), ("submit", 3), ("merge_history", 1, 2.0, 4.0), ("hold_history",), ("merge_history", 2, 1.0, 3.0)]
    assert r.frame == 5 and events == [] and r.status == "sampling"          # (the frame counter and the status are not the hold's business)


def test_python_reproject_validate_holds_and_merges_after_k_frames(monkeypatch):
    r, scene, cam_a, cam_b, events = trh._renderer(monkeypatch)
    r.frames = 8
    for _ in range(4):
        r.render(scene, cam_a)
    # validate = 0, the default: what it sent before
    before = len(r.ctx.calls)
    assert r.reproject(scene, cam_b) is True
    assert _names(r.ctx.calls[before:]) == ["render_aovs", "reproject"] and r.ctx.calls[-1] == ("reproject", 0.02, 0.9, 64)
    r.render(scene, cam_b)
    # validate = 3: hold at once, merge behind the third sampled frame, with the defaults
    before = len(r.ctx.calls)
    del events[:]
    assert r.reproject(scene, cam_a, maxHistory=32, validate=3) is True
    assert _names(r.ctx.calls[before:]) == ["reproject", "hold_history"] and r._validateLeft == 3
    assert events == ["reproject", "start"] and r.frame == 1
    for _ in range(5):
        r.render(scene, cam_a)
    calls = [c for c in r.ctx.calls[before:] if c[0] in KEEP]
    assert calls == [("reproject", 0.02, 0.9, 32), ("hold_history",), ("submit", 3), ("submit", 3), ("submit", 3), ("merge_history", 1, 2.0, 4.0),
                     ("submit", 3), ("submit", 3)]
    assert r._validateLeft == 0
    # frames that only present do not count; a paused renderer waits
    before = len(r.ctx.calls)
    assert r.reproject(scene, cam_b, validate=2) is True
    r.pause()
    r.render(scene, cam_b)
    assert r._validateLeft == 2
    r.start()
    r.render(scene, cam_b)
    r.render(scene, cam_b)
    assert _names(r.ctx.calls[before:]) == ["reproject", "hold_history", "submit", "submit", "merge_history"]
    # a move while the held history waits for its frames: it is merged on what is there, then the new move holds again
    before = len(r.ctx.calls)
    assert r.reproject(scene, cam_a, validate=4) is True
    r.render(scene, cam_a)
    assert r.reproject(scene, cam_b, validate=4) is True
    assert _names(r.ctx.calls[before:]) == ["reproject", "hold_history", "submit", "merge_history", "reproject", "hold_history"] and r._validateLeft == 4
    # a reset drops it (the context drops what it holds); so does switching the moments off
    r.reset()
    assert r._validateLeft == 0
    before = len(r.ctx.calls)
    for _ in range(5):
        r.render(scene, cam_b)
    assert "merge_history" not in _names(r.ctx.calls[before:])
    assert r.reproject(scene, cam_a, validate=2) is True
    r.setMoments(False)
    assert r._validateLeft == 0
    r.setMeanByCount(True)
    r.render(scene, cam_a)
    before = len(r.ctx.calls)
    with pytest.raises(ValueError):
        r.reproject(scene, cam_b, validate=-1)
    assert _names(r.ctx.calls[before:]) == []


def test_python_reproject_scene_validate(monkeypatch):
    r, scene, cam_a, cam_b, events = trh._renderer(monkeypatch)
    for _ in range(3):
        r.render(scene, cam_a)
    tsh._moved(scene)
    before = len(r.ctx.calls)
    assert r.reprojectScene(scene, cam_a, validate=1) is True
    r.render(scene, cam_a)
    r.render(scene, cam_a)
    assert _names(r.ctx.calls[before:]) == ["render_aovs", "reproject_scene", "hold_history", "submit", "merge_history", "submit"]
    assert [c for c in r.ctx.calls[before:] if c[0] == "reproject_scene"] == [("reproject_scene", 0.02, 0.9, 64, 8)]
    # a fall-back to reset() holds nothing
    tsh._moved(scene, fewer=True)
    before = len(r.ctx.calls)
    assert r.reprojectScene(scene, cam_a, validate=2) is False
    assert _names(r.ctx.calls[before:]) == ["reset"] and r._validateLeft == 0


# ---------------------------------------------------------------- the Node Renderer: the same
NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const log = [];
const native = new Proxy({}, { get: (t, fn) => (...args) => { log.push([fn].concat(args.slice(1).filter((a) => !ArrayBuffer.isView(a))));
  if (fn === 'tileLocalRows') return 16; if (fn === 'passTimeUs') return null;
  if (fn === 'hostBuildBvhF64') return Buffer.alloc(48 * (2 * args[0].length / 9 - 1));
  if (fn === 'hostEnvCdf') return new Float32Array(1024 * 512 * 4); return undefined; } });
const r = new pt.Renderer({ native, handle: {}, options: { presentEveryFrame: false } });
const { scene, camera } = buildDefaultScene(new Float32Array(1024 * 512 * 4));
r.scalingFactor = 1;
r.setMeanByCount();
r.resize(16, 16);
r.frames = 8;
const names = ['renderAovs', 'reproject', 'reprojectScene', 'holdHistory', 'mergeHistory', 'reset', 'submit'];
const keep = (from) => log.slice(from).filter((c) => names.includes(c[0]));
const out = {};
for (let i = 0; i < 4; i++) r.render(scene, camera);
let before = log.length;
r.holdHistory(); r.render(scene, camera); r.mergeHistory(); r.holdHistory(); r.mergeHistory({ radius: 2, zKeep: 1, zDrop: 3 });
out.plain = keep(before);
camera.position.x = 0.5;
before = log.length;
out.ok0 = r.reproject(scene, camera);
out.default = keep(before);
r.render(scene, camera);
camera.position.x = 0.25;
before = log.length;
out.ok = r.reproject(scene, camera, { maxHistory: 32, validate: 3 });
out.left = r._validateLeft;
for (let i = 0; i < 5; i++) r.render(scene, camera);
out.validated = keep(before); out.leftAfter = r._validateLeft;
camera.position.x = 0.5;
before = log.length;
r.reproject(scene, camera, { validate: 4 });
r.render(scene, camera);
camera.position.x = 0.75;
r.reproject(scene, camera, { validate: 4 });
out.moved = keep(before).map((c) => c[0]); out.leftMoved = r._validateLeft;
r.reset();
out.leftReset = r._validateLeft;
console.log(JSON.stringify(out));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_sends_the_same():
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"))
    p = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    j = json.loads(p.stdout.strip().splitlines()[-1])
    assert j["plain"] == [["holdHistory"], ["submit", 3], ["mergeHistory", 1, 2, 4], ["holdHistory"], ["mergeHistory", 2, 1, 3]]
    assert j["ok0"] is True and j["default"] == [["renderAovs", 15], ["reproject", 0.02, 0.9, 64]]
    assert j["ok"] is True and j["left"] == 3 and j["leftAfter"] == 0
    assert j["validated"] == [["reproject", 0.02, 0.9, 32], ["holdHistory"], ["submit", 3], ["submit", 3], ["submit", 3], ["mergeHistory", 1, 2, 4],
                              ["submit", 3], ["submit", 3]]
    assert j["moved"] == ["reproject", "holdHistory", "submit", "mergeHistory", "reproject", "holdHistory"] and j["leftMoved"] == 4
    assert j["leftReset"] == 0


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.holdHistory, typeof n.mergeHistory, typeof pt.Renderer.prototype.holdHistory,"
              " typeof pt.Renderer.prototype.mergeHistory].join(' '));") % (os.path.join(JS, "mi3pt.node"), JS)
    p = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[0].split() == ["function"] * 4
