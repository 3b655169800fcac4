"""The host side of the reprojection, without a device: the C ABI's declarations, mi3pt_host_view_frame against an independent computation,
and the exact call sequence Renderer.reproject of the Python and the Node renderer sends to the C ABI -- and each of its fall-backs to
reset() -- over the recording stand-in for the context of tests/test_convergence_host.py."""
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ptcommon as pc
import reproject_reference as rr
import test_convergence_host as tch
from mi3pt_host import Renderer, RaytracingCamera, RaytracingScene, capi, layout, scenes

ROOT = tch.ROOT
JS = tch.JS
F = np.float32


# ---------------------------------------------------------------- declarations
def test_the_c_abi_declares_and_exports_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # added under the same number
    assert re.search(r"\bMI3PT_PASS_REPROJECT = 6\b", hdr) and capi.PASS_REPROJECT == 6
    assert re.search(r"\bint mi3pt_set_mean_by_count\(mi3pt_ctx \*ctx, int enabled\);", hdr)
    assert re.search(r"\bint mi3pt_host_view_frame\(const void \*raytrace_uniforms, size_t nbytes, float out\[16\]\);", hdr)
    assert re.search(r"\bint mi3pt_reproject\(mi3pt_ctx \*ctx, const mi3pt_reproject_params \*params\);", hdr)
    struct = re.search(r"typedef struct mi3pt_reproject_params \{(.*?)\} mi3pt_reproject_params;", hdr, re.S)
    fields = re.findall(r"\b(float|int|unsigned)\s+([a-z_]+);", struct.group(1))
    assert fields == [("float", "plane_tolerance"), ("float", "normal_cos_min"), ("int", "max_history"), ("unsigned", "flags")]
    assert [n for n, _ in capi.ReprojectParams._fields_] == [n for _, n in fields] and ctypes.sizeof(capi.ReprojectParams) == 16
    stream_ordered = re.search(r"STREAM ORDERED.*?\.  mi3pt_set_uniforms", hdr, re.S).group(0)
    assert "mi3pt_reproject" in stream_ordered
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.mi3pt_abi_version() == 4
    for name in ("mi3pt_set_mean_by_count", "mi3pt_host_view_frame", "mi3pt_reproject"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    # a null context is refused (MI3PT_ERR_INVALID), with or without a device
    p = capi.ReprojectParams(0.02, 0.9, 64, 0)
    assert lib.mi3pt_set_mean_by_count(None, 1) == 1 and lib.mi3pt_reproject(None, ctypes.byref(p)) == 1
    for method in ("set_mean_by_count", "reproject"):
        assert callable(getattr(capi.Context, method))
    for method in ("setMeanByCount", "reproject"):
        assert callable(getattr(Renderer, method))
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for name in ("setMeanByCount(on?: boolean): void",
                 "reproject(scene: RaytracingScene, camera: RaytracingCamera, options?: { planeTolerance?: number; normalCosMin?: number; maxHistory?: number }): boolean",
                 "'reproject'"):
        assert name in dts, name
    demo = open(os.path.join(JS, "tools", "render_demo.js")).read()
    for flag in ("--orbit", "--step", "--spp", "--reproject"):
        assert flag in demo, flag
    assert "reproject(" in demo


# ---------------------------------------------------------------- mi3pt_host_view_frame
def _ulps(a, b):
    ia = np.asarray(a, F).view(np.int32).astype(np.int64)
    ib = np.asarray(b, F).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _independent_frame(u):
    """numpy float64, written from the header's lines -- not reproject_reference.view_frame, which the other tests feed to the kernel's
    reference"""
    raw = u.tobytes()
    pos = np.frombuffer(raw, F, 3, 32).astype(np.float64)
    d = np.frombuffer(raw, F, 3, 48).astype(np.float64)
    aspect, fov = np.float64(np.frombuffer(raw, F, 1, 8)[0]), np.float64(np.frombuffer(raw, F, 1, 60)[0])
    w = -d / np.linalg.norm(d)
    up = np.array([0.0, 0.0, 1.0]) if abs(w[1]) > 0.99999 else np.array([0.0, 1.0, 0.0])
    uu = np.cross(up, w)
    uu /= np.linalg.norm(uu)
    vv = np.cross(w, uu)
    t = np.tan(fov * np.pi / 360)
    return np.concatenate([pos, [aspect], -w, [t], uu, [aspect * t], vv, [0.0]])


FRAME_CASES = {
    "the demo camera": dict(),
    "straight down": dict(position=(0.5, 3.0, -0.25), direction=(0.0, -1.0, 0.0)),
    "straight up": dict(position=(0.0, -2.0, 0.0), direction=(0.0, 2.5, 0.0)),
    "almost down": dict(direction=(0.004, -1.0, 0.001)),                # |w.y| > 0.99999: still the (0, 0, 1) up
    "just not down": dict(direction=(0.005, -1.0, 0.0)),                # |w.y| = 0.9999875: the (0, 1, 0) up
    "fov 1": dict(fov=1.0),
    "fov 179": dict(fov=179.0),
    "an unnormalised direction, another aspect": dict(direction=(3.0, -1.0, -7.0), aspect=2.39),
}


@pytest.mark.parametrize("name", list(FRAME_CASES), ids=[n.replace(" ", "-").replace(",", "") for n in FRAME_CASES])
def test_view_frame_equals_an_independent_computation(built, orc, demo, name):
    u = pc.rt_uniforms(demo, 64, 48, **FRAME_CASES[name])
    got = capi.host_view_frame(u.tobytes())
    want = _independent_frame(u)
    assert got.dtype == F and got.shape == (16,)
    assert _ulps(got, want.astype(F)).max() <= 1, (got, want)
    assert np.array_equal(got, rr.view_frame(u.tobytes()))             # (what the kernel's reference is fed elsewhere)
    fwd, uu, vv = got[4:7].astype(np.float64), got[8:11].astype(np.float64), got[12:15].astype(np.float64)
    assert abs(fwd @ uu) < 1e-6 and abs(fwd @ vv) < 1e-6 and abs(uu @ vv) < 1e-6 and abs(np.linalg.norm(vv) - 1) < 1e-6
    up_z = abs(want[5]) > 0.99999
    assert abs(uu[2 if up_z else 1]) < 1e-6                              # u = up x w is at right angles to the `up` that was chosen
    # the centre ray of the ray generator points along fwd
    ray = np.asarray(orc.camera_ray(u.tobytes(), 0.5, 0.5), np.float64).ravel()
    assert np.abs(ray[-3:] - fwd).max() <= 1e-6, (ray, fwd)


def test_view_frame_refuses_invalid_input(built, demo):
    lib = capi.load_library()
    good = pc.rt_uniforms(demo, 64, 48).tobytes()
    out = np.zeros(16, F)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.mi3pt_host_view_frame(good, 96, ptr) == 0
    assert lib.mi3pt_host_view_frame(good, 95, ptr) == 1 and lib.mi3pt_host_view_frame(good + b"\0" * 4, 100, ptr) == 1
    assert lib.mi3pt_host_view_frame(None, 96, ptr) == 1 and lib.mi3pt_host_view_frame(good, 96, None) == 1
    assert "96 bytes" in capi.last_error() or "null" in capi.last_error()
    bad = [dict(direction=(0.0, 0.0, 0.0)), dict(direction=(float("nan"), 0.0, 1.0)), dict(direction=(float("inf"), 0.0, 1.0)),
           dict(fov=0.0), dict(fov=180.0), dict(fov=-45.0), dict(fov=float("nan")), dict(fov=float("inf")),
           dict(position=(float("nan"), 1.0, 4.0)), dict(position=(0.0, float("-inf"), 4.0))]
    for kw in bad:
        with pytest.raises(capi.Mi3ptError) as e:
            capi.host_view_frame(pc.rt_uniforms(demo, 64, 48, **kw).tobytes())
        assert e.value.code == 1, kw


# ---------------------------------------------------------------- Renderer.reproject: what it sends
class WholeContext(tch.RecordingContext):
    """... one device, the whole image"""
    group_size = 1
    _tile = (0, 1, 8)


class RankContext(WholeContext):
    _tile = (1, 2, 8)


class GroupContext(WholeContext):
    group_size = 2


def _renderer(monkeypatch, context=WholeContext, by_count=True):
    monkeypatch.setattr(capi, "host_env_cdf", lambda env: np.zeros_like(env))
    r = Renderer(context([]))
    r.scalingFactor = 1
    r.presentEveryFrame = False
    if by_count:
        r.setMeanByCount()
    content = scenes.demo_scene()
    content.nodes = np.zeros(1, layout.BVH_NODE)
    scene = RaytracingScene(content, scenes.synthetic_env())
    scene.needsUpdate = True
    r.resize(16, 16)
    events = []
    for ev in ("reset", "reproject", "start", "complete"):
        r.on(ev, lambda ev=ev: events.append(ev))
    return r, scene, RaytracingCamera(45.0), RaytracingCamera(45.0, position=(0.5, 1.0, 4.0)), events


def _names(calls, keep=("render_aovs", "reproject", "reset", "submit", "set_moments", "set_mean_by_count")):
    return [c[0] for c in calls if c[0] in keep]


def _rt_blocks(calls):
    return [bytes(c[2]) for c in calls if c[0] == "set_uniforms" and c[1] == capi.PASS_RAYTRACE]


def test_python_set_mean_by_count_enables_moments_itself(monkeypatch):
    r, *_ = _renderer(monkeypatch, by_count=False)
    before = len(r.ctx.calls)
    r.setMeanByCount()
    assert r.ctx.calls[before:] == [("set_moments", True), ("set_mean_by_count", True)] and r._moments and r._meanByCount
    before = len(r.ctx.calls)
    r.setMeanByCount(True)
    r.setMeanByCount(False)
    assert r.ctx.calls[before:] == [("set_mean_by_count", True), ("set_mean_by_count", False)] and r._moments and not r._meanByCount
    r.setMeanByCount()
    r.setMoments(False)
    assert not r._meanByCount


def test_python_reproject_sends(monkeypatch):
    r, scene, cam_a, cam_b, events = _renderer(monkeypatch)
    r.frames = 5
    for _ in range(6):
        r.render(scene, cam_a)
    assert r.status == "idle" and r.frame == 6
    old_view = _rt_blocks(r.ctx.calls)[-1]
    before = len(r.ctx.calls)
    del events[:]
    assert r.reproject(scene, cam_b, maxHistory=32) is True
    calls = r.ctx.calls[before:]
    # the old view's features first, under the old uniforms; then the camera; then the call
    assert _names(calls) == ["render_aovs", "reproject"]
    at = [c[0] for c in calls].index("render_aovs")
    sent = _rt_blocks(calls[:at])
    assert sent and sent[-1][32:64] == old_view[32:64]
    new_view = _rt_blocks(calls[at:])
    assert len(new_view) == 1 and new_view[0][32:44] == np.array([0.5, 1.0, 4.0], F).tobytes() and new_view[0][:12] == old_view[:12]
    assert calls[-1] == ("reproject", 0.02, 0.9, 32)
    assert events == ["reproject", "start"] and r.status == "sampling" and r.frame == 1
    assert r._aovKey == r._aovKeyNow() and r._seedOffset == 5
    # the next frame: the budget starts over, the raytrace pass's `frame` goes on where the old view stopped, the accumulate pass's does not
    before = len(r.ctx.calls)
    r.render(scene, cam_b)
    calls = r.ctx.calls[before:]
    assert np.frombuffer(_rt_blocks(calls)[-1], "<u4", 1, 12)[0] == 2 + 5
    acc = [bytes(c[2]) for c in calls if c[0] == "set_uniforms" and c[1] == capi.PASS_ACCUMULATE][-1]
    assert np.frombuffer(acc, "<u4", 1, 8)[0] == 2
    # features that are current are not rendered again; the defaults; a paused renderer stays paused
    r.pause()
    before = len(r.ctx.calls)
    assert r.reproject(scene, cam_a) is True
    assert _names(r.ctx.calls[before:]) == ["reproject"] and r.ctx.calls[-1] == ("reproject", 0.02, 0.9, 64)
    assert r.status == "paused" and r._seedOffset == 6 and r.frame == 1


@pytest.mark.parametrize("why", ["the scene changed", "the mode is off", "no mean yet", "a tile rank", "a device group"])
def test_python_reproject_falls_back_to_reset(monkeypatch, why):
    context = {"a tile rank": RankContext, "a device group": GroupContext}.get(why, WholeContext)
    r, scene, cam_a, cam_b, events = _renderer(monkeypatch, context, by_count=why != "the mode is off")
    if why != "no mean yet":
        for _ in range(3):
            r.render(scene, cam_a)
    else:
        r.update(scene, cam_a)
    if why == "the scene changed":
        scene.needsUpdate = True
    before = len(r.ctx.calls)
    del events[:]
    assert r.reproject(scene, cam_b) is False
    assert _names(r.ctx.calls[before:]) == ["reset"] and events[0] == "reset" and "reproject" not in events
    assert r.frame == 1 and r._seedOffset == 0


NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const out = {};
function make(tile, devices) {
  const log = [];
  const native = new Proxy({}, { get: (t, fn) => (...args) => { log.push([fn].concat(args.slice(1).map((a) => (ArrayBuffer.isView(a) ? Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('hex') : a))));
    if (fn === 'tileLocalRows') return 16; if (fn === 'passTimeUs') return null;
    if (fn === 'hostBuildBvhF64') return Buffer.alloc(48 * (2 * args[0].length / 9 - 1));
    if (fn === 'hostEnvCdf') return new Float32Array(1024 * 512 * 4); return undefined; } });
  const r = new pt.Renderer({ native, handle: {}, options: { presentEveryFrame: false }, tile });
  if (devices) r.devices = devices;
  const { scene, camera } = buildDefaultScene(new Float32Array(1024 * 512 * 4));
  r.scalingFactor = 1;
  const events = [];
  for (const ev of ['reset', 'reproject', 'start', 'complete']) r.on(ev, () => events.push(ev));
  return { r, log, scene, camera, events };
}
const keep = (log) => log.filter((c) => ['renderAovs', 'reproject', 'reset', 'submit', 'setMoments', 'setMeanByCount', 'setUniforms'].includes(c[0]));
{
  const { r, log, scene, camera, events } = make();
  r.setMeanByCount();
  out.enable = keep(log).filter((c) => c[0] !== 'setUniforms');
  r.resize(16, 16);
  r.frames = 5;
  for (let i = 0; i < 6; i++) r.render(scene, camera);
  const row = { status0: r.status, frame0: r.frame };
  let before = log.length; events.length = 0;
  camera.position.x = 0.5;
  row.ok = r.reproject(scene, camera, { maxHistory: 32 });
  row.calls = keep(log.slice(before)); row.events = events.slice(); row.status = r.status; row.frame = r.frame; row.seed = r._seedOffset;
  row.current = r._aovKey === r._aovKeyNow();
  before = log.length;
  r.render(scene, camera);
  row.next = keep(log.slice(before));
  r.pause();
  before = log.length;
  row.ok2 = r.reproject(scene, camera);
  row.calls2 = keep(log.slice(before)).filter((c) => c[0] !== 'setUniforms'); row.status2 = r.status; row.seed2 = r._seedOffset;
  out.main = row;
}
for (const why of ['the scene changed', 'the mode is off', 'no mean yet', 'a tile rank', 'a device group']) {
  const { r, log, scene, camera, events } = make(why === 'a tile rank' ? { rank: 1, nranks: 2, blockRows: 8 } : undefined, why === 'a device group' ? [0, 1] : undefined);
  if (why !== 'the mode is off') r.setMeanByCount();
  r.resize(16, 16);
  if (why !== 'no mean yet') for (let i = 0; i < 3; i++) r.render(scene, camera); else r.update(scene, camera);
  if (why === 'the scene changed') scene.needsUpdate = true;
  const before = log.length; events.length = 0;
  const ok = r.reproject(scene, camera);
  out[why] = { ok, calls: keep(log.slice(before)).filter((c) => c[0] !== 'setUniforms'), events: events.slice(), frame: r.frame, seed: r._seedOffset };
}
console.log(JSON.stringify(out));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_reproject_sends_the_same():
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"))
    p = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    j = json.loads(p.stdout.strip().splitlines()[-1])
    assert j["enable"] == [["setMoments", 1], ["setMeanByCount", 1]]
    row = j["main"]
    assert row["status0"] == "idle" and row["frame0"] == 6 and row["ok"] is True
    names = [c[0] for c in row["calls"]]
    assert [n for n in names if n != "setUniforms"] == ["renderAovs", "reproject"]
    at = names.index("renderAovs")
    blocks = lambda calls: [bytes.fromhex(c[2]) for c in calls if c[0] == "setUniforms" and c[1] == 0]
    old_view, new_view = blocks(row["calls"][:at]), blocks(row["calls"][at:])
    assert old_view and old_view[-1][32:44] == np.array([0.0, 1.0, 4.0], F).tobytes()
    assert len(new_view) == 1 and new_view[0][32:44] == np.array([0.5, 1.0, 4.0], F).tobytes() and new_view[0][:12] == old_view[-1][:12]
    assert row["calls"][-1] == ["reproject", 0.02, 0.9, 32]
    assert row["events"] == ["reproject", "start"] and row["status"] == "sampling" and row["frame"] == 1 and row["seed"] == 5 and row["current"]
    assert np.frombuffer(blocks(row["next"])[-1], "<u4", 1, 12)[0] == 2 + 5
    acc = [bytes.fromhex(c[2]) for c in row["next"] if c[0] == "setUniforms" and c[1] == 1][-1]
    assert np.frombuffer(acc, "<u4", 1, 8)[0] == 2
    assert row["ok2"] is True and row["calls2"] == [["reproject", 0.02, 0.9, 64]] and row["status2"] == "paused" and row["seed2"] == 6
    for why in ("the scene changed", "the mode is off", "no mean yet", "a tile rank", "a device group"):
        row = j[why]
        assert row["ok"] is False and row["calls"] == [["reset"]] and row["events"][0] == "reset" and "reproject" not in row["events"], why
        assert row["frame"] == 1 and row["seed"] == 0, why


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.setMeanByCount, typeof n.reproject, typeof n.hostViewFrame, typeof pt.Renderer.prototype.setMeanByCount,"
              " typeof pt.Renderer.prototype.reproject].join(' '));"
              "const u = Buffer.alloc(96); u.writeFloatLE(1.5, 8); u.writeFloatLE(1, 36); u.writeFloatLE(-1, 56); u.writeFloatLE(90, 60);"
              "console.log(JSON.stringify(Array.from(n.hostViewFrame(u))));"
              "try { n.hostViewFrame(Buffer.alloc(96)); console.log('accepted'); } catch (e) { console.log('refused'); }") % (os.path.join(JS, "mi3pt.node"), JS)
    p = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[0].split() == ["function"] * 5
    frame = json.loads(lines[1])
    u = np.zeros(96, np.uint8)
    u.view(F)[[2, 9, 14, 15]] = (1.5, 1, -1, 90)
    assert np.array_equal(np.array(frame, F), capi.host_view_frame(u.tobytes()))
    assert frame[4:8] == [0, 0, -1, F(math.tan(math.pi / 4))] or _ulps(frame[7], 1.0) <= 1
    assert lines[2] == "refused"
