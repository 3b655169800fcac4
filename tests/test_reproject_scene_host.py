"""The host side of the reprojection across a scene change, without a device: the C ABI's declarations and exports, and the exact call
sequence Renderer.reprojectScene of the Python and the Node renderer sends to the C ABI -- each of its fall-backs to reset(), and
reproject() itself unchanged -- over the recording stand-ins of tests/test_reproject_host.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_reproject_host as trh
from mi3pt_host import Renderer, RaytracingScene, capi, layout, scenes

ROOT, JS = trh.ROOT, trh.JS
F = np.float32
KEEP = ("render_aovs", "keep_geometry", "upload_bvh", "upload_triangles", "upload_materials", "reproject_scene", "reproject", "reset", "submit")


# ---------------------------------------------------------------- declarations
def test_the_c_abi_declares_and_exports_the_new_entry_points(built):
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # added under the same number
    added = re.search(r"Added since under the same number.*?\*/", hdr, re.S).group(0)
    for name in ("mi3pt_keep_geometry", "mi3pt_reproject_scene", "struct mi3pt_reproject_scene_params"):
        assert name in added, name
    assert re.search(r"\bint mi3pt_keep_geometry\(mi3pt_ctx \*ctx, int keep\);", hdr)
    assert re.search(r"\bint mi3pt_reproject_scene\(mi3pt_ctx \*ctx, const mi3pt_reproject_scene_params \*params\);", hdr)
    struct = re.search(r"typedef struct mi3pt_reproject_scene_params \{(.*?)\} mi3pt_reproject_scene_params;", hdr, re.S)
    fields = re.findall(r"\b(float|int|unsigned)\s+([a-z_]+);", struct.group(1))
    assert fields == [("float", "plane_tolerance"), ("float", "normal_cos_min"), ("int", "max_history"), ("int", "max_history_moved"),
                      ("unsigned", "flags")]
    assert [n for n, _ in capi.ReprojectSceneParams._fields_] == [n for _, n in fields] and ctypes.sizeof(capi.ReprojectSceneParams) == 20
    assert "112 B per triangle" in hdr
    stream_ordered = re.search(r"STREAM ORDERED.*?\.  mi3pt_set_uniforms", hdr, re.S).group(0)
    assert "mi3pt_reproject_scene" in stream_ordered
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.mi3pt_abi_version() == 4
    for name in ("mi3pt_keep_geometry", "mi3pt_reproject_scene"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    # a null context is refused (MI3PT_ERR_INVALID), with or without a device
    p = capi.ReprojectSceneParams(0.02, 0.9, 64, 8, 0)
    assert lib.mi3pt_keep_geometry(None, 1) == 1 and lib.mi3pt_keep_geometry(None, 0) == 1
    assert lib.mi3pt_reproject_scene(None, ctypes.byref(p)) == 1
    for method in ("keep_geometry", "reproject_scene"):
        assert callable(getattr(capi.Context, method))
    assert callable(Renderer.reprojectScene)
    dts = open(os.path.join(JS, "index.d.ts")).read()
    assert ("reprojectScene(scene: RaytracingScene, camera: RaytracingCamera, options?: { planeTolerance?: number; normalCosMin?: number; "
            "maxHistory?: number; maxHistoryMoved?: number }): boolean") in dts
    demo = open(os.path.join(JS, "tools", "render_demo.js")).read()
    for flag in ("--slide", "--step", "--spp", "--reproject"):
        assert flag in demo, flag
    assert "reprojectScene(" in demo


# ---------------------------------------------------------------- Renderer.reprojectScene: what it sends
def _names(calls):
    return [c[0] for c in calls if c[0] in KEEP]


def _moved(scene, fewer=False):
    """the scene's content replaced by one whose triangles moved (fewer: and whose last triangle is gone)"""
    old = scene.content
    pos = np.array(old.positions, np.float64) + 0.125
    n = len(pos) - 1 if fewer else len(pos)
    content = scenes.Scene(pos[:n], np.array(old.normals)[:n], np.array(old.material_index)[:n], old.materials)
    content.nodes = np.zeros(1, layout.BVH_NODE)
    scene.content = content
    scene.needsUpdate = True


def test_python_reproject_scene_sends(monkeypatch):
    r, scene, cam_a, cam_b, events = trh._renderer(monkeypatch)
    r.frames = 5
    for _ in range(6):
        r.render(scene, cam_a)
    assert r.status == "idle" and r.frame == 6 and r._trianglesUploaded == len(scene.content.triangles) == 1998
    old_view = trh._rt_blocks(r.ctx.calls)[-1]
    _moved(scene)
    before = len(r.ctx.calls)
    del events[:]
    assert r.reprojectScene(scene, cam_b, maxHistory=32, maxHistoryMoved=4) is True
    calls = r.ctx.calls[before:]
    # the old view's features of the old scene; keep; the upload (and the camera); the call; release
    assert _names(calls) == ["render_aovs", "keep_geometry", "upload_bvh", "upload_triangles", "upload_materials", "reproject_scene", "keep_geometry"]
    kept = [c for c in calls if c[0] == "keep_geometry"]
    assert kept == [("keep_geometry", True), ("keep_geometry", False)]
    at = [c[0] for c in calls].index("render_aovs")
    sent = trh._rt_blocks(calls[:at])
    assert sent and sent[-1][32:64] == old_view[32:64]
    new_view = trh._rt_blocks(calls[at:])
    assert len(new_view) == 1 and new_view[0][32:44] == np.array([0.5, 1.0, 4.0], F).tobytes() and new_view[0][:12] == old_view[:12]
    uploaded = [c for c in calls if c[0] == "upload_triangles"][0][1]
    assert uploaded is scene.content.triangles and not scene.needsUpdate
    assert [c for c in calls if c[0] == "reproject_scene"] == [("reproject_scene", 0.02, 0.9, 32, 4)]
    assert events == ["reproject", "start"] and r.status == "sampling" and r.frame == 1
    assert r._aovKey == r._aovKeyNow() and r._seedOffset == 5
    # the next frame: the raytrace pass's `frame` goes on where the old scene stopped, the accumulate pass's starts over
    before = len(r.ctx.calls)
    r.render(scene, cam_b)
    calls = r.ctx.calls[before:]
    assert np.frombuffer(trh._rt_blocks(calls)[-1], "<u4", 1, 12)[0] == 2 + 5
    acc = [bytes(c[2]) for c in calls if c[0] == "set_uniforms" and c[1] == capi.PASS_ACCUMULATE][-1]
    assert np.frombuffer(acc, "<u4", 1, 8)[0] == 2
    # current features are not rendered again; the defaults; a paused renderer stays paused
    r.pause()
    _moved(scene)
    before = len(r.ctx.calls)
    assert r.reprojectScene(scene, cam_b) is True
    calls = r.ctx.calls[before:]
    assert _names(calls) == ["keep_geometry", "upload_bvh", "upload_triangles", "upload_materials", "reproject_scene", "keep_geometry"]
    assert [c for c in calls if c[0] == "reproject_scene"] == [("reproject_scene", 0.02, 0.9, 64, 8)]
    assert r.status == "paused" and r._seedOffset == 6 and r.frame == 1
    # with the scene unchanged it is reproject(); and reproject() itself still sends what it sent
    r.start()
    r.render(scene, cam_b)
    before = len(r.ctx.calls)
    assert r.reprojectScene(scene, cam_a, maxHistory=16, maxHistoryMoved=2) is True
    assert _names(r.ctx.calls[before:]) == ["reproject"] and r.ctx.calls[-1] == ("reproject", 0.02, 0.9, 16)
    r.render(scene, cam_a)
    before = len(r.ctx.calls)
    assert r.reproject(scene, cam_b) is True
    assert _names(r.ctx.calls[before:]) == ["reproject"] and r.ctx.calls[-1] == ("reproject", 0.02, 0.9, 64)
    _moved(scene)
    before = len(r.ctx.calls)
    assert r.reproject(scene, cam_a) is False and _names(r.ctx.calls[before:]) == ["reset"]      # (a scene change is not reproject()'s business)


FALLBACKS = ["the mode is off", "no mean yet", "a tile rank", "a device group", "no content", "nothing uploaded yet", "the count differs"]


@pytest.mark.parametrize("why", FALLBACKS)
def test_python_reproject_scene_falls_back_to_reset(monkeypatch, why):
    context = {"a tile rank": trh.RankContext, "a device group": trh.GroupContext}.get(why, trh.WholeContext)
    r, scene, cam_a, cam_b, events = trh._renderer(monkeypatch, context, by_count=why != "the mode is off")
    if why == "nothing uploaded yet":
        r.frame = 4                            # (a host that counted frames without ever rendering this scene)
        assert r._trianglesUploaded == 0
    elif why == "no mean yet":
        r.update(scene, cam_a)
    else:
        for _ in range(3):
            r.render(scene, cam_a)
    if why == "no content":
        scene.content = None
        scene.needsUpdate = True
    elif why != "nothing uploaded yet":
        _moved(scene, fewer=why == "the count differs")
    before = len(r.ctx.calls)
    del events[:]
    assert r.reprojectScene(scene, cam_b) is False
    assert _names(r.ctx.calls[before:]) == ["reset"] and events[0] == "reset" and "reproject" not in events
    assert r.frame == 1 and r._seedOffset == 0 and scene.needsUpdate


NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const out = {};
function make(tile, devices) {
  const log = [];
  const native = new Proxy({}, { get: (t, fn) => (...args) => { log.push([fn].concat(args.slice(1).map((a) => (ArrayBuffer.isView(a) ? (a.byteLength > 96 ? a.byteLength : Buffer.from(a.buffer, a.byteOffset, a.byteLength).toString('hex')) : a))));
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
const names = ['renderAovs', 'keepGeometry', 'uploadBvh', 'uploadTriangles', 'uploadMaterials', 'reprojectScene', 'reproject', 'reset', 'submit', 'setUniforms'];
const keep = (log) => log.filter((c) => names.includes(c[0]));
const noUniforms = (calls) => calls.filter((c) => c[0] !== 'setUniforms');
const box = (scene) => scene.children.find((c) => c instanceof pt.Mesh && c.geometry instanceof pt.BoxGeometry);
{
  const { r, log, scene, camera, events } = make();
  r.setMeanByCount();
  r.resize(16, 16);
  r.frames = 5;
  for (let i = 0; i < 6; i++) r.render(scene, camera);
  const row = { status0: r.status, frame0: r.frame, uploaded: r._trianglesUploaded, counted: pt.RaytracePass.countTriangles(scene) };
  let before = log.length; events.length = 0;
  box(scene).position.x += 0.125; scene.needsUpdate = true;
  camera.position.x = 0.5;
  row.ok = r.reprojectScene(scene, camera, { maxHistory: 32, maxHistoryMoved: 4 });
  row.calls = keep(log.slice(before)); row.events = events.slice(); row.status = r.status; row.frame = r.frame; row.seed = r._seedOffset;
  row.current = r._aovKey === r._aovKeyNow(); row.needsUpdate = scene.needsUpdate;
  before = log.length;
  r.render(scene, camera);
  row.next = keep(log.slice(before));
  r.pause();
  box(scene).position.x += 0.125; scene.needsUpdate = true;
  before = log.length;
  row.ok2 = r.reprojectScene(scene, camera);
  row.calls2 = noUniforms(keep(log.slice(before))); row.status2 = r.status; row.seed2 = r._seedOffset;
  r.start();
  r.render(scene, camera);
  camera.position.x = 0.25;
  before = log.length;
  row.ok3 = r.reprojectScene(scene, camera, { maxHistory: 16, maxHistoryMoved: 2 });
  row.calls3 = noUniforms(keep(log.slice(before)));
  r.render(scene, camera);
  camera.position.x = 0.5;
  before = log.length;
  row.ok4 = r.reproject(scene, camera);
  row.calls4 = noUniforms(keep(log.slice(before)));
  out.main = row;
}
for (const why of %s) {
  const { r, log, scene, camera, events } = make(why === 'a tile rank' ? { rank: 1, nranks: 2, blockRows: 8 } : undefined, why === 'a device group' ? [0, 1] : undefined);
  if (why !== 'the mode is off') r.setMeanByCount();
  r.resize(16, 16);
  if (why === 'nothing uploaded yet') r.frame = 4;
  else if (why === 'no mean yet') r.update(scene, camera);
  else for (let i = 0; i < 3; i++) r.render(scene, camera);
  if (why === 'no content') scene.clear();
  else if (why === 'the count differs') scene.remove(scene.children[scene.children.length - 1]);
  else if (why !== 'nothing uploaded yet') box(scene).position.x += 0.125;
  scene.needsUpdate = true;
  const before = log.length; events.length = 0;
  const ok = r.reprojectScene(scene, camera);
  out[why] = { ok, calls: noUniforms(keep(log.slice(before))), events: events.slice(), frame: r.frame, seed: r._seedOffset, needsUpdate: scene.needsUpdate };
}
console.log(JSON.stringify(out));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_reproject_scene_sends_the_same():
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"), json.dumps(FALLBACKS))
    p = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    j = json.loads(p.stdout.strip().splitlines()[-1])
    row = j["main"]
    assert row["status0"] == "idle" and row["frame0"] == 6 and row["uploaded"] == row["counted"] == 1998 and row["ok"] is True
    names = [c[0] for c in row["calls"]]
    assert [n for n in names if n != "setUniforms"] == ["renderAovs", "keepGeometry", "uploadBvh", "uploadTriangles", "uploadMaterials", "reprojectScene",
                                                        "keepGeometry"]
    assert [c for c in row["calls"] if c[0] == "keepGeometry"] == [["keepGeometry", 1], ["keepGeometry", 0]]
    at = names.index("renderAovs")
    blocks = lambda calls: [bytes.fromhex(c[2]) for c in calls if c[0] == "setUniforms" and c[1] == 0]
    old_view, new_view = blocks(row["calls"][:at]), blocks(row["calls"][at:])
    assert old_view and old_view[-1][32:44] == np.array([0.0, 1.0, 4.0], F).tobytes()
    assert len(new_view) == 1 and new_view[0][32:44] == np.array([0.5, 1.0, 4.0], F).tobytes() and new_view[0][:12] == old_view[-1][:12]
    assert [c for c in row["calls"] if c[0] == "uploadTriangles"] == [["uploadTriangles", 1998 * 112]]
    assert [c for c in row["calls"] if c[0] == "reprojectScene"] == [["reprojectScene", 0.02, 0.9, 32, 4]]
    assert row["events"] == ["reproject", "start"] and row["status"] == "sampling" and row["frame"] == 1 and row["seed"] == 5 and row["current"]
    assert row["needsUpdate"] is False
    assert np.frombuffer(blocks(row["next"])[-1], "<u4", 1, 12)[0] == 2 + 5
    acc = [bytes.fromhex(c[2]) for c in row["next"] if c[0] == "setUniforms" and c[1] == 1][-1]
    assert np.frombuffer(acc, "<u4", 1, 8)[0] == 2
    assert row["ok2"] is True and [c[0] for c in row["calls2"]] == ["keepGeometry", "uploadBvh", "uploadTriangles", "uploadMaterials", "reprojectScene", "keepGeometry"]
    assert row["calls2"][4] == ["reprojectScene", 0.02, 0.9, 64, 8] and row["status2"] == "paused" and row["seed2"] == 6
    # with the scene unchanged it is reproject(); reproject() itself still sends what it sent
    assert row["ok3"] is True and row["calls3"] == [["reproject", 0.02, 0.9, 16]]
    assert row["ok4"] is True and row["calls4"] == [["reproject", 0.02, 0.9, 64]]
    for why in FALLBACKS:
        row = j[why]
        assert row["ok"] is False and row["calls"] == [["reset"]] and row["events"][0] == "reset" and "reproject" not in row["events"], why
        assert row["frame"] == 1 and row["seed"] == 0 and row["needsUpdate"] is True, why


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.keepGeometry, typeof n.reprojectScene, typeof pt.Renderer.prototype.reprojectScene,"
              " typeof pt.RaytracePass.countTriangles].join(' '));") % (os.path.join(JS, "mi3pt.node"), JS)
    p = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().splitlines()[0].split() == ["function"] * 4
