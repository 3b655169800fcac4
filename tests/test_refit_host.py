"""The host side of the BVH refit, without a device: the C ABI's declarations and exports, the refusals that need no context, and what
RaytracePass.updateScene of the Python and the Node renderer sends under `refit = true` -- the refit itself, the rebuild when the
triangle count changed, the rebuild above refitCostLimit, and today's sequence with the switch off -- over recording stand-ins for the
context, as tests/test_reproject_scene_host.py drives reprojectScene."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import refit_reference as rr
import test_reproject_host as trh
from mi3pt_host import Renderer, RaytracingCamera, RaytracingScene, capi, layout, scenes

ROOT, JS = trh.ROOT, trh.JS
KEEP = ("upload_bvh", "upload_triangles", "upload_materials", "device_refit_bvh", "keep_geometry", "reproject_scene", "reset")


# ---------------------------------------------------------------- declarations
def test_the_c_abi_declares_and_exports_both_functions(built):
    hdr = open(os.path.join(ROOT, "include", "mi3pt.h")).read()
    assert re.search(r"#define MI3PT_ABI_VERSION 4\b", hdr)             # added under the same number
    added = re.search(r"Added since under the same number.*?\*/", hdr, re.S).group(0)
    for name in ("mi3pt_device_refit_bvh", "mi3pt_host_bvh_cost"):
        assert name in added, name
    assert re.search(r"\bint mi3pt_device_refit_bvh\(mi3pt_ctx \*ctx, void \*nodes_out, size_t nodes_capacity_bytes,\s*size_t \*nnodes_out, "
                     r"float \*refit_ms\);", hdr)
    assert re.search(r"\bint mi3pt_host_bvh_cost\(const void \*nodes, size_t nnodes, double \*cost\);", hdr)
    at_build, at_refit = hdr.index("int mi3pt_device_build_bvh("), hdr.index("int mi3pt_device_refit_bvh(")
    assert at_build < at_refit < hdr.index("int mi3pt_debug_set_packet_layout(")          # beside the device build
    blocking = re.search(r"BLOCKING \(the host waits.*?mi3pt_destroy\.", hdr, re.S).group(0)
    assert "mi3pt_device_refit_bvh" in blocking
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert lib.mi3pt_abi_version() == 4
    for name in ("mi3pt_device_refit_bvh", "mi3pt_host_bvh_cost"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert callable(capi.Context.device_refit_bvh) and callable(capi.host_bvh_cost)
    srcs = open(os.path.join(ROOT, "webgpu-pathtracer_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bpt_refit\.hip\b", srcs, re.M)
    dts = open(os.path.join(JS, "index.d.ts")).read()
    for text in ("refit: boolean;", "refitCostLimit: number;", "readonly lastRefitCostRatio: number | null;", "readonly lastRefitMs: number | null;",
                 "deviceRefitBvh(): { nodes: Buffer; ms: number };", "hostBvhCost(nodes: Uint8Array): number;"):
        assert text in dts, text
    demo = open(os.path.join(JS, "tools", "render_demo.js")).read()
    assert "--refit" in demo and "lastRefitCostRatio" in demo


def test_null_arguments_are_refused_without_a_device(built):
    lib = capi.load_library()
    buf = np.full(48, 0xa5, np.uint8)
    n, ms, cost = ctypes.c_size_t(12345), ctypes.c_float(-1.0), ctypes.c_double(-1.0)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.mi3pt_device_refit_bvh(None, ptr, 48, ctypes.byref(n), ctypes.byref(ms)) == 1
    assert "null context" in capi.last_error()
    assert lib.mi3pt_device_refit_bvh(None, None, 0, None, None) == 1
    assert (buf == 0xa5).all() and n.value == 12345 and ms.value == -1.0
    node = np.zeros(1, layout.BVH_NODE)
    nptr = node.ctypes.data_as(ctypes.c_void_p)
    assert lib.mi3pt_host_bvh_cost(None, 1, ctypes.byref(cost)) == 1
    assert lib.mi3pt_host_bvh_cost(nptr, 1, None) == 1
    assert lib.mi3pt_host_bvh_cost(nptr, 0, ctypes.byref(cost)) == 1
    assert cost.value == -1.0
    assert lib.mi3pt_host_bvh_cost(nptr, 1, ctypes.byref(cost)) == 0 and cost.value == 0.0


# ---------------------------------------------------------------- RaytracePass.updateScene under `refit`
class RefitContext(trh.WholeContext):
    """... whose device_refit_bvh answers with the law's records for what was uploaded last"""

    def __getattr__(self, name):
        record = super().__getattr__(name)
        if name != "device_refit_bvh":
            return record

        def refit(*args):
            record(*args)
            nodes = [c[1] for c in self.calls if c[0] == "upload_bvh"][-1]
            tris = [c[1] for c in self.calls if c[0] == "upload_triangles"][-1]
            return rr.refit_vectorised(nodes, tris), 0.125
        return refit


def _names(calls):
    return [c[0] for c in calls if c[0] in KEEP]


def _setup(monkeypatch, refit=True):
    builds = []
    real = capi.host_build_bvh_f64
    monkeypatch.setattr(capi, "host_build_bvh_f64", lambda pos, nthreads=0: (builds.append(len(pos)), real(pos, nthreads))[1])
    r, scene, cam_a, cam_b, events = trh._renderer(monkeypatch, RefitContext)
    scene.content = scenes.demo_scene()            # (nodes None: the renderer builds, as a host that sets no tree of its own has it)
    r.refit = refit
    r.frames = 3
    for _ in range(3):
        r.render(scene, cam_a)
    return r, scene, cam_a, builds


def _move(scene, slide, fewer=False):
    moved = rr.moved_demo(slide, 30.0)
    if fewer:
        moved = scenes.Scene(moved.positions[:-1], moved.normals[:-1], moved.material_index[:-1], moved.materials)
    scene.content = moved
    scene.needsUpdate = True


def test_python_refit_uploads_triangles_first_then_the_refitted_tree(monkeypatch, built):
    r, scene, cam, builds = _setup(monkeypatch)
    first = scene.content.nodes
    assert builds == [1998] and r.lastRefitCostRatio is None and r.lastRefitMs is None and r.refitCostLimit == float("inf")
    assert _names(r.ctx.calls) == ["reset", "upload_bvh", "upload_triangles", "upload_materials"]      # (resize resets) the first upload: nothing to re-fit
    before = len(r.ctx.calls)
    _move(scene, 0.3)
    r.update(scene, cam)
    calls = r.ctx.calls[before:]
    assert _names(calls) == ["upload_triangles", "device_refit_bvh", "upload_bvh", "upload_materials"]
    assert builds == [1998] and not scene.needsUpdate and r._trianglesUploaded == 1998
    want = rr.refit_vectorised(first, scene.content.triangles)
    sent = [c[1] for c in calls if c[0] == "upload_bvh"][0]
    assert sent.tobytes() == want.tobytes() and scene.content.nodes is sent           # the host's copy stays the device's
    assert r.lastRefitMs == 0.125
    assert r.lastRefitCostRatio == rr.bvh_cost(want) / rr.bvh_cost(first) and r.lastRefitCostRatio >= 1.0
    # a second move: re-fitted from the re-fitted tree, measured against the last FULL build
    before = len(r.ctx.calls)
    _move(scene, 0.6)
    r.update(scene, cam)
    assert _names(r.ctx.calls[before:]) == ["upload_triangles", "device_refit_bvh", "upload_bvh", "upload_materials"] and builds == [1998]
    again = rr.refit_vectorised(want, scene.content.triangles)
    assert scene.content.nodes.tobytes() == again.tobytes() == rr.refit_vectorised(first, scene.content.triangles).tobytes()
    assert r.lastRefitCostRatio == rr.bvh_cost(again) / rr.bvh_cost(first) > 1.0


def test_python_refit_falls_back_to_a_rebuild_when_the_count_changed(monkeypatch, built):
    r, scene, cam, builds = _setup(monkeypatch)
    before = len(r.ctx.calls)
    _move(scene, 0.3, fewer=True)
    r.update(scene, cam)
    assert _names(r.ctx.calls[before:]) == ["upload_bvh", "upload_triangles", "upload_materials"]
    assert builds == [1998, 1997] and r.lastRefitCostRatio is None and r.lastRefitMs is None and r._trianglesUploaded == 1997
    assert len(scene.content.nodes) == 2 * 1997 - 1
    # the next move of the smaller scene is re-fitted again, against the new build
    built_nodes = scene.content.nodes
    moved = scenes.Scene(scene.content.positions + 0.125, scene.content.normals, scene.content.material_index, scene.content.materials)
    scene.content, scene.needsUpdate = moved, True
    before = len(r.ctx.calls)
    r.update(scene, cam)
    assert _names(r.ctx.calls[before:]) == ["upload_triangles", "device_refit_bvh", "upload_bvh", "upload_materials"] and builds == [1998, 1997]
    assert r.lastRefitCostRatio == rr.bvh_cost(scene.content.nodes) / rr.bvh_cost(built_nodes)


def test_python_refit_rebuilds_above_the_cost_limit(monkeypatch, built):
    r, scene, cam, builds = _setup(monkeypatch)
    r.refitCostLimit = 1.0
    before = len(r.ctx.calls)
    _move(scene, 0.6)
    r.update(scene, cam)
    assert _names(r.ctx.calls[before:]) == ["upload_triangles", "device_refit_bvh", "upload_bvh", "upload_triangles", "upload_materials"]
    assert builds == [1998, 1998] and r.lastRefitCostRatio > 1.0 and r.lastRefitMs == 0.125
    assert scene.content.nodes.tobytes() == capi.host_build_bvh_f64(scene.content.positions).tobytes()


def test_python_without_the_switch_sends_what_it_sent(monkeypatch, built):
    r, scene, cam, builds = _setup(monkeypatch, refit=False)
    before = len(r.ctx.calls)
    _move(scene, 0.3)
    r.update(scene, cam)
    assert _names(r.ctx.calls[before:]) == ["upload_bvh", "upload_triangles", "upload_materials"] and builds == [1998, 1998]
    assert r.lastRefitCostRatio is None and r.refit is False


def test_python_reproject_scene_goes_through_the_same_path(monkeypatch, built):
    r, scene, cam, builds = _setup(monkeypatch)
    _move(scene, 0.3)
    before = len(r.ctx.calls)
    assert r.reprojectScene(scene, RaytracingCamera(45.0, position=(0.5, 1.0, 4.0))) is True
    assert _names(r.ctx.calls[before:]) == ["keep_geometry", "upload_triangles", "device_refit_bvh", "upload_bvh", "upload_materials",
                                            "reproject_scene", "keep_geometry"]
    assert builds == [1998] and r.lastRefitCostRatio >= 1.0


NODE_SCRIPT = r"""
const pt = require(%r);
const { buildDefaultScene } = require(%r);
const out = {};
function make(refit) {
  const log = [];
  let builds = 0;
  const native = new Proxy({}, { get: (t, fn) => (...args) => { log.push([fn].concat(args.slice(1).map((a) => (ArrayBuffer.isView(a) ? a.byteLength : a))));
    if (fn === 'tileLocalRows') return 16; if (fn === 'passTimeUs') return null;
    if (fn === 'hostBuildBvhF64') { builds++; const b = Buffer.alloc(48 * (2 * args[0].length / 9 - 1)); b.writeUInt32LE(builds, 12); return b; }
    if (fn === 'deviceRefitBvh') { const b = Buffer.alloc(48 * args[1]); b.writeUInt32LE(77, 12); return { nodes: b, ms: 0.25 }; }
    if (fn === 'hostBvhCost') return args[0].readUInt32LE(12) === 77 ? 3 : 2;
    if (fn === 'hostEnvCdf') return new Float32Array(1024 * 512 * 4); return undefined; } });
  const r = new pt.Renderer({ native, handle: {}, options: { presentEveryFrame: false } });
  const { scene, camera } = buildDefaultScene(new Float32Array(1024 * 512 * 4));
  r.scalingFactor = 1;
  r.setMeanByCount();
  r.resize(16, 16);
  const defaults = [r.refit, r.refitCostLimit, r.lastRefitCostRatio, r.lastRefitMs];
  r.refit = refit;
  r.frames = 3;
  for (let i = 0; i < 3; i++) r.render(scene, camera);
  return { r, log, scene, camera, defaults, builds: () => builds };
}
const names = ['uploadBvh', 'uploadTriangles', 'uploadMaterials', 'deviceRefitBvh', 'hostBuildBvhF64', 'keepGeometry', 'reprojectScene', 'reset'];
const keep = (log) => log.filter((c) => names.includes(c[0])).map((c) => c[0]);
const box = (scene) => scene.children.find((c) => c instanceof pt.Mesh && c.geometry instanceof pt.BoxGeometry);
const step = (m, fn) => { const before = m.log.length; fn(); return { calls: keep(m.log.slice(before)), raw: m.log.slice(before), ratio: m.r.lastRefitCostRatio, ms: m.r.lastRefitMs,
  builds: m.builds(), needsUpdate: m.scene.needsUpdate, held: m.r.passes.raytrace.nodeBytes.readUInt32LE(12), nodes: m.r.passes.raytrace.stats['BVH Nodes'] }; };
const slide = (m) => { box(m.scene).position.x += 0.125; m.scene.needsUpdate = true; };
{
  const m = make(true);
  out.defaults = m.defaults.map((v) => (v === Infinity ? 'Infinity' : v));
  out.first = keep(m.log);
  out.refit = step(m, () => { slide(m); m.r.update(m.scene, m.camera); });
  out.refitArgs = out.refit.raw.filter((c) => c[0] === 'deviceRefitBvh' || c[0] === 'uploadBvh');
  out.reproject = step(m, () => { slide(m); out.reprojectOk = m.r.reprojectScene(m.scene, m.camera); });
  out.fewer = step(m, () => { m.scene.remove(m.scene.children[m.scene.children.length - 1]); m.scene.needsUpdate = true; m.r.update(m.scene, m.camera); });
  out.afterFewer = step(m, () => { slide(m); m.r.update(m.scene, m.camera); });
  m.r.refitCostLimit = 1.25;
  out.limit = step(m, () => { slide(m); m.r.update(m.scene, m.camera); });
  m.r.refitCostLimit = 1.5;
  out.atLimit = step(m, () => { slide(m); m.r.update(m.scene, m.camera); });
  out.direct = m.r.deviceRefitBvh().ms;
}
{
  const m = make(false);
  out.off = step(m, () => { slide(m); m.r.update(m.scene, m.camera); });
}
delete out.refit.raw; delete out.reproject.raw; delete out.fewer.raw; delete out.afterFewer.raw; delete out.limit.raw; delete out.atLimit.raw; delete out.off.raw;
console.log(JSON.stringify(out));
"""


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_refit_sends_the_same():
    script = NODE_SCRIPT % (JS, os.path.join(JS, "examples", "default_scene"))
    p = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    j = json.loads(p.stdout.strip().splitlines()[-1])
    assert j["defaults"] == [False, "Infinity", None, None]
    assert j["first"] == ["reset", "hostBuildBvhF64", "uploadBvh", "uploadTriangles", "uploadMaterials"]      # (resize resets)
    row = j["refit"]
    assert row["calls"] == ["uploadTriangles", "deviceRefitBvh", "uploadBvh", "uploadMaterials"]
    assert row["ratio"] == 1.5 and row["ms"] == 0.25 and row["builds"] == 1 and row["needsUpdate"] is False and row["held"] == 77 and row["nodes"] == 3995
    assert j["refitArgs"] == [["deviceRefitBvh", 3995], ["uploadBvh", 3995 * 48]]
    assert j["reprojectOk"] is True
    assert j["reproject"]["calls"] == ["keepGeometry", "uploadTriangles", "deviceRefitBvh", "uploadBvh", "uploadMaterials", "reprojectScene", "keepGeometry"]
    # the triangle count changed: today's rebuild; the move after it is re-fitted again
    row = j["fewer"]
    assert row["calls"] == ["hostBuildBvhF64", "uploadBvh", "uploadTriangles", "uploadMaterials"] and row["ratio"] is None and row["ms"] is None
    assert row["builds"] == 2 and row["held"] == 2
    assert j["afterFewer"]["calls"] == ["uploadTriangles", "deviceRefitBvh", "uploadBvh", "uploadMaterials"] and j["afterFewer"]["ratio"] == 1.5
    # above the limit: the refit is measured, then the tree is rebuilt as today
    row = j["limit"]
    assert row["calls"] == ["uploadTriangles", "deviceRefitBvh", "hostBuildBvhF64", "uploadBvh", "uploadTriangles", "uploadMaterials"]
    assert row["ratio"] == 1.5 and row["builds"] == 3 and row["held"] == 3
    assert j["atLimit"]["calls"] == ["uploadTriangles", "deviceRefitBvh", "uploadBvh", "uploadMaterials"] and j["atLimit"]["builds"] == 3
    assert j["direct"] == 0.25
    assert j["off"]["calls"] == ["hostBuildBvhF64", "uploadBvh", "uploadTriangles", "uploadMaterials"] and j["off"]["ratio"] is None


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.deviceRefitBvh, typeof n.hostBvhCost, typeof pt.Renderer.prototype.deviceRefitBvh,"
              " typeof pt.RaytracePass.prototype.refitScene].join(' '));"
              "const b = Buffer.alloc(96); b.writeFloatLE(1, 16); b.writeFloatLE(2, 20); b.writeFloatLE(3, 24); b.writeFloatLE(1, 64 + 0);"
              "b.writeFloatLE(1, 64 + 4); b.writeFloatLE(1, 64 + 8); console.log(n.hostBvhCost(b));") % (os.path.join(JS, "mi3pt.node"), JS)
    p = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert lines[0].split() == ["function"] * 4
    # a 1 x 2 x 3 root (area 22) and a unit cube (area 6): (22 + 6) / 22
    assert float(lines[1]) == (22.0 + 6.0) / 22.0
