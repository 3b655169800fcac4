"""The hosts' device-builder option without a device: what RaytracePass.updateScene sends, in which order, under options["deviceBvh"] --
also on the rebuild a refit above refitCostLimit falls back to -- with a stand-in context that answers device_build_bvh with the law's
records (tests/ploc_reference.py) and device_refit_bvh with the refit's (tests/test_refit_host.py's context); and the Node host's
reading of the two options."""
import json
import os
import shutil
import subprocess

import pytest

import lbvh_reference as lr
import ploc_reference as pr
import refit_reference as rr
import test_refit_host as trf
import test_reproject_host as trh
from mi3pt_host import capi, scenes

JS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "webgpu-pathtracer_amd", "js")
KEEP = ("upload_bvh", "upload_triangles", "upload_materials", "device_refit_bvh", "device_build_bvh")


class BuilderContext(trf.RefitContext):
    """... whose device_build_bvh answers with the named builder's records for the triangles uploaded last"""

    def __getattr__(self, name):
        record = super().__getattr__(name)
        if name != "device_build_bvh":
            return record

        def build(method="lbvh", radius=16, max_search_iterations=1024):
            record(method, radius)
            tris = [c[1] for c in self.calls if c[0] == "upload_triangles"][-1]
            if method == "lbvh":
                return lr.reference_nodes(tris), capi.BvhBuildInfo(0.5)
            nodes, searched, forced = pr.build(tris, radius, max_search_iterations)
            return nodes, capi.BvhBuildInfo(0.75, searched, forced)
        return build


def _names(calls):
    return [c[0] for c in calls if c[0] in KEEP]


def _setup(monkeypatch, options):
    builds = []
    real = capi.host_build_bvh_f64
    monkeypatch.setattr(capi, "host_build_bvh_f64", lambda pos, nthreads=0: (builds.append(len(pos)), real(pos, nthreads))[1])
    r, scene, cam, _, _ = trh._renderer(monkeypatch, BuilderContext)
    r.options.update(options)
    scene.content = scenes.demo_scene()
    r.frames = 3
    return r, scene, cam, builds


@pytest.mark.parametrize("option,radius,sent", [("ploc", None, ("ploc", 16)), ("ploc", 4, ("ploc", 4)), (True, None, ("lbvh", 16)),
                                                ("lbvh", 32, ("lbvh", 32))])
def test_python_option_builds_on_the_device_from_the_uploaded_triangles(monkeypatch, built, option, radius, sent):
    r, scene, cam, builds = _setup(monkeypatch, {"deviceBvh": option, **({"deviceBvhRadius": radius} if radius else {})})
    r.update(scene, cam)
    assert _names(r.ctx.calls) == ["upload_triangles", "device_build_bvh", "upload_bvh", "upload_materials"] and builds == []
    assert [c[1:] for c in r.ctx.calls if c[0] == "device_build_bvh"] == [sent]
    tris = scene.content.triangles
    want = pr.build(tris, sent[1])[0] if sent[0] == "ploc" else lr.reference_nodes(tris)
    uploaded = [c[1] for c in r.ctx.calls if c[0] == "upload_bvh"][0]
    assert uploaded.tobytes() == want.tobytes() and scene.content.nodes is uploaded
    assert r.lastRefitCostRatio is None and r.lastRefitMs is None


def test_python_defaults_and_a_supplied_tree_do_not_touch_the_device_builder(monkeypatch, built):
    r, scene, cam, builds = _setup(monkeypatch, {})
    r.update(scene, cam)
    assert _names(r.ctx.calls) == ["upload_bvh", "upload_triangles", "upload_materials"] and builds == [1998]
    r, scene, cam, builds = _setup(monkeypatch, {"deviceBvh": False})
    r.update(scene, cam)
    assert _names(r.ctx.calls) == ["upload_bvh", "upload_triangles", "upload_materials"] and builds == [1998]
    # a tree the content brings is uploaded as it is, whatever the option says
    r, scene, cam, builds = _setup(monkeypatch, {"deviceBvh": "ploc"})
    scene.content.build_bvh()
    mine = scene.content.nodes
    r.update(scene, cam)
    assert _names(r.ctx.calls) == ["upload_bvh", "upload_triangles", "upload_materials"] and builds == [1998]
    assert [c[1] for c in r.ctx.calls if c[0] == "upload_bvh"][0] is mine
    r, scene, cam, builds = _setup(monkeypatch, {"deviceBvh": "sah"})
    with pytest.raises(ValueError):
        r.update(scene, cam)


def test_python_refit_above_the_limit_rebuilds_through_the_device_builder(monkeypatch, built):
    r, scene, cam, builds = _setup(monkeypatch, {"deviceBvh": "ploc"})
    r.refit, r.refitCostLimit = True, 1.0
    r.update(scene, cam)
    first = scene.content.nodes
    before = len(r.ctx.calls)
    scene.content, scene.needsUpdate = rr.moved_demo(0.6, 30.0), True
    r.update(scene, cam)
    assert _names(r.ctx.calls[before:]) == ["upload_triangles", "device_refit_bvh", "upload_triangles", "device_build_bvh", "upload_bvh",
                                            "upload_materials"]
    assert builds == [] and r.lastRefitCostRatio > 1.0
    assert r.lastRefitMs == 0.75                                                      # the build's time, not the refit's 0.125
    want = pr.build(scene.content.triangles)[0]
    assert scene.content.nodes.tobytes() == want.tobytes() and len(want) == len(first)
    # the rebuilt tree is the new "last full build": the same triangles again re-fit to the ratio 1 and stay
    before = len(r.ctx.calls)
    scene.needsUpdate = True
    r.update(scene, cam)
    assert _names(r.ctx.calls[before:]) == ["upload_triangles", "device_refit_bvh", "upload_bvh", "upload_materials"]
    assert r.lastRefitCostRatio == 1.0 and r.lastRefitMs == 0.125
    # without a limit the refit is kept and no builder runs
    r.refitCostLimit = float("inf")
    before = len(r.ctx.calls)
    scene.content, scene.needsUpdate = rr.moved_demo(0.3, 10.0), True
    r.update(scene, cam)
    assert _names(r.ctx.calls[before:]) == ["upload_triangles", "device_refit_bvh", "upload_bvh", "upload_materials"]


def test_context_method_keeps_its_old_answer():
    """device_build_bvh() with no arguments returns what it always did: (nodes, milliseconds as a float)"""
    info = capi.BvhBuildInfo(1.5, 3, 2)
    assert isinstance(info, float) and info == 1.5 and info > 0 and f"{info:.2f}" == "1.50"
    assert (info.build_ms, info.search_iterations, info.forced_iterations) == (1.5, 3, 2)
    import inspect
    sig = inspect.signature(capi.Context.device_build_bvh)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("method", "lbvh"), ("radius", 16), ("max_search_iterations", 1024)]


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_host_reads_the_two_options():
    script = """
const { RaytracePass } = require(process.argv[1] + '/src/passes/raytrace');
const out = {};
const cases = { none: {}, off: { deviceBvh: false }, on: { deviceBvh: true }, lbvh: { deviceBvh: 'lbvh' }, ploc: { deviceBvh: 'ploc' },
  ploc4: { deviceBvh: 'ploc', deviceBvhRadius: 4 }, sah: { deviceBvh: 'sah' }, r0: { deviceBvh: 'ploc', deviceBvhRadius: 0 },
  r65: { deviceBvh: 'ploc', deviceBvhRadius: 65 }, rhalf: { deviceBvh: 'ploc', deviceBvhRadius: 2.5 } };
for (const [k, o] of Object.entries(cases)) { try { out[k] = RaytracePass.deviceBuilder(o); } catch (e) { out[k] = 'throws'; } }
console.log(JSON.stringify(out));
"""
    r = subprocess.run([shutil.which("node"), "-e", script, JS], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["none"] is None and j["off"] is None
    assert j["on"] == j["lbvh"] == {"method": 0, "radius": 16, "maxSearchIterations": 1024}
    assert j["ploc"] == {"method": 1, "radius": 16, "maxSearchIterations": 1024} and j["ploc4"]["radius"] == 4
    assert j["sah"] == j["r0"] == j["r65"] == j["rhalf"] == "throws"
    dts = open(os.path.join(JS, "index.d.ts")).read()
    assert "deviceBvh?: boolean | 'lbvh' | 'ploc';" in dts and "deviceBvhRadius?: number;" in dts
