"""First-hit feature images (mi3pt_render_aovs), host side -- no GPU: the C ABI's declarations and exports, the argument checks
that need no device, both hosts' surface, and the reference helper (tests/aov_reference.py) against itself."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import aov_reference as ar
import ptcommon as pc
from mi3pt_host import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "webgpu-pathtracer_amd", "js")
NAMES = ("mi3pt_render_aovs", "mi3pt_read_aov", "mi3pt_aov_device_ptr")


def _header():
    return open(os.path.join(ROOT, "include", "mi3pt.h")).read()


def test_header_declares_the_enum_and_the_three_functions():
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"typedef\s+enum\s+mi3pt_aov\s*\{(.*?)\}\s*mi3pt_aov\s*;", hdr, flags=re.S)
    assert m, "enum mi3pt_aov"
    values = dict((k, int(v)) for k, v in re.findall(r"(MI3PT_AOV_\w+)\s*=\s*(\d+)", m.group(1)))
    assert values == {"MI3PT_AOV_ALBEDO": 0, "MI3PT_AOV_NORMAL": 1, "MI3PT_AOV_POSITION": 2, "MI3PT_AOV_IDS": 3, "MI3PT_AOV_COUNT": 4}
    assert re.search(r"int\s+mi3pt_render_aovs\s*\(\s*mi3pt_ctx\s*\*\s*ctx\s*,\s*unsigned\s+aov_mask\s*\)\s*;", hdr)
    assert re.search(r"int\s+mi3pt_read_aov\s*\(\s*mi3pt_ctx\s*\*\s*ctx\s*,\s*int\s+which\s*,\s*void\s*\*\s*dst\s*,\s*size_t\s+nbytes\s*\)\s*;", hdr)
    assert re.search(r"int\s+mi3pt_aov_device_ptr\s*\(\s*mi3pt_ctx\s*\*\s*ctx\s*,\s*int\s+which\s*,\s*void\s*\*\*\s*dev_ptr\s*,\s*size_t\s*\*\s*nbytes\s*\)\s*;", hdr)
    assert re.search(r"MI3PT_PASS_AOV\s*=\s*3\b", hdr)
    assert re.search(r"#define\s+MI3PT_ABI_VERSION\s+4\b", hdr)


def test_python_host_has_the_constants_and_methods():
    assert (capi.AOV_ALBEDO, capi.AOV_NORMAL, capi.AOV_POSITION, capi.AOV_IDS, capi.AOV_COUNT) == (0, 1, 2, 3, 4)
    assert capi.PASS_AOV == 3 and capi.AOV_ALL == 15
    for n in NAMES:
        assert n in capi.SYMBOLS
    for m in ("render_aovs", "read_aov", "aov_device_ptr"):
        assert callable(getattr(capi.Context, m))
    from mi3pt_host import renderer
    assert callable(renderer.Renderer.renderAovs) and callable(renderer.Renderer.readAov)


def test_library_exports_the_symbols_and_refuses_a_null_context(built):
    lib = capi.load_library()
    assert lib.mi3pt_abi_version() == 4
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (mi3pt_\w+)", out))
    assert set(NAMES) <= exported
    lib.mi3pt_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_uint8 * 16)()
    ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
    calls = (lambda: lib.mi3pt_render_aovs(None, 15),
             lambda: lib.mi3pt_read_aov(None, 0, buf, 16),
             lambda: lib.mi3pt_aov_device_ptr(None, 0, ctypes.byref(ptr), ctypes.byref(n)))
    for call in calls:
        lib.mi3pt_abi_version()
        assert call() == 1                                   # MI3PT_ERR_INVALID
        assert b"null" in lib.mi3pt_last_error()


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_addon_under_node_has_the_entry_points(built):
    script = ("const n = require(%r); const pt = require(%r);"
              "console.log([typeof n.renderAovs, typeof n.readAov, typeof pt.Renderer.prototype.renderAovs,"
              " typeof pt.Renderer.prototype.readAov, pt.AOV_NAMES.join(',')].join(' '));") % (os.path.join(JS, "mi3pt.node"), JS)
    r = subprocess.run([shutil.which("node"), "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["function", "function", "function", "function", "albedo,normal,position,ids"]
    dts = open(os.path.join(JS, "index.d.ts")).read()
    assert "renderAovs(" in dts and "readAov(" in dts
    assert "--aovs" in open(os.path.join(JS, "tools", "render_demo.js")).read()


def _shares(ref):
    inside = ref["computed"] & ref["inside"]
    n = int(inside.sum())
    hits = int((ref["hit"] & inside).sum())
    return n, hits, n - hits


def test_helper_meets_the_input_conditions_of_the_demo_scene(orc, demo):
    """Properties of the inputs, measured on the oracle alone: the whole-image demo cases are neither all hits nor all misses, both
    materials occur, the miss values are the contract's."""
    osc = pc.oracle_scene(orc, demo)
    for w, h, want_hits in ((64, 64, 2431), (100, 52, 4202)):
        ref = ar.reference(orc, osc, pc.rt_uniforms(demo, w, h).tobytes(), w, h)
        n, hits, misses = _shares(ref)
        print(f"demo {w}x{h}: {n} texels, {hits} hits")
        assert n == w * h and ref["computed"].all()
        assert hits >= 0.15 * n and misses >= 0.15 * n
        assert hits == want_hits
        assert set(np.unique(ref["ids"][..., 1][ref["hit"]])) == {0, 1}
        miss = ~ref["hit"]
        assert (ref["albedo"][miss] == 0).all() and (ref["normal"][miss] == 0).all()
        assert (ref["position"][miss] == np.array([0, 0, 0, 1e20], np.float32)).all()
        assert (ref["ids"][miss] == np.array([-1, -1, 0, 0])).all()
        assert (ref["albedo"][ref["hit"]][:, 3] == 1).all() and (ref["normal"][ref["hit"]][:, 3] == 0).all()
        nn = np.linalg.norm(ref["normal"][ref["hit"]][:, :3].astype(np.float64), axis=1)
        assert np.abs(nn - 1).max() < 1e-5
    # a fractional resolution: texels outside hold the miss values
    w = h = 64
    ref = ar.reference(orc, osc, pc.rt_uniforms(demo, w, h, res=(31.75, 47.5)).tobytes(), w, h)
    n, hits, misses = _shares(ref)
    print(f"demo 64x64, resolution (31.75, 47.5): {n} inside, {hits} hits")
    assert n == 31 * 47 == 1457 and hits == 874 and hits >= 0.15 * n and misses >= 0.15 * n
    assert not ref["hit"][~ref["inside"]].any() and (ref["position"][~ref["inside"]] == np.array([0, 0, 0, 1e20], np.float32)).all()


@pytest.mark.parametrize("nranks,block_rows", [(2, 8), (3, 8), (3, 4)])
def test_helper_agrees_with_itself_across_a_tile_split(orc, demo, nranks, block_rows):
    w, h = 100, 52
    osc = pc.oracle_scene(orc, demo)
    u = pc.rt_uniforms(demo, w, h).tobytes()
    whole = ar.reference(orc, osc, u, w, h)
    seen = np.zeros(h, int)
    for rank in range(nranks):
        part = ar.reference(orc, osc, u, w, h, rank, nranks, block_rows)
        rows = capi.tile_local_rows(h, rank, nranks, block_rows)
        assert part["albedo"].shape == (rows, w, 4)
        for ly in range(rows):
            gy = capi.tile_global_row(ly, rank, nranks, block_rows)
            seen[gy] += 1
            for name in ("albedo", "normal", "position", "ids"):
                assert part[name][ly].tobytes() == whole[name][gy].tobytes(), f"{name}: rank {rank} row {ly} = image row {gy}"
    assert (seen == 1).all()


def test_single_triangle_condition_identifies_one_triangle(orc, demo):
    """check_ids' condition on oracle data alone: for sampled hit texels of the demo scene exactly one triangle reproduces the record."""
    w = h = 32
    osc = pc.oracle_scene(orc, demo)
    u = pc.rt_uniforms(demo, w, h).tobytes()
    ref = ar.reference(orc, osc, u, w, h)
    hits = np.argwhere(ref["hit"])[::97]
    assert len(hits) >= 4
    ntris = len(demo.triangles.tobytes()) // 112
    for ly, x in hits:
        meets = [t for t in range(ntris) if ar.triangle_matches(orc, osc, u, int(x), int(ly), t)[0]]
        assert len(meets) == 1
