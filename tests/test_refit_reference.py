"""The refit law on the CPU (tests/refit_reference.py against itself, against the host builder, and mi3pt_host_bvh_cost against the Python
figure).  The property the law is chosen for: re-fitting an unchanged scene gives the host-built records back bit for bit."""
import functools
import struct

import numpy as np
import pytest

import refit_reference as rr
from mi3pt_host import capi, layout, scenes

F = np.float32
PZ, NZ = F(0.0), F(-0.0)


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _scene_of(pos):
    n = len(pos)
    return scenes.Scene(np.asarray(pos, np.float64), np.tile([0.0, 0.0, 1.0], (n, 3, 1)), np.zeros(n, int), [scenes.WHITE])


def zero_case():
    """eight triangles whose x coordinates run through every pattern of +0 / -0 over (a, b, c): zeros of both signs inside a leaf and on
    both sides of the unions above it.  (nodes, triangles)"""
    rng = np.random.default_rng(5)
    pos = rng.normal(size=(8, 3, 3))
    for t in range(8):
        for v in range(3):
            pos[t, v, 0] = -0.0 if (t >> v) & 1 else 0.0
    sc = _scene_of(pos)
    sc.build_bvh()
    return sc.nodes, sc.triangles


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (tree as uploaded, triangles as they stand now)"""
    demo = scenes.demo_scene()
    demo.build_bvh()
    moved = rr.moved_demo()
    out = {"demo unchanged": (demo.nodes, demo.triangles), "demo moved": (demo.nodes, moved.triangles), "chain": rr.chain(),
           "zeros": zero_case()}
    for n in (1, 2):
        sc = _scene_of(np.random.default_rng(n).normal(size=(n, 3, 3)))
        sc.build_bvh()
        out[f"{n} triangle(s)"] = (sc.nodes, sc.triangles)
    nan = moved.triangles.copy()
    nan["bPosition"][5] = np.nan                   # one vertex
    nan["aPosition"][40], nan["bPosition"][40], nan["cPosition"][40] = np.nan, np.nan, np.nan
    out["non-finite"] = (demo.nodes, nan)
    return out


NAMES = ("demo unchanged", "demo moved", "chain", "zeros", "1 triangle(s)", "2 triangle(s)", "non-finite")


@pytest.mark.parametrize("name", NAMES)
def test_scalar_and_vectorised_agree(built, name):
    nodes, tris = cases()[name]
    a, b = rr.refit_scalar(nodes, tris), rr.refit_vectorised(nodes, tris)
    assert rr.first_difference(a, b) is None, rr.first_difference(a, b)
    # words 3 and 7 .. 11 are the uploaded record's
    w0 = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1).view("<u4").reshape(-1, 12)
    w1 = a.view(np.uint8).reshape(-1).view("<u4").reshape(-1, 12)
    assert (w0[:, [3, 7, 8, 9, 10, 11]] == w1[:, [3, 7, 8, 9, 10, 11]]).all()


def test_unchanged_demo_scene_gives_the_host_built_records_back(built):
    nodes, tris = cases()["demo unchanged"]
    assert len(nodes) == 3995
    for fn in (rr.refit_scalar, rr.refit_vectorised):
        got = fn(nodes, tris)
        assert got.tobytes() == np.ascontiguousarray(nodes).tobytes(), rr.first_difference(got, nodes)
    # ... and it would not, had a leaf read another triangle or had a word not been carried
    wrong = tris.copy()
    wrong[[3, 4]] = wrong[[4, 3]]
    assert rr.refit_vectorised(nodes, wrong).tobytes() != np.ascontiguousarray(nodes).tobytes()


def test_lo_and_hi_on_zeros_and_a_nan():
    for x, y in ((PZ, NZ), (NZ, PZ)):
        assert _bits(rr.lo(x, y)) == 0x80000000 and _bits(rr.hi(x, y)) == 0
        assert _bits(rr.lo_v(np.array([x]), np.array([y]))[0]) == 0x80000000 and _bits(rr.hi_v(np.array([x]), np.array([y]))[0]) == 0
    assert _bits(rr.lo(PZ, PZ)) == 0 and _bits(rr.hi(NZ, NZ)) == 0x80000000
    nan = F(np.nan)
    for f, fv in ((rr.lo, rr.lo_v), (rr.hi, rr.hi_v)):
        assert f(F(1.0), nan) == 1.0 and np.isnan(f(nan, F(1.0)))                  # a NaN y is dropped, a NaN x is kept
        assert fv(np.array([F(1.0)]), np.array([nan]))[0] == 1.0 and np.isnan(fv(np.array([nan]), np.array([F(1.0)]))[0])
    # in a tree: a leaf of mixed zeros spans [-0, +0]; a union of a +0 leaf and a -0 leaf does too, whichever is left
    nodes, tris = cases()["zeros"]
    got = rr.refit_scalar(nodes, tris)
    x_min = got["min"][:, 0].view("<u4")
    x_max = got["max"][:, 0].view("<u4")
    leaf = got["isLeaf"] == 1
    t = got["triangleIndex"][leaf]
    assert (x_min[leaf] == np.where(t == 0, 0, 0x80000000)).all() and (x_max[leaf] == np.where(t == 7, 0x80000000, 0)).all()
    assert (x_min[~leaf] == 0x80000000).all() and (x_max[~leaf] == 0).all()
    both = [(int(l), int(r)) for l, r in zip(got["left"][~leaf], got["right"][~leaf])]
    assert any(x_min[l] == 0 and x_min[r] == 0x80000000 for l, r in both) or any(x_min[l] == 0x80000000 and x_min[r] == 0 for l, r in both)


@pytest.mark.parametrize("name", ("demo moved", "chain", "zeros"))
def test_boxes_contain_what_is_below_them(built, name):
    nodes, tris = cases()[name]
    got = rr.refit_vectorised(nodes, tris)
    leaf = got["isLeaf"] == 1
    t = np.ascontiguousarray(tris).view(np.uint8).reshape(-1).view(layout.TRIANGLE)[got["triangleIndex"][leaf]]
    for v in ("aPosition", "bPosition", "cPosition"):
        assert (got["min"][leaf] <= t[v]).all() and (t[v] <= got["max"][leaf]).all()
    stacked = np.stack([t["aPosition"], t["bPosition"], t["cPosition"]])
    assert (got["min"][leaf] == stacked.min(0)).all() and (got["max"][leaf] == stacked.max(0)).all()          # tight, as values
    l, r = got["left"][~leaf], got["right"][~leaf]
    for c in (l, r):
        assert (got["min"][~leaf] <= got["min"][c]).all() and (got["max"][c] <= got["max"][~leaf]).all()
    # word-exactly: every bound of a parent is the bound of one of its two children
    u = lambda a: a.view("<u4")
    assert ((u(got["min"][~leaf]) == u(got["min"][l])) | (u(got["min"][~leaf]) == u(got["min"][r]))).all()
    assert ((u(got["max"][~leaf]) == u(got["max"][l])) | (u(got["max"][~leaf]) == u(got["max"][r]))).all()


@pytest.mark.parametrize("name", ("demo unchanged", "demo moved", "chain"))
def test_host_bvh_cost_is_the_python_figure(built, name):
    nodes, tris = cases()[name]
    tree = rr.refit_vectorised(nodes, tris)
    got, want = capi.host_bvh_cost(tree), rr.bvh_cost(tree)
    assert struct.pack("<d", got) == struct.pack("<d", want), (got, want)
    assert got > 1.0                               # the root itself counts


def test_host_bvh_cost_edges(built):
    nodes, tris = cases()["demo unchanged"]
    flat = np.zeros(3, layout.BVH_NODE)             # a root without area
    flat["max"][:, 0] = 1.0
    assert capi.host_bvh_cost(flat) == 0.0 and rr.bvh_cost(flat) == 0.0
    moved = rr.refit_vectorised(nodes, cases()["demo moved"][1])
    assert capi.host_bvh_cost(moved) / capi.host_bvh_cost(nodes) > 1.0     # the box left the place its subtree was built for
