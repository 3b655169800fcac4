"""Which kernel a raytrace launch runs (csrc/pt_host_route.cpp: raytrace_route, through its host-only entry point mi3pt_host_route)
against tests/golden/route_table.npz: for every launch of tests/route_table.py's table -- which kernel, the packing limits' edges, how
many blocks -- what THE COMMIT BEFORE THE DECISION MOVED OUT OF pt_kernels.hip reported (raytrace_route) and what it launched
(launch_raytrace_setup, launch_raytrace: the k_raytrace_sm instantiation, the grid), recorded from that commit's own functions
(profiles/route_move_record.py, profiles/route_move.log).  Every field must be equal.  No GPU needed."""
import os

import numpy as np
import pytest

import route_table
from mi3pt_host import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "route_table.npz")
OUT = {name: k for k, name in enumerate(capi.ROUTE_OUTPUTS)}
BUILD = slice(OUT["build_defer"], OUT["build_w8"] + 1)


@pytest.fixture(scope="module")
def table(built):
    with np.load(GOLDEN) as z:
        golden = {k: z[k] for k in z.files}
    rows = golden["inputs"].T
    return rows, golden, capi.host_route(rows)


def test_the_table_is_the_generators(table):
    rows, _, _ = table
    assert np.array_equal(rows, route_table.table_rows())


def test_every_launch_routes_as_recorded(table):
    rows, golden, got = table

    def equal(what, have, want, where=slice(None)):
        have, want = have[where], want[where]
        bad = np.flatnonzero((have != want).reshape(len(have), -1).any(axis=1))
        assert not len(bad), f"{what}: {len(bad)} rows differ, first {dict(zip(capi.ROUTE_INPUTS, rows[where][bad[0]].tolist()))}: " \
                             f"{have[bad[0]].tolist()} recorded {want[bad[0]].tolist()}"

    equal("reported kind, variant, lean, blocks, waves, ymax, walk_min", got[:, :7], golden["reported"].T)
    # the instantiation: the parent's k_raytrace_sm<...> where it launched one; a build is named for every launch of kind 1, an empty tile's too
    launched = golden["launches"] > 0
    sm = got[:, OUT["kind"]] == 1
    equal("k_raytrace_sm's template arguments", got[:, BUILD], golden["build"].T, launched)
    assert not got[~sm, BUILD].any()
    # the grid: the route's blocks, in one launch of the state-machine kernel or one per frame of a per-pixel kernel; none for an empty tile
    tiles = ((rows[:, 1] + 7) // 8) * ((rows[:, 2] + 7) // 8)
    assert np.array_equal(launched, tiles > 0)
    equal("grid", got[:, OUT["blocks"]], golden["grid"], launched)
    equal("launches", np.where(tiles > 0, np.where(sm, 1, np.maximum(rows[:, 3], 1)), 0), golden["launches"])
    equal("the setup kernel runs", got[:, OUT["setup"]], golden["setup"])
    assert (got[sm, OUT["has_kernel"]] == 1).all()
    # (the table does reach every kind of answer)
    assert set(got[:, OUT["kind"]]) == {0, 1} and set(got[:, OUT["setup"]]) == {0, 1} and set(got[sm, OUT["lean"]]) == {0, 1}


def test_the_builds_of_the_table_are_the_release_list(table):
    _, _, got = table
    builds = {tuple(b) for b in got[got[:, OUT["kind"]] == 1, BUILD].tolist()}
    assert builds == set(route_table.RELEASE_BUILDS.values())
