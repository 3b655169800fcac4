"""mi3pt_host_freeze_tiles (plain host code in libmi3pt.so, no device) against tests/adaptive_reference.py: random and hand-made tile maps,
both guards, masks with frozen entries; the reference's own list composition, composite and loop on small hand-checked inputs."""
import ctypes

import numpy as np
import pytest

import adaptive_reference as ar
from mi3pt_host import capi

F = np.float32
T2 = lambda threshold: (F(threshold) * F(threshold)) * F(3.0)


def _random_map(rng, ty, tx, threshold):
    """sums scattered around the bound t2 x count, with the special values mixed in"""
    rec = np.zeros((ty, tx, 4), F)
    rec[..., 2] = rng.choice([0, 1, 37, 64], (ty, tx), p=[0.15, 0.05, 0.2, 0.6])
    rec[..., 3] = rng.choice([1, 15, 16, 17, 200], (ty, tx))
    bound = T2(threshold) * rec[..., 2]
    rec[..., 0] = bound * rng.choice([0, 0.5, 0.999, 1.0, 1.001, 4.0], (ty, tx)).astype(F)
    odd = rng.random((ty, tx))
    rec[..., 0] = np.where(odd < 0.05, F(np.nan), np.where(odd < 0.08, F(np.inf), rec[..., 0]))
    rec[..., 1] = rec[..., 0]
    rec[rec[..., 2] == 0] = 0
    return rec


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (7, 1), (3, 3), (6, 11)])
@pytest.mark.parametrize("guard", [0, 1])
def test_random_maps(built, shape, guard):
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + guard)
    seen = set()
    for trial in range(40):
        threshold, min_frames = (0.05, 16) if trial % 2 else (0.3, 0)
        rec = _random_map(rng, *shape, threshold)
        mask = None if trial % 3 == 0 else (rng.random(shape) < 0.7).astype(np.uint8)
        want, want_n = ar.freeze_tiles(rec, threshold, min_frames, guard, mask)
        got, got_n = capi.host_freeze_tiles(rec, threshold, min_frames, guard, mask)
        assert got.dtype == np.uint8 and got.shape == shape
        assert np.array_equal(got, want) and got_n == want_n == int(want.sum()), f"trial {trial}\n{rec[..., 0]}\n{got}\n{want}"
        if mask is not None:
            assert not got[mask == 0].any()                    # never thaws
        seen.update(np.unique(want).tolist())
    assert seen == {0, 1} or shape == (1, 1)


def _plain(ty, tx, threshold=0.1):
    """every tile well under the threshold, 64 texels, 20 frames"""
    rec = np.zeros((ty, tx, 4), F)
    rec[..., 0] = T2(threshold) * F(64) * F(0.25)
    rec[..., 2] = 64
    rec[..., 3] = 20
    return rec


def test_hand_made_maps(built):
    th, mf = 0.1, 16
    both = lambda rec, guard, mask=None: (capi.host_freeze_tiles(rec, th, mf, guard, mask), ar.freeze_tiles(rec, th, mf, guard, mask))

    def held(rec, guard, want, mask=None):
        (got, n), (ref, ref_n) = both(rec, guard, mask)
        assert np.array_equal(got, np.array(want, np.uint8)) and np.array_equal(ref, got) and n == ref_n == int(np.sum(want))

    # everything under: all frozen, with and without the ring
    for guard in (0, 1):
        held(_plain(3, 3), guard, np.zeros((3, 3)))
        held(_plain(1, 1), guard, [[0]])
    # exactly at sum_r == t2 * count: not above, frozen; one ulp more: above
    rec = _plain(1, 1)
    rec[0, 0, 0] = T2(th) * F(64)
    held(rec, 0, [[0]])
    rec[0, 0, 0] = np.nextafter(rec[0, 0, 0], F(np.inf))
    held(rec, 0, [[1]])
    # a NaN sum is above; so is a young tile (n_min < min_frames), whatever its sum
    rec = _plain(1, 3)
    rec[0, 0, 0] = np.nan
    rec[0, 2, 3] = 15
    held(rec, 0, [[1, 0, 1]])
    held(rec, 1, [[1, 1, 1]])                                  # the middle tile waits for its neighbours
    # count == 0: frozen at once, and no obstacle to its neighbours
    rec = _plain(1, 3)
    rec[0, 1] = 0
    held(rec, 1, [[0, 0, 0]])
    rec[0, 0, 0] = np.inf
    held(rec, 1, [[1, 0, 0]])                                  # (the empty tile does not pass the noise on)
    # the ring is the eight neighbours, diagonals included, and ends at the map's edge
    rec = _plain(3, 4)
    rec[0, 0, 0] = 1e9
    held(rec, 0, [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    held(rec, 1, [[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0]])
    # 1 x N
    rec = _plain(1, 5)
    rec[0, 2, 0] = 1e9
    held(rec, 1, [[0, 1, 1, 1, 0]])
    # an already frozen tile stays frozen although it reads above, and still keeps its neighbours sampling (the rule reads the verdicts)
    held(rec, 0, [[0, 0, 0, 0, 0]], mask=[[1, 1, 0, 1, 1]])
    held(rec, 1, [[0, 1, 0, 1, 0]], mask=[[1, 1, 0, 1, 1]])
    # a non-0/1 mask byte counts as sampled
    held(rec, 0, [[0, 0, 1, 0, 0]], mask=[[7, 255, 2, 1, 1]])


def test_errors(built):
    lib = capi.load_library()
    rec = _plain(2, 2)
    mask = np.ones((2, 2), np.uint8)
    n = ctypes.c_uint32()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.mi3pt_host_freeze_tiles(p(rec), 2, 2, 0.1, 16, 2, p(mask), ctypes.byref(n)) == 1
    assert lib.mi3pt_host_freeze_tiles(p(rec), 2, 2, 0.1, 16, -1, p(mask), ctypes.byref(n)) == 1
    assert lib.mi3pt_host_freeze_tiles(None, 2, 2, 0.1, 16, 1, p(mask), ctypes.byref(n)) == 1
    assert lib.mi3pt_host_freeze_tiles(p(rec), 2, 2, 0.1, 16, 1, None, ctypes.byref(n)) == 1
    assert lib.mi3pt_host_freeze_tiles(p(rec), -1, 2, 0.1, 16, 1, p(mask), ctypes.byref(n)) == 1
    assert mask.all()                                          # a refused call changes nothing
    assert lib.mi3pt_host_freeze_tiles(p(rec), 2, 2, 0.1, 16, 1, p(mask), None) == 0 and not mask.any()
    assert lib.mi3pt_host_freeze_tiles(None, 0, 0, 0.1, 16, 1, None, ctypes.byref(n)) == 0 and n.value == 0
    with pytest.raises(ValueError):
        ar.freeze_tiles(rec, 0.1, 16, 2)


def test_list_composition():
    mask = np.array([[1, 0, 1], [1, 1, 0]])
    empty = np.array([[1, 1, 0], [0, 1, 0]])
    a, s = ar.compose_lists(mask, empty)
    assert a.tolist() == [2, 3] and s.tolist() == [0, 4]
    a, s = ar.compose_lists(None, empty)
    assert a.tolist() == [2, 3, 5] and s.tolist() == [0, 1, 4]           # no mask: what the sky split lists today
    a, s = ar.compose_lists(mask, None)
    assert a.tolist() == [0, 2, 3, 4] and s.size == 0
    a, s = ar.compose_lists(np.zeros(6), empty)
    assert a.size == 0 and s.size == 0
    a, s = ar.compose_lists(empty, empty)                                # only empty tiles sampled: S alone
    assert a.size == 0 and s.tolist() == [0, 1, 4]


def test_composite_and_texels():
    snaps = [np.full((12, 20, 4), k, F) for k in range(3)]
    last = np.array([[2, 1, 0], [1, 2, 2]])
    out = ar.composite(snaps, last)
    assert out.shape == (12, 20, 4)
    assert (out[:8, :8] == 2).all() and (out[:8, 8:16] == 1).all() and (out[:8, 16:] == 0).all()
    assert (out[8:, :8] == 1).all() and (out[8:, 8:] == 2).all()
    assert ar.tile_texels([[1, 0, 1]], 5, 20).sum() == 5 * 12


def _scripted(sums):
    """tile_map_at for a 1 x 3 map whose tile sums at frames 4, 8, 12, ... are the rows of `sums`; threshold 0.1 -> bound t2 * 64"""
    def at(frames):
        rec = _plain(1, 3)
        rec[0, :, 0] = np.array(sums[frames // 4 - 1], F) * T2(0.1) * F(64)
        rec[0, :, 3] = frames
        return rec
    return at


def test_the_adaptive_loop_on_a_script():
    # multiples of the bound per tile after 4, 8, 12, 16, 20 frames; min_frames 4
    sums = [[0.5, 2.0, 3.0], [0.4, 0.9, 2.0], [9.0, 0.8, 1.5], [9.0, 0.7, 0.9], [9.0, 0.6, 0.8]]
    at = _scripted(sums)
    # immediate, no ring: tile 0 freezes at 4, tile 1 at 8, tile 2 at 16 -- its 9.0 later on is never seen: it is not sampled
    out = ar.render_until_adaptive(at, (1, 3), 0.1, 4, 40, 4, lookahead=False, guard=0)
    assert (out["converged"], out["frames"], out["sampled"]) == (True, 16, 4 * (3 + 2 + 1 + 1))
    assert [h.tolist() for h in out["history"]] == [[[0, 1, 1]], [[0, 0, 1]], [[0, 0, 1]], [[0, 0, 0]]]
    assert out["last"].tolist() == [[4, 8, 16]]
    assert out["tiles"][0, :, 3].tolist() == [4, 8, 16]
    # the ring: tile 0 waits for tile 1 (8 frames: under, but by then it reads 0.4), tile 1 for tile 2
    out = ar.render_until_adaptive(at, (1, 3), 0.1, 4, 40, 4, lookahead=False, guard=1)
    assert [h.tolist() for h in out["history"]][:2] == [[[1, 1, 1]], [[0, 1, 1]]]
    # lookahead: the decision of the estimate at 4 frames is applied after 8, so tile 0 is sampled for 8
    out = ar.render_until_adaptive(at, (1, 3), 0.1, 4, 40, 4, lookahead=True, guard=0)
    assert out["last"].tolist() == [[8, 12, 20]] and out["frames"] == 20 and out["converged"]
    assert out["sampled"] == 4 * (3 + 3 + 2 + 1 + 1)
    # the budget: not converged, the last decision (of the estimate at the budget) is not taken
    out = ar.render_until_adaptive(at, (1, 3), 0.1, 4, 12, 4, lookahead=False, guard=0)
    assert (out["converged"], out["frames"]) == (False, 12) and out["history"][-1].tolist() == [[0, 0, 1]]
