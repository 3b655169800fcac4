"""The compressed-packet walks (kernel variants 13 and 14) on the CPU, from the bytes a context uploads: the builders held to
pt_kernels.h's contract (a decoded box contains its child's uploaded box by a whole cell on every side), the node step's box test held to
conservativeness on the real fma quotients (PROOFS.md 4: it never rejects what the reference's slab test passes), and the place where
both walks could be wrong without the suite noticing -- EMPTY child slots, which that test does not reject on micro-geometry
(tests/micro_geometry.py; PROOFS.md 4a).  tests/packet_walk_reference.py restates the node step; no device anywhere.

Accepted empty slots on the probe rays (camera 64 x 48: the whole view and the close-up of one cluster; tests/walk_probe_inputs.py's
families; 2 000 aimed rays: 19 472 rays per scene), counted by the restatement WITHOUT the 8-wide walk's occupancy mask, rays on the fma
path only, default grouping:
    scene          4-ary: rays, events     8-wide: rays, events
    dust              6 387   31 588          5 792   35 842
    collapsed         6 776   34 291          6 222  273 731
    flat dust         6 600   41 840          6 228   45 324
    tail              3 389    3 389          3 389   16 945
    dust + 0.02       1 158   10 000          1 077   41 073       (control)
    dust + 1             57      155             50      884       (control)
The controls are not at zero over ALL probe rays, and cannot be: the condition is  255 cell / |d_i| < 2^-20 x (distance to the packet),
the cell is floored at 2^-20 of the largest coordinate, so a packet one unit from the origin is accepted from beyond ~255 units -- the
aimed rays from 500 units, and the families' far origins for the 0.02 control.  What distinguishes the condition is asserted instead:
zero on the camera rays and on the aimed rays from 0.5 and 5 units (the distances the figures of the issue were measured at), and on EVERY
scene every event satisfies the stated inequality.  Rays on the plain-division path (NaN, |d_i| < 1e-6, ...) pass inverted boxes by
another route -- the reference's own slab test answers "hit" for a NaN -- on every scene with an empty slot, the demo scene included."""
import numpy as np
import pytest

import micro_geometry as mg
import packet_walk_reference as pw
import walk_probe_inputs as wpi
from mi3pt_host import capi

ORDINARY = ("demo", "tiny next to huge", wpi.TIE_SCENE)
ALL_SCENES = ORDINARY + mg.SCENES
FNV_OFFSET, FNV_PRIME = 0xcbf29ce484222325, 0x100000001b3


def fnv1a(raw):
    h = FNV_OFFSET
    for b in raw.tobytes():
        h = ((h ^ b) * FNV_PRIME) & 0xffffffffffffffff
    return h


class Case:
    """One scene: its records, its probe rays, the decoded packets per grouping and the restated walks, each computed once."""

    def __init__(self, name, orc):
        self.name, self.orc = name, orc
        if name in mg.SCENES:
            sc = mg.scene(name)
            self.nodes, self.tris, self.mats = sc.nodes, sc.triangles, sc.material_bytes
            fam = mg.probe_rays(sc, orc)
        else:
            self.nodes, self.tris, self.mats = _ordinary()[name]
            fam = wpi.scene_rays(self.nodes, self.tris)
        self.families = list(fam)
        self.rays = pw.Rays(np.concatenate([fam[k] for k in self.families]))
        self.owner = np.concatenate([np.full(len(fam[k]), i) for i, k in enumerate(self.families)])
        self._packets, self._walks, self._passes = {}, {}, None

    def packets(self, collapse=-1):
        if collapse not in self._packets:
            c4, c8 = pw.load(capi, self.nodes, self.tris, collapse)
            self._packets[collapse] = {4: (c4, pw.Grouping(self.nodes, c4)), 8: (c8, pw.Grouping(self.nodes, c8))}
        return self._packets[collapse]

    def walk(self, W, collapse=-1, masked=False):
        key = (W, collapse, masked)
        if key not in self._walks:
            self._walks[key] = pw.walk(self.packets(collapse)[W][0], self.rays, len(self.tris), self.orc, apply_occupancy=masked)
        return self._walks[key]

    def passes(self):
        if self._passes is None:
            self._passes = pw.leaves_passing(self.orc, self.nodes, self.rays.rays)
        return self._passes

    def family(self, name):
        return self.owner == self.families.index(name)


_ordinary_cache, _cases = {}, {}


def _ordinary():
    if not _ordinary_cache:
        _ordinary_cache.update({k: v for k, v in wpi.scenes().items() if k in ORDINARY})
    return _ordinary_cache


@pytest.fixture
def case(orc, request):
    name = request.param
    if name not in _cases:
        _cases[name] = Case(name, orc)
    return _cases[name]


by_scene = pytest.mark.parametrize("case", ALL_SCENES, indirect=True)


# ---------------------------------------------------------------- part 1: the bytes are the ones a context uploads

def test_walk_buffers_hash_to_the_scene_compile_digests(built):
    seen = set()
    for name in ("demo", "tail", "collapsed"):
        nodes, tris = (_ordinary()[name][:2] if name == "demo" else (mg.scene(name).nodes, mg.scene(name).triangles))
        for collapse, order in ((-1, 0), (0, 0), (1, 1), (1, 2)):
            digests = capi.host_scene_compile(nodes, tris, collapse, order, True)
            assert digests["cwide_ok"] == 1 and digests["cw8_ok"] == 1
            for kind in (capi.WALK_WIDE, capi.WALK_CWIDE, capi.WALK_TRI64, capi.WALK_CW8, capi.WALK_TRI8):
                raw = capi.host_walk_buffer(nodes, tris, kind, collapse, order)
                assert len(raw) > 0 and raw.shape[1] == capi.WALK_RECORD_BYTES[kind]
                assert fnv1a(raw) == digests[capi.WALK_DIGEST_FIELD[kind]], (name, collapse, order, kind)
                seen.add(kind)
            assert len(capi.host_walk_buffer(nodes, tris, capi.WALK_CW8, collapse, order)) == digests["cw8_packets"]
            assert len(capi.host_walk_buffer(nodes, tris, capi.WALK_TRI8, collapse, order)) == digests["cw8_records"]
            assert len(capi.host_walk_buffer(nodes, tris, capi.WALK_CULL, collapse, order)) == digests["packets"]
    assert len(seen) == 5
    broken = wpi.broken_boxes(_ordinary()["demo"][0])          # boxes that do not nest: no compressed packets, and the call says so with 0 bytes
    assert len(capi.host_walk_buffer(broken, _ordinary()["demo"][1], capi.WALK_CWIDE)) == 0
    with pytest.raises(capi.Mi3ptError, match="bad argument"):
        capi.host_walk_buffer(_ordinary()["demo"][0], _ordinary()["demo"][1], 6)


# ---------------------------------------------------------------- part 2: the restatement's own arithmetic

def test_the_float64_fma_rounds_once_or_is_recomputed_exactly():
    """fma32 forms q B + A in float64 and rounds to float32: safe unless the inexact float64 sum sits exactly half way between two float32
    values.  On a million operand triples of the node step's kind (q an 8-bit index, B a cell quotient far below A, A a distance) and a
    million of cwide_hit's kind (key x (1 - 2^-20) - f with key ~ f): the detector flags at most a handful, and on every flagged triple and
    on 2 000 others the result equals the exact sum, rounded once, computed with fractions."""
    from fractions import Fraction
    rng = np.random.default_rng(41)
    n = 1_000_000
    q = rng.integers(0, 256, n).astype(np.float32)
    A = (rng.normal(size=n) * 10 ** rng.uniform(-3, 3, n)).astype(np.float32)
    B = (np.abs(A) * 2.0 ** rng.uniform(-40, 2, n) * rng.choice([-1, 1], n)).astype(np.float32)
    key = np.abs(A)
    f = (key * (1 + rng.integers(-40, 41, n) * 2.0 ** -24)).astype(np.float32)
    for a, b, c in ((q, B, A), (key, np.full(n, pw.SHRINK), -f)):
        r, flagged = pw.fma32_flagged(a, b, c)
        assert flagged.sum() <= 16, int(flagged.sum())
        got = pw.fma32(a, b, c)
        pick = np.union1d(np.flatnonzero(flagged), rng.integers(0, n, 2000))
        for i in pick:
            want = pw._round_f32_exact(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
            assert got[i] == want, (a[i], b[i], c[i], got[i], want)
    # the half-way case itself: (2^-12 + 2^-30)(2^-12 - 2^-30) + (1 + 2^-23) = 1 + 2^-23 + 2^-24 - 2^-60 rounds DOWN once, but UP (a tie,
    # to even) when float64 has dropped the 2^-60 first
    a, b, c = (np.array([v], np.float32) for v in (2.0 ** -12 + 2.0 ** -30, 2.0 ** -12 - 2.0 ** -30, 1 + 2.0 ** -23))
    r, flagged = pw.fma32_flagged(a, b, c)
    assert flagged[0] and r[0] == np.float32(1 + 2.0 ** -22) and pw.fma32(a, b, c)[0] == np.float32(1 + 2.0 ** -23)
    # cwide_hit's conventions: tfar < 0 rejects, equality passes, a product that only just exceeds tfar rejects
    one = np.float32(1.0)
    assert pw.cwide_hit(np.array([one]), np.array([one]))[0] and not pw.cwide_hit(np.array([one]), np.array([-one]))[0]
    assert pw.cwide_hit(np.array([one]), np.array([pw.SHRINK]))[0] and not pw.cwide_hit(np.array([one]), np.array([np.nextafter(pw.SHRINK, np.float32(0))]))[0]


# ---------------------------------------------------------------- containment: the builders against pt_kernels.h's contract

@by_scene
@pytest.mark.parametrize("collapse", [-1, 0], ids=["default grouping", "greedy grouping"])
def test_decoded_boxes_contain_the_uploaded_child_boxes_by_a_whole_cell(case, collapse):
    for W, (P, G) in case.packets(collapse).items():
        assert (P.marked_empty == (P.kind == 0)).all(), f"{W}-ary: a slot without a child whose box is not (255, 0), or the reverse"
        ok = pw.containment(case.nodes, P, G)
        assert len(ok) and ok.all(), f"{W}-ary: {int((~ok).sum())} of {ok.size} decoded planes lie less than a whole cell outside their child's"
        # ... and the kernel's own decode (one float32 fma per plane) still contains it
        lo32, hi32 = P.box32()
        occ = P.kind != 0
        nd = np.where(occ, G.slot_node, 0)
        assert (lo32[occ] <= case.nodes["min"][nd][occ]).all() and (hi32[occ] >= case.nodes["max"][nd][occ]).all()
        assert (P.qlo[occ] < P.qhi[occ]).all() and P.qhi[occ].max() <= 254
        if W == 4:
            assert (P.nchild == occ.sum(1)).all()


# ---------------------------------------------------------------- conservativeness, as a property

@by_scene
def test_no_ancestor_slot_rejects_a_leaf_whose_own_box_the_reference_passes(case, orc):
    passes = case.passes()
    # (every box nested: the leaves whose own box passes are the triangles the reference tests -- the oracle's own count, ray by ray)
    _, cnt = orc.ray_scene_n(orc.OracleScene(case.tris, case.mats, case.nodes), case.rays.rays)
    assert (cnt[:, 2] == 0).all() and (passes.sum(1) == cnt[:, 1]).all()
    assert passes.any()
    for W in (4, 8):
        for masked in ((False, True) if W == 8 else (False,)):
            reached = case.walk(W, masked=masked).reached
            lost = passes & ~reached
            assert not lost.any(), f"{case.name}, {W}-ary walk: ray {np.argwhere(lost)[0].tolist()[0]} never reaches triangle {np.argwhere(lost)[0].tolist()[1]}, whose box the reference passes"
    if case.name in ("demo", "tail"):
        reached = pw.walk(case.packets(0)[8][0], case.rays, len(case.tris), orc, apply_occupancy=True).reached      # the greedy grouping
        assert not (passes & ~reached).any()


# ---------------------------------------------------------------- the condition on the inputs

def _events(case, W, collapse=-1):
    """(accepted empty slots per ray, with the rays of the plain-division path zeroed; the walk)"""
    res = case.walk(W, collapse)
    return np.where(case.rays.slow, 0, res.empty), res


@pytest.mark.parametrize("case", mg.SCENES, indirect=True)
def test_micro_scenes_put_rays_into_empty_slots_and_the_controls_do_not(case):
    """the counts: this module's docstring"""
    n = len(case.rays.rays)
    aimed, closeup = case.family("aimed into the clusters"), case.family("camera 64 x 48, close-up")
    camera = case.family("camera 64 x 48") | closeup
    radius = np.arange(int(aimed.sum())) % 3            # micro_geometry.aimed_rays: 0.5, 5, 500 in turn
    near = np.zeros(n, bool)
    near[np.flatnonzero(aimed)[radius < 2]] = True
    for W in (4, 8):
        ev, res = _events(case, W)
        rays_with, events = int((ev > 0).sum()), int(ev.sum())
        print(f"{case.name}, {W}-ary: {rays_with} of {n} rays accept an empty slot, {events} times")
        if case.name in mg.CONTROLS:
            assert ev[near].sum() == 0 and ev[camera].sum() == 0, (W, int(ev[near].sum()), int(ev[camera].sum()))
        else:
            assert rays_with >= 0.01 * n and events >= 100, (W, rays_with, events)
            assert ev[near].sum() >= 100
            assert (ev[closeup] > 0).sum() >= 0.1 * closeup.sum()          # the view tests/test_gpu_micro_geometry.py renders: 563 of its 3 072 rays
        # every event is the stated condition at work: on every axis 255 cells are below 2^-19 of the entry distance (2^-20 of
        # cwide_hit's band + one rounding of the fma) -- a packet is only ever accepted from far enough away
        P = case.packets()[W][0]
        R = case.rays
        for p, s, hit in res.events:
            k = hit[~R.slow[hit]]
            if len(k) == 0:
                continue
            with np.errstate(all="ignore"):
                A = ((P.origin[p][None, :] - R.o[k]).astype(np.float32) * R.inv[k]).astype(np.float32)
                B = (P.cell32()[p][None, :] * R.inv[k]).astype(np.float32)
            assert (255.0 * np.abs(B.astype(np.float64)) <= 2.0 ** -19 * np.abs(A.astype(np.float64)).max(1, keepdims=True)).all(), (case.name, W, p, s)


# ---------------------------------------------------------------- the 8-wide walk with its occupancy mask

def check_record_indices(P, G, apply_occupancy=True):
    """Every record index the 8-wide triangle step can form -- base + slot for the slots of (occupancy & ~internal); without the kernel's
    mask: of ~internal, any of which the box test can set -- lies inside the records, is formed once, and names the triangle of the leaf
    that sits in that slot of that packet."""
    seen = {}
    for p in range(len(P.kind)):
        slots = (int(P.occupancy[p]) if apply_occupancy else 0xff) & ~int(P.imask[p]) & 0xff
        for s in range(8):
            if not (slots >> s) & 1:
                continue
            i = int(P.rec_index[p, s])
            assert i < len(P.records), f"packet {p} slot {s}: record {i} of {len(P.records)}"
            assert G.slot_node[p, s] >= 0, f"packet {p} slot {s}: an empty slot's record index ({i}) can be formed"
            assert i not in seen, f"record {i}: packet {p} slot {s} and packet {seen[i][0]} slot {seen[i][1]}"
            seen[i] = (p, s)
            assert not pw.record_is_inert(P.records, i)
            assert G.leaf_of_tri[int(P.rec_tri[p, s])] == G.slot_node[p, s]
    assert len(seen) == G.nleaves


@by_scene
@pytest.mark.parametrize("collapse", [-1, 0], ids=["default grouping", "greedy grouping"])
def test_eight_wide_occupancy_mask_keeps_every_ray_and_every_index_out_of_empty_slots(case, orc, collapse):
    P, G = case.packets(collapse)[8]
    bit = 1 << np.arange(8)
    assert (((P.occupancy[:, None] & bit) != 0) == ~P.marked_empty).all(), "CW8Packet::tri bits 24-31 are not the non-empty slots"
    assert ((P.imask & ~P.occupancy) == 0).all()
    assert (P.rec_base + 7 < len(P.records)).all() and (P.rec_base[(P.kind == 2).any(1)] >= 1).all()
    for i in list(range(8)) + list(range(len(P.records) - 8, len(P.records))):
        assert pw.record_is_inert(P.records, i)
    check_record_indices(P, G, apply_occupancy=True)
    res = case.walk(8, collapse, masked=True) if collapse == -1 else pw.walk(P, case.rays, len(case.tris), orc, apply_occupancy=True)
    assert res.empty.sum() == 0 and not res.events
    for p, s, i in res.records:
        assert G.slot_node[p, s] >= 0 and i < len(P.records)


@pytest.mark.parametrize("case", [s for s in mg.SCENES if s not in mg.CONTROLS], indirect=True)
def test_without_the_mask_the_restated_eight_wide_walk_does_enter_empty_slots(case):
    """what the mask is for, on the host restatement alone: with the kernel's AND taken out the same packets send rays into empty slots
    and form record indices that belong to no slot of their packet"""
    P, G = case.packets()[8]
    res = case.walk(8, masked=False)
    assert res.empty.sum() >= 100
    assert any(G.slot_node[p, s] < 0 for p, s, _ in res.records)
    with pytest.raises(AssertionError, match="an empty slot's record index"):
        check_record_indices(P, G, apply_occupancy=False)


@by_scene
def test_eight_wide_host_check_passes_with_both_groupings(case):
    for greedy in (False, True):
        r = capi.host_eight_wide_check(case.nodes, case.tris, greedy)
        assert r["leaves"] == len(case.tris) and r["offered"]
        raw = capi.host_walk_buffer(case.nodes, case.tris, capi.WALK_TRI8, 0 if greedy else -1)
        assert r["records"] == len(raw)


def test_tail_scene_ends_the_records_behind_a_micro_packet_with_leaves_in_its_lowest_slots(built):
    """build_cw8's past-the-end case, read from the bytes: the LAST packet that owns records is the micro cluster at the origin, its three
    leaves sit in slots 0 .. 2, and slots 3 .. 7 index records behind its last one -- the eight inert tail records, nothing else"""
    sc = mg.scene("tail")
    for collapse in (-1, 0):
        c4, P = pw.load(capi, sc.nodes, sc.triangles, collapse)
        owners = np.flatnonzero((P.kind == 2).any(1))
        last = int(owners[np.argmax(P.rec_base[owners])])
        assert last == len(P.kind) - 1
        assert (P.kind[last] == [2, 2, 2, 0, 0, 0, 0, 0]).all() and P.occupancy[last] == 0b111 and P.imask[last] == 0
        assert sorted(P.tri[last, :3].tolist()) == [14, 15, 16]
        lo, hi = P.box64()
        assert np.abs(lo[last, :3]).max() < 1e-7 and np.abs(hi[last, :3]).max() < 1e-7
        assert P.rec_base[last] + 3 == len(P.records) - 8
        for s in range(3, 8):
            assert pw.record_is_inert(P.records, int(P.rec_index[last, s]))
