"""tests/despike_edge_cases.py without a device: the firefly pre-pass's count folded over more waves than it has slots, and its value
range -- the catalogue of means and the worked examples -- run over the numpy restatement (tests/guided_despike_reference.py) and the
scalar walk through the header's lines (tests/test_guided_despike_reference.py: _scalar_law), with the builders, sizes and seeds the GPU
tests use (tests/test_gpu_guided_despike.py) and the ORACLE's feature images where the device's own are used there
(tests/test_gpu_aov.py holds the two bit-identical).  Every condition that keeps a GPU case from passing vacuously is asserted here on
the references alone."""
import numpy as np
import pytest

import aov_reference as ar
import despike_edge_cases as de
import guided_despike_reference as dr
import guided_reference as gr
import moments_edge_cases as ec
import ptcommon as pc
import test_gpu_guided_despike as tg
from test_guided_despike_reference import _ids, _scalar_law

F = np.float32
_feat = {}


@pytest.fixture
def features(orc, demo, env):
    osc = pc.oracle_scene(orc, demo, env)

    def at(w, h):
        if (w, h) not in _feat:
            _feat[(w, h)] = ar.reference(orc, osc, pc.rt_uniforms(demo, w, h).tobytes(), w, h)
        return _feat[(w, h)]
    return at


# ---------------------------------------------------------------- the count past its slots
def test_count_slots_restates_the_launch_arithmetic():
    """96 x 48: three block columns, six block rows; a wave is two rows of a 32 x 8 tile"""
    clamped = np.zeros((48, 96), bool)
    for y, x in ((0, 0), (1, 31), (2, 0), (9, 40), (47, 95), (40, 0), (40, 1)):
        clamped[y, x] = True
    texels, waves, adding = de.count_slots(clamped)
    # (0, 0), (1, 31): block 0, wave 0; (2, 0): wave 1; (9, 40): block 1 * 3 + 1, rows 0 .. 1 of its tile: wave 16; (47, 95): block 17, wave 71 =
    # slot 7; (40, 0), (40, 1): block 15, wave 60
    assert adding.tolist() == [0, 1, 16, 60, 71] and de.launch_shape(96, 48) == (18, 72)
    want = np.zeros(64, int)
    want[[0, 1, 16, 60, 7]] = [2, 1, 1, 2, 1]
    assert texels.tolist() == want.tolist() and waves.tolist() == (want > 0).astype(int).tolist()
    clamped[0, 33] = True                                      # block 1, wave 4; and wave 68 = block 17's first wave shares its slot
    clamped[40, 64] = True
    texels, waves, _ = de.count_slots(clamped)
    assert texels[4] == 2 and waves[4] == 2
    with pytest.raises(AssertionError):
        de.assert_crosses_the_slots(clamped)


SLOT_SIZES = sorted({(w, h) for w, h, _, _ in tg.SLOT_SIZES})


@pytest.mark.parametrize("w,h", SLOT_SIZES, ids=[f"{w}x{h}" for w, h in SLOT_SIZES])
def test_the_gpu_sizes_fold_the_count_over_more_waves_than_slots(features, w, h):
    """no slot empty, eight slots and more shared by two waves, waves numbered 64 and above add, and the first 32 slots do not hold the
    whole count.  Measured: 96 x 48: 18 blocks / 72 waves, 580 clamped, 8 shared slots, 317 in slots 0 .. 31; 160 x 32: 20 / 80, 603, 16,
    367; 264 x 260: 297 / 1188, 7732, 64, 3931"""
    feat = features(w, h)
    _, s, stats = dr.despike(de.spiked_accum(feat["ids"]), feat["ids"])
    texels, waves, adding = de.assert_crosses_the_slots(s != 1)
    print(f"{w} x {h}: {de.launch_shape(w, h)} blocks / waves, {stats['count']} clamped ({stats['clamped']:.3f}), {int((texels == 0).sum())} empty slots, "
          f"{int((waves >= 2).sum())} shared by two waves and more, slots 0 .. 31 hold {int(texels[:32].sum())}")
    tg.not_vacuous(stats, w, h)
    assert de.launch_shape(w, h)[1] > de.SLOTS and stats["count"] == texels.sum()
    # nothing to clamp in the image the three-call test filters in between
    assert dr.despike(de.smooth_accum(feat["ids"]), feat["ids"])[2]["count"] == 0


def test_a_ragged_last_block_row_leaves_slots_empty(features):
    """100 x 52 is no size for the slot test: the last block row's waves 2 and 3 lie outside the image"""
    feat = features(100, 52)
    _, s, _ = dr.despike(de.spiked_accum(feat["ids"]), feat["ids"])
    texels, _, _ = de.count_slots(s != 1)
    assert (texels == 0).sum() == 2
    with pytest.raises(AssertionError):
        de.assert_crosses_the_slots(s != 1)


# ---------------------------------------------------------------- the value range
def test_the_examples_as_derived_by_hand():
    """what _derive gives for every example, stated once more as literals"""
    by_name = {e[0]: e for e in de.EXAMPLES}
    fill9 = lambda e, j=0: [e[2]] * (9 - len(e[1])) + [c for i, c in enumerate(e[1]) if i != j]
    verdict = {name: [de._derive(c, fill9(e, j)) for j, c in enumerate(e[1])] for name, e in by_name.items()}
    for name in ("tie", "two infinite luminances", "negative neighbours, centre 0", "negative neighbours, centre -0"):
        assert all(not v[0] and v[1] == 1 for v in verdict[name]), name
    assert de._lum(by_name["tie"][1][0]) == de._lum(by_name["tie"][1][1]) == F(10)
    assert np.isposinf(de._lum(by_name["two infinite luminances"][1][1])) and np.isfinite(by_name["two infinite luminances"][1][1]).all()
    assert np.signbit(de._lum(by_name["negative neighbours, centre -0"][1][0])) and de._lum(by_name["negative neighbours, centre -0"][1][0]) == 0
    for name in ("negative neighbours", "-0 neighbours"):
        clamped, s, rgb = verdict[name][0]
        assert clamped and s == 0 and not np.signbit(s) and [np.signbit(v) for v in rgb] == [False, True, False] and not any(rgb)
    assert np.signbit(de._lum(by_name["-0 neighbours"][2])) and de._lum(by_name["negative neighbours"][2]) < 0
    for name in ("NaN neighbours", "luminance overflows"):
        clamped, s, rgb = verdict[name][0]
        assert clamped and s == 0 and rgb == (0, 0, 0) and not any(np.signbit(v) for v in rgb), name
    assert np.isnan(de._lum(by_name["NaN neighbours"][2])) and np.isposinf(de._lum(by_name["luminance overflows"][1][0]))
    clamped, s, rgb = verdict["subnormal over subnormal"][0]
    cap, lp = de._lum(by_name[ "subnormal over subnormal"][2]), de._lum(by_name["subnormal over subnormal"][1][0])
    assert clamped and 0 < cap < lp < gr.TINY and abs(float(s) - float(cap) / float(lp)) <= 2.0 ** -25 and 0.33 < s < 0.34
    assert all(0 < v < gr.TINY for v in rgb)
    for name in ("subnormal s", "subnormal s, infinite M2"):
        clamped, s, rgb = verdict[name][0]
        assert clamped and 0 < s < gr.TINY and abs(float(s) - 1e-39) < 1e-41 and s * s == 0 and all(abs(float(v) - 1e-3) < 1e-6 for v in rgb)


def test_a_texel_alone_in_its_class_is_left_alone_whatever_it_holds(features):
    for value in (de.LONE, (de.INF,) * 3):
        C = np.ones((3, 3, 4), F)
        C[1, 1, :3] = value
        mat = np.zeros((3, 3), int)
        mat[1, 1] = 5
        for out, s in (dr.despike(C, _ids(mat))[:2], _scalar_law(C, _ids(mat))[:2]):
            assert out.tobytes() == C.tobytes() and np.all(s == 1)
    # the size test_gpu_guided_despike.py::test_a_texel_alone_in_its_class_keeps_the_largest_mean runs at has such a texel; the catalogue's sizes have none
    assert (de.taps_of_class(de.class_of(features(48, 12)["ids"])) == 0).sum() >= 1
    assert all((de.taps_of_class(de.class_of(features(w, h)["ids"])) == 0).sum() == 0 for w, h in tg.EDGE_SIZES)


@pytest.mark.parametrize("w,h", tg.EDGE_SIZES, ids=[f"{w}x{h}" for w, h in tg.EDGE_SIZES])
def test_the_catalogue_places_every_entry_and_every_example(features, w, h):
    feat = features(w, h)
    names = {e[0] for e in ec.entries(False) if e[0].startswith("mean=")}
    assert len(names) == 13
    for finite in (True, False):
        moments = de.mixed_moments(w, h)
        accum, where, placed = de.catalogue(feat["ids"], finite, moments)
        want = {n for n in names if finite is False or dict((e[0], e[2]) for e in ec.MEANS)[n[5:]]}
        assert set(where) == want and not ec.seam_sides(where, w, h)
        cover = de.coverage(where, placed, feat["ids"])
        print(f"{w} x {h}, finite {finite}, pitch {de.PITCH}: every entry at {min(len(v) for v in where.values())} places and more; pairs of an "
              f"entry and a plain texel of its class: {min(cover.values())} .. {max(cover.values())} per entry")
        # every entry at least once as a centre with a plain counting tap and as a counting tap of a plain centre (counting is symmetric)
        assert min(cover.values()) >= 1
        # every example at a seam site and away from one, inside one class, its patch as written
        cls = de.class_of(feat["ids"])
        for name in [e[0] for e in de.EXAMPLES]:
            sites = [e for e in placed if e["name"] == name]
            assert [e["seam"] for e in sites] == [True, False], name
            for e in sites:
                y, x = e["centres"][0]
                assert (cls[y - 1:y + 2, x - 1:x + 3] == cls[y, x]).all() and (de.taps_of_class(cls)[y, x] == 8)
                if e["seam"]:
                    assert x % 32 == 31 or y % 8 in (0, 7), (name, y, x)
        seams = [(e["centres"][0][1] % 32 == 31, e["centres"][0][0] % 8 in (0, 7)) for e in placed if e["seam"]]
        assert any(c for c, _ in seams) and any(r for _, r in seams)               # a column seam and a row seam are both crossed
        # the verdicts, on the numpy restatement and on the scalar walk
        cd, s, stats = dr.despike(accum, feat["ids"])
        de.check_examples(placed, cd, s, accum)
        cd2, s2, _ = _scalar_law(accum, feat["ids"].view(np.int32) if feat["ids"].dtype != np.int32 else feat["ids"])
        de.check_examples(placed, cd2, s2, accum)
        assert pc.same_bits_or_nan(cd, cd2) and pc.same_bits(s, s2)
        # the branches: clamped and not, s = 0, a subnormal s, negative, -0, infinite and NaN luminances as centres and as taps
        L = dr.luminance(accum)
        assert (s == 0).sum() >= 6 and ((s > 0) & (s < gr.TINY)).sum() >= 4 and (L < 0).any() and (np.signbit(L) & (L == 0)).any()
        assert np.isposinf(L).any() and np.isnan(L).any() and ((L > 0) & (L < gr.TINY)).any()
        if not finite:
            assert np.isneginf(accum).any() and np.isposinf(accum).any() and np.isnan(accum).any()


def test_why_the_whole_catalogue_lies_six_texels_apart(orc, features):
    """three apart, one level leaves a NaN in more than half of the filtered texels and little to compare"""
    w, h = tg.EDGE_SIZES[0]
    feat = features(w, h)
    share = {}
    for pitch in (3, 6):
        accum, _, _ = de.catalogue(feat["ids"], False, de.mixed_moments(w, h), pitch=pitch)
        out = dr.guided(orc, accum, feat["normal"], feat["position"], feat["albedo"], feat["ids"], 1, *tg.SIGMAS)[0]
        share[pitch] = float(np.isnan(out).any(axis=-1).mean())
    print(f"a NaN in {share[3]:.3f} of the filtered texels at pitch 3, {share[6]:.3f} at pitch 6")
    assert share[3] > 0.5 >= share[6] > 0 and de.PITCH == 6


@pytest.mark.parametrize("w,h,mode,sigmas", tg.EDGE_CASES, ids=[f"{w}x{h}-{m}-{'tight' if s is tg.TIGHT else 'default'}" for w, h, m, s in tg.EDGE_CASES])
def test_the_gpu_cases_are_not_vacuous(orc, features, w, h, mode, sigmas):
    """test_gpu_guided_despike.py::test_value_edges' own conditions with the oracle's features: count > 0, a NaN in more than 0 and at most
    half of the filtered texels, every example's verdict, var_0 of the subnormal-s examples 0 and NaN, sigma_color 1e-3 follows c'"""
    tg.edge_reference(orc, features(w, h), w, h, mode, sigmas)


@pytest.mark.parametrize("mode", list(tg.MODES))
def test_the_finite_catalogue_as_binary16_stores_it(orc, features, mode):
    """test_gpu_guided_despike.py::test_value_edges_of_a_mean_stored_as_binary16 on the reference alone"""
    w, h = tg.EDGE_SIZES[0]
    feat = features(w, h)
    accum, _, _ = de.catalogue(feat["ids"], True, None, examples=False)
    with np.errstate(over="ignore"):
        stored = accum.copy()
        stored[..., :3] = accum[..., :3].astype(np.float16).astype(F)
    assert np.isfinite(accum).all() and np.isinf(stored).any()
    tg.edge_reference(orc, feat, w, h, mode, tg.SIGMAS, finite=True, examples=False, stored=stored)
