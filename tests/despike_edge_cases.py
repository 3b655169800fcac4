"""Inputs for the firefly pre-pass of the guided de-noise (include/mi3pt.h: mi3pt_set_guided_despike; csrc/pt_guided.hip:
k_guided_despike) at the edges of its decomposition and of its value range (DESIGN.md "Pinned decomposition", "Pinned value range").

The decomposition: count_slots() restates the kernel's launch arithmetic -- which wave clamps a texel and which of the DESPIKE_SLOTS
count words it adds to -- from a mask of clamped texels, so that a test can say on the reference alone that an image folds more waves
than there are slots.

The value range: catalogue() writes the means of tests/moments_edge_cases.py over the spiked image, and worked examples -- small patches
inside one feature class, placed from the ids image, each once across a 32 x 8 tile seam and once away from one -- whose results were
derived by hand from the header's lines (exact arithmetic in binary64, rounded once; never taken from a restatement under test).
tests/test_despike_edge_cases.py asserts them on the numpy reference and on the scalar walk.  Nothing here looks at the device.  No test
lives in this file.
"""
import numpy as np

import moments_edge_cases as ec

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
TILE_W, TILE_H, WAVES, SLOTS = 32, 8, 4, 64        # k_guided_despike: a 32 x 8 tile per block of four waves; pt_kernels.h: DESPIKE_SLOTS
THIRD = np.float64(F(1) / F(3))
BELOW_FOUR = np.nextafter(F(4), F(0))


# ---- the plain images (tests/test_gpu_guided_despike.py writes them; here so that the CPU tests build the same ones)
def class_of(ids):
    words = np.ascontiguousarray(ids).view(np.int32)
    return words[..., 1].astype(np.int64) * 2 + words[..., 2]


def spiked_accum(ids, seed=20261020):
    """seeded colours in [0, 4) -- a texel that happens to be the brightest of its class in its 3 x 3 is clamped by a little -- with
    spikes of 30 .. 200 times that planted in the four image corners, on the texels of a class border (one whose right or upper
    neighbour is of another class; every third of them), and as an adjacent pair inside a class where the image has room for one"""
    h, w = ids.shape[:2]
    rng = np.random.default_rng(seed + 1000 * w + h)
    a = (rng.random((h, w, 4), dtype=F) * F(4)).astype(F)
    cls = class_of(ids)
    border = np.zeros((h, w), bool)
    border[:, :-1] |= cls[:, :-1] != cls[:, 1:]
    border[:-1, :] |= cls[:-1, :] != cls[1:, :]
    planted = np.zeros((h, w), bool)
    ys, xs = np.nonzero(border)
    planted[ys[::3], xs[::3]] = True
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        planted[y, x] = True
    if w >= 8 and h >= 4:
        same = (cls[:, :-1] == cls[:, 1:]) & ~border[:, :-1] & ~border[:, 1:]
        same[0, :] = same[-1, :] = False
        ys, xs = np.nonzero(same)
        if len(ys):
            k = len(ys) // 2
            planted[ys[k], xs[k]] = planted[ys[k], xs[k] + 1] = True
    boost = (F(30) + rng.random((h, w), dtype=F) * F(170)).astype(F)
    a[..., :3] = np.where(planted[..., None], a[..., :3] * boost[..., None], a[..., :3])
    return a


def smooth_accum(ids):
    """a colour per class: nothing to clamp"""
    cls = class_of(ids)
    values, index = np.unique(cls, return_inverse=True)
    palette = (np.random.default_rng(5).random((len(values), 4), dtype=F) * F(4)).astype(F)
    return palette[index.reshape(cls.shape)]


def mixed_moments(w, h, seed=20261019):
    """seeded M2 in [0, 24) where the count holds a variance, counts on either side of MI3PT_GUIDED_YOUNG_COUNT"""
    rng = np.random.default_rng(seed)
    counts = np.array([1, 2, 3, BELOW_FOUR, 4, 64], F)
    m = (rng.random((h, w, 4), dtype=F) * F(24)).astype(F)
    m[..., 3] = counts[rng.integers(0, len(counts), (h, w))]
    m[..., :3] = np.where(m[..., 3:] >= 2, m[..., :3], 0)
    return m


# ---- the count's decomposition
def count_slots(clamped):
    """k_guided_despike's launch arithmetic from a (rows, w) mask of clamped texels: grid = ceil(w / 32) x ceil(rows / 8) blocks of four
    waves, a wave is two tile rows; wave = (by * grid_x + bx) * 4 + (row in tile) / 2 adds its clamped texels to slot wave mod 64.
    Returns (texels added per slot, number of distinct waves that add per slot, the numbers of the waves that add) -- a wave that clamps
    nothing adds nothing."""
    clamped = np.asarray(clamped, bool)
    rows, w = clamped.shape
    grid_x = (w + TILE_W - 1) // TILE_W
    ys, xs = np.nonzero(clamped)
    wave = ((ys // TILE_H) * grid_x + xs // TILE_W) * WAVES + (ys % TILE_H) // 2
    adding = np.unique(wave)
    return np.bincount(wave % SLOTS, minlength=SLOTS), np.bincount(adding % SLOTS, minlength=SLOTS), adding


def launch_shape(w, rows):
    """(blocks, waves) of the launch"""
    blocks = ((w + TILE_W - 1) // TILE_W) * ((rows + TILE_H - 1) // TILE_H)
    return blocks, blocks * WAVES


# ---- the header's lines in exact arithmetic, rounded once per operation: what a worked example's result is derived with
def _lum(t):
    """L of one texel: every sum and the product rounded to fp32 once (a binary64 sum or product of two fp32 values is exact or
    rounds the same way twice: 53 >= 2 * 24 + 2)"""
    with np.errstate(all="ignore"):
        a = F(np.float64(t[0]) + np.float64(t[1]))
        a = F(np.float64(a) + np.float64(t[2]))
        return F(np.float64(a) * THIRD)


def _derive(centre, neighbours):
    """(clamped, s, c'.rgb) of a centre all of whose eight taps count, from the header's lines"""
    cap = F(0)
    for q in neighbours:
        lq = _lum(q)
        if lq > cap:                                  # fmaxf from +0: a NaN and a -0 both leave +0
            cap = lq
    lp = _lum(centre)
    if not lp > cap:
        return False, F(1), tuple(F(v) for v in centre)
    with np.errstate(all="ignore"):
        s = F(np.float64(cap) / np.float64(lp))
        return True, s, tuple(F(np.float64(v) * np.float64(s)) for v in centre)


# name, the centre(s) -- one texel or an adjacent pair --, the colour of every other texel of the 3 x 4 patch, (M2.rgb, n) of the centre or
# None, and what the header's lines give, stated in words.  An s that rounds to 1 for a clamped texel cannot occur and has no example:
# cap / L(p) with cap < L(p) lies at least 2^-24 below 1.
_NEG = (F(-1), F(-2), F(-0.5))
EXAMPLES = [
    ("tie", [(F(30), F(0), F(0)), (F(0), F(30), F(0))], (F(1), F(1), F(1)), None, "L = 10 both, each is the other's cap: neither is clamped"),
    ("negative neighbours", [(F(1), F(-0.25), F(0.5))], _NEG, None, "cap stays +0, s = 0, c' = (0, -0, 0)"),
    ("negative neighbours, centre 0", [(F(0), F(0), F(0))], _NEG, None, "L = +0 is not above +0: not clamped"),
    ("negative neighbours, centre -0", [(F(-0.0), F(-0.0), F(-0.0))], _NEG, None, "L = -0 is not above +0: not clamped"),
    ("-0 neighbours", [(F(1), F(-0.25), F(0.5))], (F(-0.0), F(-0.0), F(-0.0)), None,
     "fmaxf(+0, -0): the header pins +0 (a luminance of -0 never becomes the cap), s = +0, c' = (0, -0, 0)"),
    ("NaN neighbours", [(F(2), F(1), F(3))], (NAN, F(1), NAN), None, "fmaxf drops every tap: cap 0, s = 0, c' = 0"),
    ("luminance overflows", [(F(3e38), F(3e38), F(3e38))], (F(1), F(1), F(1)), None, "L = +inf from finite channels over cap 1: s = 0, c' = 3e38 * 0 = 0"),
    ("two infinite luminances", [(F(3e38), F(3e38), F(3e38)), (F(3e38), F(3e38), F(1))], (F(1), F(1), F(1)), None, "inf > inf is false: neither is clamped"),
    ("subnormal over subnormal", [(F(3e-42), F(3e-42), F(3e-42))], (F(1e-42), F(1e-42), F(1e-42)), None,
     "cap about 1e-42 under L about 3e-42: s the correctly rounded quotient, about 1/3; c' subnormal"),
    ("subnormal s", [(F(1e36), F(1e36), F(1e36))], (F(1e-3), F(1e-3), F(1e-3)), ((F(6), F(6), F(6)), F(4)),
     "s about 1e-39, s * s = 0: var_0 = 1.5 * 0 = 0"),
    ("subnormal s, infinite M2", [(F(1e36), F(1e36), F(1e36))], (F(1e-3), F(1e-3), F(1e-3)), ((INF, F(1), F(1)), F(4)),
     "s about 1e-39, s * s = 0: var_0 = inf * 0, a NaN"),
]
LONE = (F(3e38), F(3e38), F(3e38))          # a texel alone in its class takes the largest finite mean of the catalogue: m = 0, left alone
PATCH_MOMENTS = ((F(6), F(6), F(6)), F(4))  # every other texel of a patch that writes moments: v = 18 / 12


def _sites(cls, used):
    """(seam sites, other sites): the (y, x) whose patch -- rows y - 1 .. y + 1, columns x - 1 .. x + 2 -- lies inside the image, in one
    class and on unused texels.  A seam site has a 32 x 8 tile seam between the centre and one of its taps (between the two centres of a
    pair where the seam is a column)"""
    rows, w = cls.shape
    seam, other = [], []
    for y in range(1, rows - 1):
        for x in range(1, w - 2):
            block = cls[y - 1:y + 2, x - 1:x + 3]
            if (block != block[0, 0]).any() or used[y - 1:y + 2, x - 1:x + 3].any():
                continue
            (seam if x % TILE_W == TILE_W - 1 or y % TILE_H in (0, TILE_H - 1) else other).append((y, x))
    return seam, other


def place_examples(accum, moments, ids):
    """writes every example twice, at a seam site and at another one, and LONE on the texels without a tap of their class (in place;
    moments may be None).  Returns [{name, centres: [(y, x)], clamped: [bool], s: [fp32], rgb: [3 fp32], seam: bool, m2: ...}]; the
    expected values come from _derive, never from a restatement under test."""
    cls = class_of(ids)
    rows, w = cls.shape
    used = np.zeros((rows, w), bool)
    placed = []
    for k, (name, centres, fill, mo, _) in enumerate(EXAMPLES):
        for want_seam in (True, False):
            seam, other = _sites(cls, used)
            pool = seam if want_seam else other
            if want_seam and len(centres) == 1 and k % 2:          # single centres: a row seam and a column seam in turn
                pool = [p for p in seam if p[0] % TILE_H in (0, TILE_H - 1)] or seam
            elif want_seam:
                pool = [p for p in seam if p[1] % TILE_W == TILE_W - 1] or seam
            assert pool, f"no {'seam ' if want_seam else ''}site left for {name!r} at {w} x {rows}"
            y, x = pool[(7 * k) % len(pool)]
            accum[y - 1:y + 2, x - 1:x + 3, :3] = fill
            at = [(y, x + j) for j in range(len(centres))]
            for (cy, cx), c in zip(at, centres):
                accum[cy, cx, :3] = c
            if mo is not None and moments is not None:
                moments[y - 1:y + 2, x - 1:x + 3, :3] = PATCH_MOMENTS[0]
                moments[y - 1:y + 2, x - 1:x + 3, 3] = PATCH_MOMENTS[1]
                moments[y, x, :3], moments[y, x, 3] = mo
            used[max(0, y - 2):y + 3, max(0, x - 2):x + 4] = True
            verdicts = []
            for j, c in enumerate(centres):
                taps = [fill] * (9 - len(centres)) + [c2 for i, c2 in enumerate(centres) if i != j]
                verdicts.append(_derive(c, taps))
            placed.append(dict(name=name, centres=at, clamped=[v[0] for v in verdicts], s=[v[1] for v in verdicts],
                               rgb=[v[2] for v in verdicts], seam=want_seam, m2=mo))
    # the texels alone in their class
    m = taps_of_class(cls)
    lone = [(int(y), int(x)) for y, x in np.argwhere((m == 0) & ~used)]
    for y, x in lone:
        accum[y, x, :3] = LONE
    if lone:
        placed.append(dict(name="alone in its class", centres=lone, clamped=[False] * len(lone), s=[F(1)] * len(lone),
                           rgb=[LONE] * len(lone), seam=False, m2=None))
    return placed


def taps_of_class(cls):
    """m per texel: the 3 x 3 neighbours inside the image whose class is the centre's"""
    rows, w = cls.shape
    m = np.zeros((rows, w), np.int32)
    pad = np.full((rows + 2, w + 2), -1, np.int64)
    pad[1:-1, 1:-1] = cls
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                m += pad[dy:dy + rows, dx:dx + w] == cls
    return m


def check_examples(placed, cd, s, accum):
    """every placed example's verdict on a restatement's (c', s): the scale's bits, the colour's bits (the sign of a zero included),
    an untouched texel where the example is not clamped"""
    for e in placed:
        for (y, x), clamped, want_s, rgb in zip(e["centres"], e["clamped"], e["s"], e["rgb"]):
            what = f"{e['name']} at ({y}, {x})"
            assert (s[y, x] != 1) == clamped, what
            assert F(s[y, x]).tobytes() == F(want_s).tobytes(), f"{what}: s {s[y, x]!r} for {want_s!r}"
            assert cd[y, x, :3].tobytes() == np.array(rgb, F).tobytes(), f"{what}: c' {cd[y, x, :3]} for {rgb}"
            assert cd[y, x, 3].tobytes() == accum[y, x, 3].tobytes(), what
            if not clamped:
                assert cd[y, x].tobytes() == accum[y, x].tobytes(), what


# ---- the catalogue of means over the spiked image
PITCH = 6          # three apart a level leaves a NaN in three quarters of the filtered texels (it spreads one over 5 x 5), six apart in 0.37


def catalogue(ids, finite, moments=None, examples=True, pitch=None, seed=6):
    """(accum, where, placed): spiked_accum with the `mean=` entries of moments_edge_cases written over it `pitch` texels apart and on both
    sides of every multiple of 8 (the 32 x 8 tile's seams among them), then the worked examples (which may overwrite an entry: `where`
    lists what is left).  moments: an image the examples that need one write into, in place."""
    accum = spiked_accum(ids)
    rows, w = accum.shape[:2]
    where = ec.overlay(accum, np.zeros((rows, w, 4), F), seed, finite, seam=8, only=lambda name: name.startswith("mean="),
                       pitch=PITCH if pitch is None else pitch)
    placed = place_examples(accum, moments, ids) if examples else []
    patch = patch_mask(placed, rows, w)
    where = {name: [p for p in at if not patch[p]] for name, at in where.items()}
    return accum, where, placed


def patch_mask(placed, rows, w):
    """the texels the examples wrote"""
    mask = np.zeros((rows, w), bool)
    for e in placed:
        if e["name"] == "alone in its class":
            for y, x in e["centres"]:
                mask[y, x] = True
        else:
            y, x = e["centres"][0]
            mask[y - 1:y + 2, x - 1:x + 3] = True
    return mask


def coverage(where, placed, ids):
    """name -> the number of (entry texel, plain texel) pairs that are 3 x 3 neighbours of one class; plain: neither an entry nor written
    by an example.  Counting is symmetric -- q counts for p iff p counts for q -- so each pair is the entry as a centre with a plain
    counting tap AND the entry as a counting tap of a plain centre."""
    cls = class_of(ids)
    rows, w = cls.shape
    plain = ~patch_mask(placed, rows, w)
    for at in where.values():
        for p in at:
            plain[p] = False
    out = {}
    for name, at in where.items():
        n = 0
        for y, x in at:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx = y + dy, x + dx
                    if (dy or dx) and 0 <= qy < rows and 0 <= qx < w and plain[qy, qx] and cls[qy, qx] == cls[y, x]:
                        n += 1
        out[name] = n
    return out


def assert_crosses_the_slots(clamped):
    """the conditions under which a (rows, w) mask of clamped texels folds the count over more waves than it has slots: a read that sums
    half of the slots, a clear of half of the buffer, a wrong slot stride or a wrong wave number then show in the count"""
    texels, waves, adding = count_slots(clamped)
    assert (texels > 0).all(), f"empty slots: {np.nonzero(texels == 0)[0].tolist()}"
    assert int((waves >= 2).sum()) >= 8, waves.tolist()
    assert adding.max() >= SLOTS and (adding >= SLOTS).sum() >= 8
    assert texels[:SLOTS // 2].sum() != texels.sum() and texels.sum() == int(np.asarray(clamped, bool).sum())
    return texels, waves, adding


def check_example_variances(placed, var0, scaled):
    """the examples that write moments, on a restatement's var_0 before and after the pre-pass's s * s: a positive var_0 becomes 0 under
    an s whose square underflows, an infinite one a NaN"""
    seen = 0
    for e in placed:
        if e["m2"] is None:
            continue
        y, x = e["centres"][0]
        if np.isinf(e["m2"][0][0]):
            assert np.isinf(var0[y, x]) and np.isnan(scaled[y, x]), e["name"]
        else:
            assert var0[y, x] == F(1.5) and scaled[y, x] == 0 and not np.signbit(scaled[y, x]), e["name"]
        seen += 1
    assert seen == 4
