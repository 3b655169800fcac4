"""Edge values of the (mean, moments) pair the image-space kernels pass among themselves, and where a test image holds them
(DESIGN.md "Pinned value range").  The counts n, the sums M2 and the means on either side of every value branch of include/mi3pt.h:
`!(n >= 1)`, `n >= 2`, the fmaxf that clamps a negative quotient and drops a NaN, `nk >= 1`, "n stops growing at 2^24", the binary16
rounding of a stored mean, fp32 subnormals.  placed() puts every entry at recorded coordinates of an otherwise plain image, on both
sides of the block seams of the kernel under test; THRESHOLDS and BY_COUNT hold worked examples whose results were computed by hand
from the header's lines (tests/test_moments_edge_cases.py asserts them on the numpy restatements).  Nothing here looks at the device.
No test lives in this file.
"""
import numpy as np

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
BELOW_ONE, BELOW_TWO = np.nextafter(F(1), F(0)), np.nextafter(F(2), F(0))

# (name, value, finite): finite=False entries are left out of the finite catalogue
COUNTS = [("nan", NAN, False), ("-1", F(-1), True), ("-0", F(-0.0), True), ("0", F(0), True), ("0.5", F(0.5), True),
          ("below 1", BELOW_ONE, True), ("1", F(1), True), ("1.5", F(1.5), True), ("below 2", BELOW_TWO, True), ("2", F(2), True),
          ("3", F(3), True), ("2^24-1", F(2 ** 24 - 1), True), ("2^24", F(2 ** 24), True), ("3e38", F(3e38), True), ("inf", INF, False)]
M2S = [("0", F(0), True), ("-0", F(-0.0), True), ("-1", F(-1), True), ("1e-42", F(1e-42), True), ("1e-38", F(1e-38), True),
       ("1", F(1), True), ("3e38", F(3e38), True), ("inf", INF, False), ("nan", NAN, False)]
# 6e-8: a binary16 subnormal; 65504: the largest binary16; 65519.996: the largest fp32 binary16 rounds to it; 65520: the first it rounds to inf;
# 1e19 squares finitely, 3e38 does not
MEANS = [("0", F(0), True), ("-0", F(-0.0), True), ("1e-42", F(1e-42), True), ("6e-8", F(6e-8), True), ("65504", F(65504), True),
         ("65519.996", F(65519.996), True), ("65520", F(65520), True), ("1e19", F(1e19), True), ("3e38", F(3e38), True),
         ("-2.5", F(-2.5), True), ("inf", INF, False), ("-inf", -INF, False), ("nan", NAN, False)]


def _triples(values, finite):
    """one (name, (v_i, v_i+1, v_i+2)) per value: the channels of a texel differ"""
    vals = [(n, v) for n, v, f in values if f or not finite]
    return [(vals[i][0], tuple(vals[(i + k) % len(vals)][1] for k in range(3))) for i in range(len(vals))]


def entries(finite):
    """the catalogue as texels: (name, n, M2.rgb, mean.rgb), None = the background's value stays"""
    out = []
    for name, v, f in COUNTS:
        if f or not finite:
            out.append((f"n={name}", v, None, None))
    for i, (name, t) in enumerate(_triples(M2S, finite)):
        out.append((f"m2={name}", F(3) if i % 2 == 0 else F(500), t, None))
        out.append((f"m2={name},n=2", F(2), t, None))
    for name, t in _triples(MEANS, finite):
        out.append((f"mean={name}", None, None, t))
    # a count on one side of a branch with an M2 that tells the sides apart
    one = (F(1), F(-1), F(1e-38))
    out += [("n=1.5,m2=1,-1,1e-38", F(1.5), one, None), ("n=below 2,m2=1,-1,1e-38", BELOW_TWO, one, None), ("n=2,m2=1,-1,1e-38", F(2), one, None),
            ("n=1,m2=3e38", F(1), (F(3e38), F(3e38), F(-3e38)), None), ("n=2^24,m2=3e38", F(2 ** 24), (F(3e38), F(1), F(0)), None),
            ("n=3e38,m2=3e38", F(3e38), (F(3e38), F(1), F(-1)), None), ("n=below 1,mean=65520", BELOW_ONE, None, (F(65520), F(-65520), F(65504))),
            ("n=3,mean=65520", F(3), None, (F(65520), F(-65519.996), F(6e-8)))]
    if not finite:
        out += [("n=nan,m2=nan", NAN, (NAN, F(1), INF), None), ("n=inf,m2=inf", INF, (INF, F(1), NAN), None), ("n=2,mean=nan", F(2), None, (NAN, F(1), INF))]
    return out


def background(w, h, seed):
    """a plain pair: the mean in [0, 4), alpha 1, M2 in [0, 50), n of 0, 1, 2 and 500"""
    rng = np.random.default_rng(seed)
    mean = (rng.random((h, w, 4), dtype=F) * 4).astype(F)
    mean[..., 3] = 1
    mo = (rng.random((h, w, 4), dtype=F) * 50).astype(F)
    mo[..., 3] = rng.choice(np.array([0, 1, 2, 500], F), size=(h, w), p=[0.15, 0.15, 0.2, 0.5])
    return mean, mo


def positions(w, h, seam=8, linear=None, pitch=3):
    """where edge texels go, as (y, x): a lattice `pitch` = three texels apart (a radius-3 window and a 5 x 5 window four apart then hold edge and
    plain taps both), and on every third row / column of the lattice the two texels either side of each multiple of `seam` (8: the 8 x 8 tiles' seams,
    and with them the 16 x 16 and 32 x 8 ones); linear: both sides of every multiple of it in row-major order (1-D blocks)"""
    at = {(y, x) for y in range(0, h, pitch) for x in range(0, w, pitch)}
    for s in range(seam, w, seam):
        at |= {(y, x) for y in range(0, h, 3 * pitch) for x in (s - 1, s)}
    for s in range(seam, h, seam):
        at |= {(y, x) for x in range(0, w, 3 * pitch) for y in (s - 1, s)}
    if linear:
        for k in range(linear, w * h, linear):
            at |= {((k - 1) // w, (k - 1) % w), (k // w, k % w)}
    return sorted(at)


def overlay(mean, moments, seed, finite, seam=8, linear=None, only=None, pitch=3):
    """writes the catalogue into a pair (in place).  Returns where: name -> [(y, x), ...].  only: a predicate on an entry's name"""
    h, w = mean.shape[:2]
    cat = [e for e in entries(finite) if only is None or only(e[0])]
    at = positions(w, h, seam, linear, pitch)
    assert len(at) >= len(cat), f"{w} x {h}: {len(at)} places for {len(cat)} entries"
    order = np.random.default_rng(seed + 77).permutation(len(at))
    where = {}
    for k, j in enumerate(order):
        y, x = at[j]
        name, n, m2, mu = cat[k % len(cat)]
        if n is not None:
            moments[y, x, 3] = n
        if m2 is not None:
            moments[y, x, :3] = m2
        if mu is not None:
            mean[y, x, :3] = mu
        where.setdefault(name, []).append((y, x))
    return where


def placed(w, h, seed, finite, seam=8, linear=None, only=None, pitch=3):
    """(mean, moments, where): background() with the catalogue written over it"""
    mean, mo = background(w, h, seed)
    return mean, mo, overlay(mean, mo, seed, finite, seam, linear, only, pitch)


def seam_sides(where, w, h, seam=8):
    """the seams x = s - 1 | s and y = s - 1 | s (s a multiple of `seam`) that lack an edge texel on either side: [] when every seam is held"""
    ys = {y for at in where.values() for y, _ in at}
    xs = {x for at in where.values() for _, x in at}
    return [("x", s) for s in range(seam, w, seam) if not {s - 1, s} <= xs] + [("y", s) for s in range(seam, h, seam) if not {s - 1, s} <= ys]


# ---- weights in the fp32 subnormal range (mi3pt_denoise_guided): exp(x) is a subnormal for x in about (-103.97, -87.34).  A bright texel
# (1, 1, 1) in the middle of a 9 x 9 patch of colour 0: at level 0 the 24 texels around it see it at a squared colour distance of 3 and
# nothing else that is not 0, so their num is the subnormal weight itself -- a build that flushes it returns 0 there.
#   plain filter: ec = 3 / sigma_color^2 = 92.6 at sigma_color 0.18;
#   MI3PT_GUIDED_VARIANCE: ec = 3 / (sigma_color^2 * var + EPS); the patch's moments (M2 = 0.0324 per channel, n = 4) give every texel and
#   so every 3 x 3 mean the variance of the mean 3 * 0.0324 / 12 = 0.0081, and sigma_color = 2: ec = 92.6
SUBNORMAL_SIGMA_PLAIN = 0.18
SUBNORMAL_SIGMA_VARIANCE = 2.0
SUBNORMAL_M2, SUBNORMAL_N = F(0.0324), F(4)


def subnormal_patches(mean, moments=None, pitch=12, first=6):
    """writes the patches into a mean (and a moments image) in place, centres `pitch` apart from (first, first) on; returns the centres"""
    h, w = mean.shape[:2]
    centres = [(y, x) for y in range(first, h - 4, pitch) for x in range(first, w - 4, pitch)]
    for y, x in centres:
        mean[y - 4:y + 5, x - 4:x + 5, :3] = 0
        mean[y, x, :3] = 1
        if moments is not None:
            moments[y - 4:y + 5, x - 4:x + 5, :3] = SUBNORMAL_M2
            moments[y - 4:y + 5, x - 4:x + 5, 3] = SUBNORMAL_N
    return centres


# ---- squared weights in the fp32 subnormal range (MI3PT_GUIDED_VARIANCE: nv = nv + (w * w) * var(q)) under a weight that is normal
# itself -- subnormal_patches makes w subnormal, so its w * w is 0.  A 13 x 13 patch of colour 0.5, M2 = 0, n = 4 with a 3 x 3 block
# brighter by delta in every channel in its middle and M2 = 1e6 per channel at the block's centre alone: var_0 is non-zero exactly on the
# block (v = 3e6 / 12 at its centre, blurred over 3 x 3).  A texel of the two rings around the block has var = 0, so its colour
# denominator is MI3PT_GUIDED_VARIANCE_EPS = 1e-8 and with sigma_color = 1 a bright tap has ec = 3 delta^2 / 1e-8; the bright taps are
# the only ones that carry variance, so the ring's output variance is the sum of their (w * w) * var(q) over den^2 and nothing else.
#   delta = 3.873e-4: ec = 45, w = exp(-45) h = 2.9e-20 h is normal for every h = h[dx] h[dy] >= 1 / 256, w * w = 8.2e-40 h^2 is not; the
#   rings' variances lie between 2e-40 and 7e-37 (measured on the reference at 100 x 52), a build that flushes the squares returns 0;
#   ec = 40: exp(-80) h^2 is still subnormal under h = 1 / 256, but every ring sums squares of 1e-37 and more: no output is subnormal;
#   ec = 50: exp(-100) h^2 <= 3.7e-44 * (3 / 32)^2 = 3.3e-46 lies below half of the smallest subnormal: every square and every ring is 0
SQUARED_SIGMA = 1.0
SQUARED_DELTA = {40: F(3.651e-4), 45: F(3.873e-4), 50: F(4.082e-4)}       # ec -> delta = sqrt(ec * 1e-8 / 3)
SQUARED_M2, SQUARED_N, SQUARED_BASE = F(1e6), F(4), F(0.5)


def squared_weight_patches(mean, moments, hit=None, delta=SQUARED_DELTA[45], pitch=12, first=6):
    """writes the patches into a (mean, moments) pair in place, centres `pitch` apart from (first, first) on; hit: an image (the ids'
    word 2) -- only the patches whose 13 x 13 texels lie in one hit class are written
    (neighbouring patches share their outermost column or row, which holds the same values in both).  Returns the centres"""
    h, w = mean.shape[:2]
    centres = []
    for y in range(first, h - 6, pitch):
        for x in range(first, w - 6, pitch):
            if hit is not None and (hit[y - 6:y + 7, x - 6:x + 7] != hit[y, x]).any():
                continue
            mean[y - 6:y + 7, x - 6:x + 7, :3] = SQUARED_BASE
            moments[y - 6:y + 7, x - 6:x + 7, :3] = 0
            moments[y - 6:y + 7, x - 6:x + 7, 3] = SQUARED_N
            centres.append((y, x))
    for y, x in centres:
        mean[y - 1:y + 2, x - 1:x + 2, :3] = SQUARED_BASE + F(delta)
        moments[y, x, :3] = SQUARED_M2
    return centres


def rings(centres, shape):
    """the texels two and three away from a block's centre (Chebyshev): var = 0 themselves, the block in reach of their 5 x 5"""
    mask = np.zeros(shape, bool)
    for y, x in centres:
        mask[y - 3:y + 4, x - 3:x + 4] = True
        mask[y - 1:y + 2, x - 1:x + 2] = False
    return mask


def non_finite_means(mean, at):
    """writes the non-finite mean entries at the given (y, x), one after the other (few: every one of them spreads over 5 x 5 texels per
    level of the guided filter)"""
    for (y, x), (_, t) in zip(at, [e for e in _triples(MEANS, False) if not np.isfinite(e[1][0])]):
        mean[y, x, :3] = t


class FlushedExp:
    """an oracle whose exp (math_fn 4) returns 0 where the result is an fp32 subnormal: what a flushing build computes"""

    def __init__(self, orc):
        self.orc = orc

    def math_fn(self, which, x):
        out = self.orc.math_fn(which, x)
        if which != 4:
            return out
        return np.where(np.abs(out) < F(2.0 ** -126), F(0), out).astype(F)          # (a NaN stays)


# ---- the merge at its thresholds (mi3pt_merge_history), radius 0, one texel: live (mean, M2, n), held (mean, M2, n), (z_keep, z_drop), and
# the header's result: lam, nk, and for a merged texel (mean', M2', N).  With M2 = 1, n = nh = 2: var = 1, V = 1 * (1/2 + 1/2) = 1 (EPS is
# absorbed), z2 = D^2
def _t(name, diff, m2, n, z, lam, nk, merged=None, live_m2=None, held_m2=None):
    """live and held as (mean.rgb, M2.rgb, n); `merged`: the result's (mean.r, M2.r, N)"""
    return dict(name=name, live=((F(diff), F(0), F(0)) if live_m2 or held_m2 else (F(diff),) * 3, live_m2 or (F(m2),) * 3, F(n)),
                held=((F(0),) * 3, held_m2 or (F(m2),) * 3, F(n)), z=z, lam=F(lam), nk=F(nk), merged=merged)


THRESHOLDS = [
    _t("z2 equals keep2", 2, 1, 2, (2.0, 4.0), 1, 2, merged=(F(1), F(6), F(4))),        # mean 2 + (0 - 2) * 2/4; M2 (1 + 1 * 1) + 4 * (2 * 2/4)
    _t("z2 equals drop2", 4, 1, 2, (2.0, 4.0), 0, 0),
    _t("just above keep", np.nextafter(F(2), F(3)), 1, 2, (2.0, 4.0), 0.99999994, 1, merged=(F(1.3333335), F(3.6666675), F(3))),
    _t("just below drop", np.nextafter(F(4), F(3)), 1, 2, (2.0, 4.0), 1.59e-7, 0),
    _t("half kept", 2, 2, 2, (0.0, 2.0), 0.5, 1, merged=(F(1.3333333), F(4.666667), F(3))),          # nk - 1 = 0: the held variance does not enter
    _t("fractional counts", 0, 1, 1.5, (2.0, 4.0), 1, 1, merged=(F(0), F(1), F(2.5))),
    # a NaN M2 on one side: the means differ in the red channel alone, by 5, and red is the channel whose M2 is a NaN.  var()'s fmaxf drops
    # it (the variance of that side is 0), V.r = 1 * (1/2 + 1/2) from the other side, z2 = 25, dropped.  (Were the NaN kept, z.r would be a
    # NaN, the fmaxf over the channels would drop IT, z2 = 0 and the whole history would be merged.)  var() never returns a NaN, so the
    # fmaxf(sf.k, sh.k) after it never sees one.
    _t("held M2 NaN", 5, 1, 2, (2.0, 4.0), 0, 0, held_m2=(NAN, F(1), F(1))),
    _t("live M2 NaN", 5, 1, 2, (2.0, 4.0), 0, 0, live_m2=(NAN, F(1), F(1))),
    # z.g = inf / inf, a NaN, beside z.r = 25: fmaxf(fmaxf(z.r, z.g), z.b) drops it, z2 = 25, dropped (a comparison in its place: z2 = 0, merged)
    dict(name="z NaN in one channel", live=((F(5), INF, F(0)), (F(1), INF, F(1)), F(2)), held=((F(0), F(0), F(0)), (F(1), INF, F(1)), F(2)),
         z=(2.0, 4.0), lam=F(0), nk=F(0), merged=None),
]
# (z_keep, z_drop) at the ends: what lam is wherever both sides hold samples; D0: at texels whose pooled difference is exactly 0
Z_EXTREMES = [dict(name="drop2 overflows", z=(2.0, 3e19), lam=0, lam_d0=0), dict(name="squares both zero", z=(0.0, 1e-30), lam=0, lam_d0=0),
              dict(name="equal subnormal squares", z=(1e-20, 1.0000001e-20), lam=0, lam_d0=1)]

# ---- one by-count step (mi3pt_set_mean_by_count) from mean 2, M2 1 with radiance 3: n -> (mean', M2', n')
BY_COUNT = [(n, (F(3), F(0), F(1))) for n in (NAN, F(-1), F(-0.0), F(0), F(0.5), BELOW_ONE)] + [
    (F(1.5), (F(2.4), F(1.5999999), F(2.5))),
    (F(2 ** 24 - 1), (F(2), F(2), F(2 ** 24))), (F(2 ** 24), (F(2), F(2), F(2 ** 24))),
    (F(3e38), (F(2), F(2), F(3e38))), (INF, (F(2), F(2), INF))]
