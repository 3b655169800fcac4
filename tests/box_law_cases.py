"""One catalogue of inputs for the three pieces of code that write the boxes of the 48-byte BVH records -- the host SAH builder
(csrc/pt_host_scene.cpp), the device LBVH builder (csrc/pt_lbvh.hip) and the device refit (csrc/pt_refit.hip) -- at the values where
"the same box" is a question of words, not of values: zeros of both signs, subnormals next to zeros, NaNs with payloads, infinities.
The law they are held to is the refit's (include/mi3pt.h; tests/refit_reference.py is its plain statement):

    lo(x, y) = (y < x || (y == x && signbit(y))) ? y : x          hi(x, y) = (y > x || (y == x && !signbit(y))) ? y : x

which is Math.min / Math.max of the reference's Box3.expandByPoint on everything but a NaN.  Every set is tiny (at most 108 triangles);
the components a set does not speak about hold ordinary random values, so that the trees built over it are not degenerate.

    zeros(), subnormals(), non_finite()        -> Case: positions (float64), the fp32 words of the positions, a note
    mirrored(nodes), chain_right(k), zigzag(k), stamped(nodes, seed)         tree shapers over any of them

The claims the sets are built for are asserted here, at import, by evaluating the law alone (no library, no device).  No test lives
in this file."""
import functools

import numpy as np

import refit_reference as rr
from mi3pt_host import layout

F = np.float32
PZ, NZ = 0x00000000, 0x80000000                    # the words of +0 and -0
NAN_PAYLOADS = (0x7fc00001, 0xffc12345, 0x7f800001)          # quiet, quiet with the sign set, signalling
FLT_MAX = float(np.finfo(np.float32).max)


class Case:
    """positions: (n, 3, 3) float64 -- what the builders take (every value one fp32 holds exactly; a NaN here is the default NaN);
    words: (n, 3, 3) uint32 -- the fp32 words of the triangle records, NaN payloads included; build_positions: the positions a tree is
    built from (the set itself, or its finite stand-in where the set holds a NaN or an infinity: the tree a refit starts from was
    built before the vertices moved there)."""

    def __init__(self, name, positions, note, words=None, build_positions=None):
        self.name, self.note = name, note
        self.positions = np.ascontiguousarray(positions, np.float64)
        self.words = self.positions.astype(F).view("<u4").copy() if words is None else np.ascontiguousarray(words, "<u4")
        self.build_positions = self.positions if build_positions is None else np.ascontiguousarray(build_positions, np.float64)
        assert self.words.shape == self.positions.shape == self.build_positions.shape and self.positions.shape[1:] == (3, 3)

    def __len__(self):
        return len(self.positions)

    def triangles(self, count=None):
        """the 112-byte records: the position words exactly as `words` has them (no float conversion touches a NaN)"""
        n = len(self) if count is None else count
        tris = layout.pack_triangles(self.build_positions[:n], np.tile([0.0, 0.0, 1.0], (n, 3, 1)), np.zeros(n, int))
        raw = tris.view(np.uint8).reshape(n, 112).view("<u4")            # 28 words per record; a, b, c at words 0, 4, 8
        for v in range(3):
            raw[:, 4 * v:4 * v + 3] = self.words[:n, v]
        return tris


# ---------------------------------------------------------------- the law on bare vertex words (leaves) and on lists of leaves (unions)
def leaf_boxes(words, compare=None):
    """(min, max) words of the leaf boxes of (n, 3, 3) position words.  compare: None for the law; a function applied to the values
    the COMPARISONS see (the selected words stay the inputs') -- how a compare that flushes subnormals would decide."""
    v = np.ascontiguousarray(words, "<u4").view(F)
    see = (lambda x: x) if compare is None else compare

    def pick(x, y, low):
        with np.errstate(invalid="ignore"):
            sx, sy = see(x), see(y)
            take = ((sy < sx) | ((sy == sx) & np.signbit(y))) if low else ((sy > sx) | ((sy == sx) & ~np.signbit(y)))
        return np.where(take, y, x).astype(F)

    mn = pick(pick(v[:, 0], v[:, 1], True), v[:, 2], True)
    mx = pick(pick(v[:, 0], v[:, 1], False), v[:, 2], False)
    return mn.view("<u4"), mx.view("<u4")


def flush(x):
    """fp32 values with every subnormal replaced by the zero of its sign"""
    x = np.asarray(x, F)
    return np.where(np.abs(x) < np.finfo(F).tiny, np.copysign(F(0), x), x).astype(F)


def halved(n):
    """a tree over triangles 0 .. n - 1 that halves the index range at every node, children after their parents (boxes zero: to be
    fitted)"""
    nodes = np.zeros(2 * n - 1, layout.BVH_NODE)
    nodes["left"], nodes["right"], nodes["triangleIndex"] = -1, -1, -1
    work, nxt = [(0, 0, n)], 1
    while work:
        i, a, b = work.pop()
        if b - a == 1:
            nodes["isLeaf"][i], nodes["triangleIndex"][i] = 1, a
            continue
        mid = (a + b) // 2
        nodes["left"][i], nodes["right"][i] = nxt, nxt + 1
        work += [(nxt, a, mid), (nxt + 1, mid, b)]
        nxt += 2
    return nodes


# ---------------------------------------------------------------- zeros
_P, _N = (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0)
# the 20 triangles that are a zero of one sign throughout, as the groups the builder is to meet them in (each group is one cluster in
# space, its members in this order along the cluster's axis): pairs for the two-input case (children as given), triples for a sweep
# with a prefix box of two and a suffix box of two.  In index order they also pair up under halved(): (P P) (N N) (P N) (N P) ...
_GROUPS = ((_P, _P), (_N, _N), (_P, _N), (_N, _P), (_P, _N, _N), (_N, _P, _P), (_N, _N, _P), (_P, _P, _N))
BLOCK = 36                                         # triangles per component in zeros()


def _zero_block(k, rng, origin):
    """BLOCK triangles whose component k is made of zeros: 8 with a third value of either sign, the 8 sign patterns, the 20 of _GROUPS"""
    r = 0.25
    comp = []
    for j in range(8):                                       # two zeros and +r (the zeros are the minimum) or -r (the maximum)
        z = [-0.0 if (j >> b) & 1 else 0.0 for b in range(2)]
        z.insert(j % 3, r if j & 4 else -r)
        comp.append(tuple(z))
    comp += [tuple(-0.0 if (p >> v) & 1 else 0.0 for v in range(3)) for p in range(8)]
    along = [2.0 * j for j in range(16)]                     # the first 16: a row of their own
    at = 40.0
    for g in _GROUPS:                                        # each group a cluster far from the next, its members 0.6 apart
        comp += list(g)
        along += [at + 0.6 * m for m in range(len(g))]
        at += 12.0
    assert len(comp) == BLOCK
    a, b = (k + 1) % 3, (k + 2) % 3
    pos = np.zeros((BLOCK, 3, 3))
    pos[:, :, k] = comp
    pos[:, :, a] = origin[a] + np.array(along)[:, None] + rng.uniform(-0.2, 0.2, (BLOCK, 3))
    pos[:, :, b] = origin[b] + rng.normal(scale=0.3, size=(BLOCK, 3))
    return pos


@functools.lru_cache(maxsize=None)
def zeros():
    rng = np.random.default_rng(20)
    pos = np.concatenate([_zero_block(k, rng, origin=np.array([3.0, 5.0, 7.0]) * (k + 1)) for k in range(3)])
    pos = pos.astype(F).astype(np.float64)
    case = Case("zeros", pos, "108 triangles, 36 per component: that component is made of +0 / -0 in every sign pattern, with a third "
                "value of either sign in 8, and 20 one-signed triangles in pairs and triples of unlike sign, both orders")
    _assert_zeros(case)
    return case


def _assert_zeros(case):
    for k in range(3):
        block = case.words[BLOCK * k:BLOCK * (k + 1), :, k]
        assert {tuple(t) for t in block[8:16].tolist()} == {(a, b, c) for a in (PZ, NZ) for b in (PZ, NZ) for c in (PZ, NZ)}
        mn, mx = leaf_boxes(case.words[BLOCK * k:BLOCK * (k + 1)])
        zero_is_min = (mn[:8, k] == NZ) | (mn[:8, k] == PZ)
        assert 0 < zero_is_min.sum() < 8                     # a minimum in some, a maximum in the others
        # the law's result on a tree over the block's last 32 (the groups pair up under it): both zero words among the leaf AND the
        # internal bounds, low and high
        nodes = rr.refit_vectorised(halved(32), case.triangles()[BLOCK * k + 4:BLOCK * (k + 1)])
        leaf = nodes["isLeaf"] == 1
        for f in ("min", "max"):
            w = nodes[f][:, k].view("<u4")
            assert {PZ, NZ} <= set(w[leaf].tolist()) and {PZ, NZ} <= set(w[~leaf].tolist()), (k, f)
        # unions that meet a +0 child and a -0 child, in both orders
        lw, rw = nodes["min"][nodes["left"][~leaf], k].view("<u4"), nodes["min"][nodes["right"][~leaf], k].view("<u4")
        assert ((lw == PZ) & (rw == NZ)).any() and ((lw == NZ) & (rw == PZ)).any()


# ---------------------------------------------------------------- subnormals
@functools.lru_cache(maxsize=None)
def subnormals():
    rng = np.random.default_rng(21)
    values = np.array([0.0, -0.0] + [s * 2.0 ** e for e in (-149, -148, -140, -133, -127) for s in (1.0, -1.0)])
    n = 64
    pos = rng.normal(size=(n, 3, 3)) + rng.uniform(-4, 4, (n, 1, 3))
    for t in range(n):
        k = t % 3                                            # the component of this triangle that is subnormal or zero throughout
        pos[t, :, k] = values[rng.integers(0, len(values), 3)]
    # the decisions a flushing compare gets wrong, spelled out (component x of triangles 0, 3, 6, 9): the zero arrives AFTER the
    # subnormal it is to replace, or the subnormal after the zero it is not to replace
    pos[0, :, 0] = (2.0 ** -149, 0.0, 0.0)                   # min = +0 (flushed: equal, +0 does not win a minimum: stays 2^-149)
    pos[3, :, 0] = (-(2.0 ** -149), -0.0, -0.0)              # max = -0 (flushed: stays -2^-149)
    pos[6, :, 0] = (0.0, -0.0, 2.0 ** -127)                  # max = 2^-127 (flushed: +0 == +0, and +0 wins a maximum: still y; same)
    pos[9, :, 0] = (-0.0, 2.0 ** -140, -(2.0 ** -140))       # min = -2^-140, max = 2^-140
    case = Case("subnormals", pos, "64 triangles; one component of each holds only +-0 and +-2^e, e in -149 .. -127")
    _assert_subnormals(case)
    return case


def _assert_subnormals(case):
    v = case.words.view(F)
    tiny = np.finfo(F).tiny
    special = np.stack([v[t, :, t % 3] for t in range(len(case))])
    assert (np.abs(special) < tiny).all() and (special != 0).any() and (special == 0).any()
    assert (np.abs(special[special != 0]) >= F(2.0 ** -149)).all() and (np.abs(special) <= F(2.0 ** -127)).all()
    want = leaf_boxes(case.words)
    # a compare that sees flushed operands selects other words ...
    ftz = leaf_boxes(case.words, compare=flush)
    assert (ftz[0] != want[0]).any() and (ftz[1] != want[1]).any()
    assert want[0][0, 0] == PZ and ftz[0][0, 0] == 1 and want[1][3, 0] == NZ and ftz[1][3, 0] == 0x80000001
    # ... and so does the law on inputs that were flushed on the way in
    flushed = leaf_boxes(flush(v).view("<u4"))
    assert (flushed[0] != want[0]).any() and (flushed[1] != want[1]).any()


# ---------------------------------------------------------------- NaNs with payloads, infinities, FLT_MAX
@functools.lru_cache(maxsize=None)
def non_finite():
    rng = np.random.default_rng(22)
    n = 9 + 63
    base = rng.normal(size=(n, 3, 3)) + rng.uniform(-4, 4, (n, 1, 3))
    base = base.astype(F).astype(np.float64)
    words = base.astype(F).view("<u4").copy()
    inf = 0x7f800000
    fmax = int(np.array([FLT_MAX], F).view("<u4")[0])
    # 0: all nine coordinates NaN (three payloads); 1 - 8: +-inf and +-FLT_MAX, one vertex and all three
    words[0] = np.array(NAN_PAYLOADS, "<u4")[:, None]
    for j, w in enumerate((inf, inf | NZ, fmax, fmax | NZ)):
        words[1 + j, j % 3, :] = w                           # one vertex
        words[5 + j, :, j % 3] = w                           # one component of all three vertices
    # 9 .. 71: per component, NaN in a, b, c alone, in each pair, in all three -- once with each payload
    t = 9
    for payload in NAN_PAYLOADS:
        for k in range(3):
            for mask in range(1, 8):
                for vtx in range(3):
                    if (mask >> vtx) & 1:
                        words[t, vtx, k] = payload
                t += 1
    assert t == n
    with np.errstate(invalid="ignore"):                      # (the signalling NaN, converted)
        pos = words.view(F).astype(np.float64)
    case = Case("non_finite", pos, "72 triangles: one all NaN, +-inf and +-FLT_MAX in a vertex and in a component, and per component a NaN "
                "in a, b, c alone, in each pair and in all three, with payloads 0x7fc00001, 0xffc12345 and the signalling 0x7f800001",
                words=words, build_positions=base)
    _assert_non_finite(case)
    return case


def all_nan_leaves(case):
    """the triangles with a component that is NaN in all three vertices (their leaf box has a NaN there whatever the law)"""
    return np.flatnonzero(np.isnan(case.words.view(F)).all(1).any(1))


def _assert_non_finite(case):
    v = case.words.view(F)
    assert set(NAN_PAYLOADS) <= set(case.words[np.isnan(v)].tolist())
    assert np.isposinf(v).any() and np.isneginf(v).any() and (v == F(FLT_MAX)).any() and (v == -F(FLT_MAX)).any()
    assert np.isfinite(case.build_positions).all()
    assert len(all_nan_leaves(case)) == 1 + 9
    # the law only selects: every box word is one of the triangle's own nine words, NaN payloads included
    mn, mx = leaf_boxes(case.words)
    for box in (mn, mx):
        assert (box[:, None, :] == case.words).any(1).all()
    # the asymmetry: a NaN in a is kept (x), a NaN in b or c is dropped (y) -- in a chain with its leaves on one side, then the other,
    # an all-NaN leaf is x of one union and y of another
    tris = case.triangles(63)
    for shape in (chain_right(62), zigzag(62)):
        got = rr.refit_vectorised(shape, tris)
        assert np.isnan(got["min"][got["isLeaf"] != 1]).any() and not np.isnan(got["min"][got["isLeaf"] != 1]).all()


# ---------------------------------------------------------------- tree shapers
def _words(nodes):
    return np.ascontiguousarray(nodes).view(np.uint8).reshape(-1).copy().view("<u4").reshape(-1, 12)


def mirrored(nodes):
    """left and right of every internal node swapped: the indices stay valid (a child still follows its parent), the left child now
    has the higher index wherever it had the lower one, and every union takes its operands in the other order"""
    w = _words(nodes)
    inner = w[:, 7] != 1
    w[inner, 8], w[inner, 9] = w[inner, 9].copy(), w[inner, 8].copy()
    return w.reshape(-1).view(layout.BVH_NODE)


def _empty(count):
    nodes = np.zeros(count, layout.BVH_NODE)
    nodes["left"], nodes["right"], nodes["triangleIndex"] = -1, -1, -1
    return nodes


def chain_right(internal=62):
    """refit_reference.chain with its leaves on the RIGHT: internal nodes 0 .. k - 1 in a row, each with the rest of the chain on the
    left and the leaf of triangle j on the right (record k + j); the last one has the leaf of triangle k (record 2k) on the left, so
    there the left index is the higher one.  Triangles 0 .. k; boxes zero: the refit has to produce every one."""
    k = internal
    nodes = _empty(2 * k + 1)
    for j in range(k):
        nodes["left"][j] = j + 1 if j < k - 1 else 2 * k
        nodes["right"][j] = k + j
    nodes["isLeaf"][k:], nodes["triangleIndex"][k:] = 1, np.arange(k + 1)
    return nodes


def zigzag(internal=62):
    """refit_reference.chain's records (internal node 2j, its leaf 2j + 1, the rest 2j + 2) with the leaf on the left at even j and
    on the right at odd j, where left > right"""
    k = internal
    nodes = _empty(2 * k + 1)
    for j in range(k):
        i = 2 * j
        leaf, rest = i + 1, i + 2
        nodes["left"][i], nodes["right"][i] = (leaf, rest) if j % 2 == 0 else (rest, leaf)
        nodes["isLeaf"][leaf], nodes["triangleIndex"][leaf] = 1, j
    nodes["isLeaf"][2 * k], nodes["triangleIndex"][2 * k] = 1, k
    return nodes


def stamped(nodes, seed):
    """the same records with random 32-bit patterns in their two padding words, 3 and 11"""
    w = _words(nodes)
    rng = np.random.default_rng(seed)
    w[:, 3] = rng.integers(0, 1 << 32, len(w), dtype=np.uint64).astype("<u4")
    w[:, 11] = rng.integers(0, 1 << 32, len(w), dtype=np.uint64).astype("<u4")
    assert (w[:, 3] != 0).any() and (w[:, 11] != 0).any()
    return w.reshape(-1).view(layout.BVH_NODE)


def all_cases():
    return {"zeros": zeros(), "subnormals": subnormals(), "non_finite": non_finite()}
