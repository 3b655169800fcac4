"""A plain restatement of the node step of the two walks on quantised packets -- the 4-ary CWidePacket walk (kernel variant 13) and the
8-ary CW8Packet walk (variant 14) -- in numpy, on the BYTES a context uploads (mi3pt_host_walk_buffer).  No device, no test lives here.

  decode                the packets' fields; a slot's box in float64 (origin + index x 2^(e - 127): exact) and as the kernel's
                        plain-division path decodes it (one float32 fma per plane)
  Grouping              which node of the uploaded binary tree every packet and every slot stands for, recovered from the leaves
                        below it (lowest common ancestor) and checked to be a cut of that node's subtree
  fma32                 a correctly rounded float32 fma: formed in float64 (the product of two float32 values is exact there), rounded
                        once more, with the cases where that second rounding could differ detected and recomputed with fractions
  node_step             the quotients the kernels form: A = RN(RN(O - o) RN(1/d)), B = RN(cell RN(1/d)), near / far index by the sign of
                        the reciprocal, fma(q, B, A), key = max3, f = min3, cwide_hit = not(fma(key, 1 - 2^-20, -f) > 0) and not(f < 0);
                        rays on the plain-division path: the oracle's slab test on the kernel's decoded box
  walk                  top-down over the packets for a set of rays, no culling: a child is entered whenever its slot is accepted.
                        Per ray the leaves reached, and every (packet, slot) accepted with the slot EMPTY
"""
from fractions import Fraction

import numpy as np

f32, f64, u32 = np.float32, np.float64, np.uint32
REF_LEAF, REF_NONE = 0x80000000, 0xffffffff
SHRINK = f32(1.0 - 2.0 ** -20)
EPS = f32(1e-6)
LO, HI, BIG_D = f32(2.0 ** -70), f32(2.0 ** 60), f32(1048576.0)


# ---------------------------------------------------------------- a correctly rounded float32 fma

def _round_f32_exact(x):
    """Fraction -> float32, round to nearest, ties to even"""
    c = f32(float(x))
    cands = {float(c), float(np.nextafter(c, f32(np.inf))), float(np.nextafter(c, f32(-np.inf)))}
    best = None
    for v in cands:
        if not np.isfinite(v):
            continue
        err = abs(Fraction(v) - x)
        even = (int(np.array(v, f32).view(u32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even and not best[2]):
            best = (err, v, even)
    return f32(best[1])


def fma32_flagged(a, b, c):
    """(RN32(RN64(a b + c)), flagged): a, b, c float32 arrays (a b is exact in float64).  flagged: the float64 sum was inexact AND lies
    exactly half way between two float32 values (or below the float32 normal range): there, and only there, rounding twice can differ
    from rounding once."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    with np.errstate(all="ignore"):
        p = a.astype(f64) * b.astype(f64)
        c6 = c.astype(f64)
        s = p + c6
        bb = s - p
        err = (p - (s - bb)) + (c6 - bb)
        inexact = np.isfinite(s) & (err != 0)
        low = s.view(np.uint64) & np.uint64((1 << 29) - 1)
        tiny = np.abs(s) < 2.0 ** -126
        flagged = inexact & ((low == np.uint64(1 << 28)) | tiny)
        return s.astype(f32), flagged


def fma32(a, b, c):
    """the correctly rounded float32 fma(a, b, c), element-wise"""
    r, flagged = fma32_flagged(a, b, c)
    if flagged.any():
        a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
        r = r.copy()
        for i in zip(*np.nonzero(flagged)):
            r[i] = _round_f32_exact(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return r


def cwide_hit(key, f):
    """pt_kernels.hip: cwide_hit"""
    with np.errstate(invalid="ignore"):
        return ~(fma32(key, SHRINK, -f) > 0) & ~(f < 0)


# ---------------------------------------------------------------- decode

class Packets:
    """Decoded packets of one kind.  W slots per packet; per packet p and slot s:
    origin[p, ax] float32, exp[p, ax] (biased), qlo / qhi[p, s, ax] uint8, kind[p, s]: 0 empty, 1 internal, 2 leaf;
    child[p, s]: packet index (internal) ; tri[p, s]: triangle index (leaf); marked_empty[p, s]: the slot's box is (255, 0) on every axis.
    8-wide only: occupancy[p] (CW8Packet::tri bits 24-31), imask[p], rec_base[p], records (TriPacket64 as (n, 16) uint32)."""

    def __init__(self, W):
        self.W = W

    def cell(self):
        return np.ldexp(1.0, self.exp.astype(np.int64) - 127)                   # float64, exact

    def cell32(self):
        return (self.exp.astype(u32) << u32(23)).view(f32)

    def box64(self):
        """(lo, hi)[p, s, ax] in float64: exact (asserted)"""
        o, c = self.origin.astype(f64)[:, None, :], self.cell()[:, None, :]
        out = []
        for q in (self.qlo, self.qhi):
            t = q.astype(f64) * c
            s = o + t
            bb = s - o
            assert ((o - (s - bb)) + (t - bb) == 0).all(), "origin + index x cell is not exact in float64"
            out.append(s)
        return out

    def box32(self):
        """(lo, hi)[p, s, ax] as the kernel's plain-division path decodes them: one float32 fma per plane"""
        o, c = self.origin[:, None, :], self.cell32()[:, None, :]
        return fma32(self.qlo.astype(f32), c, o), fma32(self.qhi.astype(f32), c, o)


def decode_cwide(raw):
    """raw: (n, 64) uint8 CWidePacket records"""
    w = np.ascontiguousarray(raw).view(u32).reshape(-1, 16)
    P = Packets(4)
    P.origin = w[:, 0:3].copy().view(f32)
    meta = w[:, 3]
    P.exp = np.stack([(meta >> u32(8 * ax)) & u32(0xff) for ax in range(3)], 1)
    P.nchild = (meta >> u32(24)) & u32(7)
    sh = (np.arange(4, dtype=u32) * u32(8))[None, :, None]
    P.qlo = ((w[:, 4:7][:, None, :] >> sh) & u32(0xff)).astype(np.uint8)
    P.qhi = ((w[:, 7:10][:, None, :] >> sh) & u32(0xff)).astype(np.uint8)
    ref = w[:, 12:16]
    P.ref = ref
    P.kind = np.where(ref == u32(REF_NONE), 0, np.where((ref & u32(REF_LEAF)) != 0, 2, 1)).astype(np.int8)
    P.child = np.where(P.kind == 1, ref, 0).astype(np.int64)
    P.tri = np.where(P.kind == 2, ref & u32(0x7fffffff), 0).astype(np.int64)
    P.marked_empty = ((P.qlo == 255) & (P.qhi == 0)).all(2)
    return P


def decode_cw8(raw, raw_records):
    """raw: (n, 80) uint8 CW8Packet records; raw_records: (m, 64) uint8 TriPacket64 records"""
    w = np.ascontiguousarray(raw).view(u32).reshape(-1, 20)
    rec = np.ascontiguousarray(raw_records).view(u32).reshape(-1, 16)
    n = len(w)
    P = Packets(8)
    P.origin = w[:, 0:3].copy().view(f32)
    meta = w[:, 3]
    P.exp = np.stack([(meta >> u32(8 * ax)) & u32(0xff) for ax in range(3)], 1)
    P.imask = (meta >> u32(24)).astype(np.int64)
    P.qlo = np.zeros((n, 8, 3), np.uint8)
    P.qhi = np.zeros((n, 8, 3), np.uint8)
    for ax in range(3):
        for s in range(8):
            P.qlo[:, s, ax] = (w[:, 4 + 2 * ax + (s >> 2)] >> u32(8 * (s & 3))) & u32(0xff)
            P.qhi[:, s, ax] = (w[:, 10 + 2 * ax + (s >> 2)] >> u32(8 * (s & 3))) & u32(0xff)
    P.child_base = (w[:, 18] & u32(0xffffff)).astype(np.int64)
    P.rec_base = (w[:, 19] & u32(0xffffff)).astype(np.int64)
    P.occupancy = (w[:, 19] >> u32(24)).astype(np.int64)
    P.records = rec
    P.marked_empty = ((P.qlo == 255) & (P.qhi == 0)).all(2)
    bit = 1 << np.arange(8)
    internal = (P.imask[:, None] & bit) != 0
    P.kind = np.where(P.marked_empty, 0, np.where(internal, 1, 2)).astype(np.int8)
    below = np.array([[bin(int(m) & ((1 << s) - 1)).count("1") for s in range(8)] for m in P.imask]).reshape(n, 8)
    P.child = np.where(P.kind == 1, P.child_base[:, None] + below, 0)
    # the record index the triangle step forms for ANY slot: base + slot (an empty slot's too); its triangle where the index is inside
    P.rec_index = P.rec_base[:, None] + np.arange(8)[None, :]
    inside = P.rec_index < len(rec)
    P.rec_tri = np.where(inside, rec[np.minimum(P.rec_index, len(rec) - 1), 15] & u32(0x7fffffff), -1).astype(np.int64)
    P.tri = np.where(P.kind == 2, P.rec_tri, 0)
    return P


def record_is_inert(records, i):
    """build_cw8's filler: an empty box (1, -1) and a degenerate triangle"""
    r = records[i].view(f32)
    return bool((r[0:9] == 0).all() and (r[9:12] == 1).all() and (r[12:15] == -1).all() and records[i, 15] == 0)


# ---------------------------------------------------------------- the grouping: packets and slots as nodes of the uploaded tree

class Grouping:
    def __init__(self, nodes, P):
        n = len(nodes)
        left, right, leaf = nodes["left"].astype(np.int64), nodes["right"].astype(np.int64), nodes["isLeaf"] == 1
        parent, depth = np.full(n, -1, np.int64), np.zeros(n, np.int64)
        tin, tout = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for i in range(n):                                   # children have larger indices than their parent
            if not leaf[i]:
                for c in (left[i], right[i]):
                    assert c > i
                    parent[c], depth[c] = i, depth[i] + 1
        count = 0
        stack = [(0, False)]
        while stack:
            i, done = stack.pop()
            if done:
                tout[i] = count
                continue
            tin[i] = count
            if leaf[i]:
                count += 1
                tout[i] = count
            else:
                stack.append((i, True))
                stack.append((int(right[i]), False))
                stack.append((int(left[i]), False))
        leaf_of_tri = {}
        for i in np.flatnonzero(leaf):
            t = int(nodes["triangleIndex"][i])
            assert t not in leaf_of_tri
            leaf_of_tri[t] = int(i)
        self.parent, self.depth, self.tin, self.tout, self.leaf_of_tri, self.nleaves = parent, depth, tin, tout, leaf_of_tri, count

        def lca(a, b):
            while a != b:
                if depth[a] < depth[b]:
                    a, b = b, a
                a = int(parent[a])
            return a

        np_ = len(P.kind)
        self.slot_node = np.full((np_, P.W), -1, np.int64)
        self.packet_node = np.full(np_, -1, np.int64)
        for p in range(np_ - 1, -1, -1):                     # children have larger indices than their parent packet
            ks = []
            for s in range(P.W):
                if P.kind[p, s] == 2:
                    self.slot_node[p, s] = leaf_of_tri[int(P.tri[p, s])]
                elif P.kind[p, s] == 1:
                    c = int(P.child[p, s])
                    assert p < c < np_ and self.packet_node[c] >= 0, "a child packet that does not come after its parent"
                    self.slot_node[p, s] = self.packet_node[c]
                else:
                    continue
                ks.append(int(self.slot_node[p, s]))
            assert len(ks) >= 2 and len(set(ks)) == len(ks)
            x = ks[0]
            for k in ks[1:]:
                x = lca(x, k)
            self.packet_node[p] = x
            # the slots are a CUT of x's subtree: their leaf intervals tile x's
            iv = sorted((int(tin[k]), int(tout[k])) for k in ks)
            assert iv[0][0] == tin[x] and iv[-1][1] == tout[x] and all(iv[j][1] == iv[j + 1][0] for j in range(len(iv) - 1)), \
                f"packet {p}: its slots are not a cut of node {x}'s subtree"
        assert self.packet_node[0] == 0
        # every packet but the root is some slot's child exactly once
        kids = P.child[P.kind == 1]
        assert sorted(kids.tolist()) == list(range(1, np_))


def _exact_sum(a, b):
    s = a + b
    bb = s - a
    assert ((a - (s - bb)) + (b - bb) == 0).all(), "a sum that is not exact in float64"
    return s


def containment(nodes, P, G):
    """ok[occupied slots, 3]: the decoded box contains the child's uploaded box with a margin of at least one whole cell on both sides of
    the axis -- lo + cell <= child.min and hi - cell >= child.max, every term exact in float64"""
    lo, hi = P.box64()
    occ = P.kind != 0
    nd = np.where(occ, G.slot_node, 0)
    cmin, cmax = nodes["min"].astype(f64)[nd], nodes["max"].astype(f64)[nd]
    cell = np.broadcast_to(P.cell()[:, None, :], lo.shape)
    return ((_exact_sum(lo, cell) <= cmin) & (_exact_sum(hi, -cell) >= cmax))[occ]


# ---------------------------------------------------------------- the node step

def ray_slow(rays):
    """ray_prepare().flags & 8 (pt_kernels.hip): the ray takes the plain-division test"""
    o, d = rays[:, :3], rays[:, 3:]
    ad = np.abs(d)
    with np.errstate(invalid="ignore"):
        safe = (o == 0) | ((np.abs(o) >= LO) & (np.abs(o) <= HI))
        return (ad < EPS).any(1) | (ad > BIG_D).any(1) | ~safe.all(1) | np.isnan(d).any(1)


class Rays:
    def __init__(self, rays):
        self.rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
        self.o, self.d = self.rays[:, :3], self.rays[:, 3:]
        with np.errstate(all="ignore"):
            self.inv = (f32(1.0) / self.d).astype(f32)          # RN(1 / d)
        self.slow = ray_slow(self.rays)


def node_step(P, p, R, idx, orc, box32=None):
    """accept[len(idx), W]: the box decision of packet p's node step for the rays R[idx], before any mask"""
    W = P.W
    out = np.zeros((len(idx), W), bool)
    fast = ~R.slow[idx]
    if fast.any():
        k = idx[fast]
        with np.errstate(all="ignore"):
            A = ((P.origin[p][None, :] - R.o[k]).astype(f32) * R.inv[k]).astype(f32)          # two roundings (no contraction)
            B = (P.cell32()[p][None, :] * R.inv[k]).astype(f32)
        neg = R.inv[k] < 0
        qlo, qhi = P.qlo[p].astype(f32)[None, :, :], P.qhi[p].astype(f32)[None, :, :]          # [1, W, 3]
        near = np.where(neg[:, None, :], qhi, qlo)
        far = np.where(neg[:, None, :], qlo, qhi)
        tn = fma32(near, B[:, None, :], A[:, None, :])
        tf = fma32(far, B[:, None, :], A[:, None, :])
        out[fast] = cwide_hit(tn.max(2), tf.min(2))
    if (~fast).any():
        k = idx[~fast]
        lo, hi = box32 if box32 is not None else P.box32()
        for s in range(W):
            out[~fast, s] = orc.ray_aabb_n(R.rays[k], np.repeat(lo[p, s][None], len(k), 0), np.repeat(hi[p, s][None], len(k), 0))
    return out


class WalkResult:
    pass


def walk(P, rays, ntris, orc, apply_occupancy=False):
    """Top-down over the packets, no culling.  apply_occupancy (8-wide): AND the hit mask with CW8Packet::tri's occupancy mask, as the
    kernel does.  Returns reached[ray, triangle] (bool), empty[ray] (accepted empty slots per ray), events: list of (packet, slot, rays)
    with the slot empty and accepted, and (8-wide) records: the set of (packet, slot, record index) the triangle step would read."""
    R = rays if isinstance(rays, Rays) else Rays(rays)
    n = len(R.rays)
    np_ = len(P.kind)
    active = [None] * np_
    active[0] = np.arange(n)
    box32 = P.box32() if R.slow.any() else None
    res = WalkResult()
    res.reached = np.zeros((n, ntris), bool)
    res.empty = np.zeros(n, np.int64)
    res.events = []
    res.records = set()
    res.steps = 0
    for p in range(np_):                                     # parents before children
        idx = active[p]
        if idx is None or len(idx) == 0:
            continue
        active[p] = None
        res.steps += len(idx)
        acc = node_step(P, p, R, idx, orc, box32)
        if apply_occupancy:
            acc &= ((int(P.occupancy[p]) >> np.arange(P.W)) & 1 != 0)[None, :]
        for s in range(P.W):
            hit = idx[acc[:, s]]
            if len(hit) == 0:
                continue
            kind = P.kind[p, s]
            if kind == 1:
                c = int(P.child[p, s])
                active[c] = hit if active[c] is None else np.union1d(active[c], hit)
            elif kind == 2:
                res.reached[hit, int(P.tri[p, s])] = True
                if P.W == 8:
                    res.records.add((p, s, int(P.rec_index[p, s])))
            else:
                res.empty[hit] += 1
                res.events.append((p, s, hit))
                if P.W == 8:                                 # not internal: the 8-wide triangle step reads record base + slot
                    res.records.add((p, s, int(P.rec_index[p, s])))
    return res


def leaves_passing(orc, nodes, rays):
    """passes[ray, triangle]: the oracle's slab test of every leaf's OWN box (raytrace.wgsl:118-152), ray by ray"""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    leaves = np.flatnonzero(nodes["isLeaf"] == 1)
    ntris = int(nodes["triangleIndex"][leaves].max()) + 1
    out = np.zeros((len(rays), ntris), bool)
    mn, mx = nodes["min"].astype(f32), nodes["max"].astype(f32)
    chunk = max(1, 4_000_000 // max(len(rays), 1))
    for a in range(0, len(leaves), chunk):
        lv = leaves[a:a + chunk]
        r = np.tile(rays, (len(lv), 1))
        got = orc.ray_aabb_n(r, np.repeat(mn[lv], len(rays), 0), np.repeat(mx[lv], len(rays), 0)).reshape(len(lv), len(rays))
        out[:, nodes["triangleIndex"][lv]] = got.T
    return out


def load(capi, nodes, tris, collapse=-1):
    """(4-ary packets, 8-wide packets) decoded from the bytes a context would upload"""
    c4 = decode_cwide(capi.host_walk_buffer(nodes, tris, capi.WALK_CWIDE, collapse))
    c8 = decode_cw8(capi.host_walk_buffer(nodes, tris, capi.WALK_CW8, collapse), capi.host_walk_buffer(nodes, tris, capi.WALK_TRI8, collapse))
    return c4, c8
