"""Inputs of the walk probes (tests/test_gpu_walk_probes.py, tests/test_walk_probe_inputs.py): (ray, box) pairs, (ray, triangle)
pairs and rays against whole scenes, at the places where such code goes wrong.  Plain numpy, fixed seeds, no device.

Every family is a dict entry  name -> arrays;  a family stays at or below a few ten-thousand pairs.  The ordinary / corner / flat box
pairs and the grazing triangle pairs come from the generators tests/test_slab_filter.py and tests/test_cull_bound.py already have."""
import numpy as np

import test_cull_bound as tcb
import test_slab_filter as tsf

f32 = np.float32
EPS = f32(1e-6)
LO, HI = f32(2.0 ** -70), f32(2.0 ** 60)          # the fast path's magnitude guards (pt_kernels.hip: safe_magnitude)
BIG_D = f32(1048576.0)                            # ... and |d| <= 2^20


def _up(x, k=1):
    x = np.asarray(x, f32).copy()
    for _ in range(k):
        x = np.nextafter(x, f32(np.inf))
    return x


def _down(x, k=1):
    x = np.asarray(x, f32).copy()
    for _ in range(k):
        x = np.nextafter(x, f32(-np.inf))
    return x


def _unit(v):
    with np.errstate(all="ignore"):            # (a zero vector gives a NaN direction: an input like any other)
        return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rays(o, d):
    return np.ascontiguousarray(np.concatenate([np.asarray(o, f32), np.asarray(d, f32)], 1), f32)


# ---------------------------------------------------------------- host-side rules, transcribed (classification only)

def safe_magnitude(v):
    a = np.abs(v)
    with np.errstate(invalid="ignore"):
        return (v == 0) | ((a >= LO) & (a <= HI))


def box_unsafe_host(mn, mx):
    """node_box_safe (csrc/pt_host_wide.cpp), negated: a coordinate that is neither 0 nor within [2^-70, 2^60] (NaN included)."""
    return ~(safe_magnitude(np.asarray(mn, f32)).all(1) & safe_magnitude(np.asarray(mx, f32)).all(1))


def ray_flags(rays):
    """ray_prepare().flags (csrc/pt_kernels.hip): 8 = the ray takes the plain-division test."""
    o, d = rays[:, :3], rays[:, 3:]
    ad = np.abs(d)
    with np.errstate(invalid="ignore"):
        slow = (ad < EPS).any(1) | (ad > BIG_D).any(1) | ~safe_magnitude(o).all(1) | np.isnan(d).any(1)
    return np.where(slow, 8, 0)


def undecided(rays, mn, mx):
    """pairs on the fast path that the filtered slab test leaves to the exact one (tests/test_slab_filter.py: filtered)"""
    with np.errstate(all="ignore"):
        decided, _ = tsf.filtered(rays[:, :3], rays[:, 3:], np.asarray(mn, f32), np.asarray(mx, f32))
    return ~decided & (ray_flags(rays) == 0) & ~box_unsafe_host(mn, mx)


# ---------------------------------------------------------------- (ray, box) pairs

def _aimed(rng, mn, mx, spread, inside=0.6):
    """origins around the boxes, directions at a point of the box (a share `inside`) or past it"""
    n = len(mn)
    mn64, mx64 = mn.astype(np.float64), mx.astype(np.float64)
    ext = np.maximum(mx64 - mn64, 1e-3 * np.maximum(np.abs(mn64), 1e-30))
    tgt = mn64 + rng.random((n, 3)) * (mx64 - mn64)
    off = rng.random(n) > inside
    tgt[off] += (rng.normal(size=(int(off.sum()), 3)) * 2.0) * ext[off]
    o = tgt + _unit(rng.normal(size=(n, 3))) * spread * np.linalg.norm(ext, axis=1, keepdims=True) * rng.uniform(1.5, 6.0, (n, 1))
    o = o.astype(f32)
    d = _unit(tgt - o.astype(np.float64)).astype(f32)
    return o, d


def _ordinary(rng, n):
    """tests/test_slab_filter.py: test_ordinary_pairs_agree_and_are_rarely_undecided, at n pairs per scale.  Its random directions hit
    3 % of the boxes; a part of the rays here is re-aimed at a random point well INSIDE its box where every extent of the box is at
    least 1e-3 of the distance (an interval of ordinary length: 2^11 times the filter's band), so that both answers are well
    represented."""
    parts = []
    for scale in (1.0, 5.0, 300.0):
        mn, mx = tsf._boxes(rng, n, scale)
        o = (rng.uniform(-1, 1, (n, 3)) * 2 * scale).astype(f32)
        d = tsf._dirs(rng, n)
        ext = (mx.astype(np.float64) - mn.astype(np.float64)).min(1)
        tgt = mn.astype(np.float64) + rng.uniform(0.2, 0.8, (n, 3)) * (mx.astype(np.float64) - mn.astype(np.float64))
        aim = (rng.random(n) < 0.4) & (ext >= 1e-3 * np.linalg.norm(tgt - o, axis=1))      # (not at a box that is thin as seen from the origin)
        d[aim] = _unit(tgt[aim] - o[aim].astype(np.float64)).astype(f32)
        parts.append((_rays(o, d), mn, mx))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _corners_edges_faces(rng, n):
    """tests/test_slab_filter.py: test_rays_through_corners_edges_and_faces, at n pairs per combination"""
    parts = []
    for scale in (1.0, 40.0):
        mn, mx = tsf._boxes(rng, n, scale)
        mn64, mx64 = mn.astype(np.float64), mx.astype(np.float64)
        pick = rng.integers(0, 3, (n, 3))
        lam = rng.random((n, 3))
        target = np.where(pick == 0, mn64, np.where(pick == 1, mx64, mn64 + lam * (mx64 - mn64)))
        for origin_on_face in (False, True):
            if origin_on_face:
                o64 = mn64 + rng.random((n, 3)) * (mx64 - mn64)
                ax = rng.integers(0, 3, n)
                side = rng.random(n) < 0.5
                o64[np.arange(n), ax] = np.where(side, mn64[np.arange(n), ax], mx64[np.arange(n), ax])
            else:
                o64 = target + rng.normal(0, 1, (n, 3)) * scale * 3
            o = o64.astype(f32)
            d64 = target - o.astype(np.float64)
            nrm = np.linalg.norm(d64, axis=1, keepdims=True)
            good = nrm[:, 0] > 0
            d = (d64[good] / nrm[good]).astype(f32)
            for f in (f32(1), f32(-1), f32(1.7)):
                parts.append((_rays(o[good], d * f), mn[good], mx[good]))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _flat(rng, n):
    """boxes flat on one, two or three axes; half of the rays aimed into the flat face, half past it"""
    mn, mx = tsf._boxes(rng, n, 2.5)
    flat = rng.integers(1, 8, n)
    for k in range(3):
        sel = (flat >> k) & 1 == 1
        mx[sel, k] = mn[sel, k]
    o = (rng.uniform(-1, 1, (n, 3)) * 4).astype(f32)
    tgt = mn.astype(np.float64) + rng.random((n, 3)) * (mx.astype(np.float64) - mn.astype(np.float64))
    miss = rng.random(n) < 0.4
    tgt[miss] += rng.normal(size=(int(miss.sum()), 3)) * 0.05
    d = _unit(tgt - o.astype(np.float64)).astype(f32)
    return _rays(o, d), mn, mx


def _origin_inside(rng, n):
    """origins inside the box and exactly on a face, going anywhere; a third of the boxes lie behind a start just outside"""
    mn, mx = tsf._boxes(rng, n, 3.0)
    o = (mn.astype(np.float64) + rng.random((n, 3)) * (mx.astype(np.float64) - mn.astype(np.float64))).astype(f32)
    o = np.clip(o, mn, mx)
    face = rng.random(n) < 0.5
    ax = rng.integers(0, 3, n)
    idx = np.arange(n)
    o[idx[face], ax[face]] = np.where(rng.random(int(face.sum())) < 0.5, mn[idx[face], ax[face]], mx[idx[face], ax[face]])
    d = tsf._dirs(rng, n)
    out = rng.random(n) < 0.35                     # stepped outside along the direction: the box lies behind
    step = (np.linalg.norm((mx - mn).astype(np.float64), axis=1, keepdims=True) * 1.01).astype(f32)
    o[out] = o[out] + d[out] * step[out]
    return _rays(o, d), mn, mx


def _far(rng, n):
    """boxes 1e3 to 1e6 from the origin, of size 1e-2 .. 10, rays from nearby and from the origin's neighbourhood"""
    dist = 10 ** rng.uniform(3, 6, (n, 1))
    c = _unit(rng.normal(size=(n, 3))) * dist
    h = np.abs(rng.normal(size=(n, 3))) * 10 ** rng.uniform(-2, 1, (n, 1))
    mn, mx = (c - h).astype(f32), (c + h).astype(f32)
    o, d = _aimed(rng, mn, mx, 1.0, inside=0.55)
    home = rng.random(n) < 0.5
    o[home] = rng.normal(size=(int(home.sum()), 3)).astype(f32)
    tgt = mn.astype(np.float64) + rng.random((n, 3)) * (mx.astype(np.float64) - mn.astype(np.float64))
    jit = rng.random(n) < 0.45
    tgt[jit] += rng.normal(size=(int(jit.sum()), 3)) * 2.0 * h[jit]
    d[home] = _unit(tgt[home] - o[home].astype(np.float64)).astype(f32)
    return _rays(o, d), mn, mx


def _axis_values(rng, n, values):
    """one component of the direction from `values` (both signs), the origin of that axis on a plane / inside the slab / outside"""
    mn, mx = tsf._boxes(rng, n, 2.0)
    o, d = _aimed(rng, mn, mx, 1.0, inside=0.8)
    k = rng.integers(0, 3, n)
    idx = np.arange(n)
    vals = np.asarray(values, f32)
    d[idx, k] = vals[rng.integers(0, len(vals), n)] * rng.choice([-1, 1], n).astype(f32)
    where = rng.integers(0, 4, n)                   # 0 on min plane, 1 on max plane, 2 inside the slab, 3 outside
    lam = rng.random(n).astype(f32)
    inside = (mn[idx, k] + lam * (mx[idx, k] - mn[idx, k])).astype(f32)
    inside = np.clip(inside, mn[idx, k], mx[idx, k])
    outside = np.where(rng.random(n) < 0.5, _down(mn[idx, k], 1), _up(mx[idx, k], 1))
    far_out = rng.random(n) < 0.5
    outside = np.where(far_out, outside + np.sign(outside - inside) * f32(0.5), outside).astype(f32)
    o[idx, k] = np.select([where == 0, where == 1, where == 2], [mn[idx, k], mx[idx, k], inside], outside)
    return _rays(o, d), mn, mx


def _eps_dirs(rng, n):
    return _axis_values(rng, n, [EPS, _down(EPS), _up(EPS), _down(EPS, 2), _up(EPS, 2)])


def _zero_dirs(rng, n):
    r, mn, mx = _axis_values(rng, n, [f32(0.0)])            # (both signs of zero: _axis_values multiplies by +-1)
    two = rng.random(n) < 0.25                              # a second parallel axis, its origin inside the slab
    k2 = rng.integers(0, 3, n)
    idx = np.arange(n)[two]
    r[idx, 3 + k2[two]] = f32(-0.0)
    r[idx, k2[two]] = ((mn[idx, k2[two]].astype(np.float64) + mx[idx, k2[two]]) / 2).astype(f32)
    return r, mn, mx


def _big_dirs(rng, n):
    """|d_k| on both sides of 2^20 (the other components ordinary: the direction is far from normalised)"""
    mn, mx = tsf._boxes(rng, n, 2.0)
    o, d = _aimed(rng, mn, mx, 1.0, inside=0.75)
    k = rng.integers(0, 3, n)
    idx = np.arange(n)
    vals = np.array([BIG_D, _down(BIG_D), _up(BIG_D), BIG_D * 2, BIG_D / 2], f32)
    s = vals[rng.integers(0, len(vals), n)] / np.abs(d[idx, k])
    ok = np.isfinite(s) & (np.abs(d[idx, k]) > 1e-3)
    s = np.where(ok, s, f32(1)).astype(f32)
    d = (d * s[:, None]).astype(f32)                 # the whole direction scaled: still aimed at the box
    exact = ok & (rng.random(n) < 0.6)
    d[idx[exact], k[exact]] = np.sign(d[idx[exact], k[exact]]) * vals[rng.integers(0, 3, int(exact.sum()))]
    return _rays(o, d), mn, mx


def _guard_magnitudes(rng, n):
    """origin and box coordinates on both sides of 2^-70 and of 2^60"""
    parts = []
    h = n // 2
    # small: a box around the origin whose planes sit at +-2^-70 and its neighbours, rays from ordinary distances and from origins
    # whose one component is such a value
    edge = np.array([LO, _down(LO), _up(LO), LO * 2, LO / 2, 0.0], f32)
    mn = -edge[rng.integers(0, len(edge), (h, 3))]
    mx = edge[rng.integers(0, len(edge), (h, 3))]
    big = rng.random((h, 3)) < 0.5                          # ... or an ordinary extent on that axis
    mn = np.where(big, -rng.uniform(0.1, 1, (h, 3)), mn).astype(f32)
    mx = np.where(big, rng.uniform(0.1, 1, (h, 3)), mx).astype(f32)
    o = (_unit(rng.normal(size=(h, 3))) * rng.uniform(0.5, 3, (h, 1))).astype(f32)
    tgt = rng.normal(size=(h, 3)) * 0.3 * (rng.random((h, 1)) < 0.5)      # at the origin (through the box) or around it
    d = _unit(tgt - o.astype(np.float64)).astype(f32)
    oe = rng.random((h, 3)) < 0.3
    o = np.where(oe, edge[rng.integers(0, len(edge), (h, 3))] * rng.choice([-1, 1], (h, 3)), o).astype(f32)
    parts.append((_rays(o, d), mn, mx))
    # large: coordinates at 2^60 and its neighbours
    h = n - h
    edge = np.array([HI, _down(HI), _up(HI), HI * 2, HI / 2], f32)
    c = edge[rng.integers(0, len(edge), (h, 3))] * rng.choice([-1, 1], (h, 3)).astype(f32)
    ext = (np.abs(c) * rng.uniform(1e-6, 0.5, (h, 3))).astype(f32)
    mn, mx = (c - ext).astype(f32), (c + ext).astype(f32)
    on = rng.random((h, 3)) < 0.5                            # the outer plane exactly on the value
    mx = np.where(on & (c > 0), c, mx).astype(f32)
    mn = np.where(on & (c < 0), c, mn).astype(f32)
    far = rng.random(h) < 0.5
    o = np.where(far[:, None], c * rng.uniform(0.2, 0.9, (h, 3)), rng.normal(size=(h, 3))).astype(f32)
    oe = rng.random((h, 3)) < 0.15
    o = np.where(oe, edge[rng.integers(0, len(edge), (h, 3))] * np.sign(c), o).astype(f32)
    tgt = mn.astype(np.float64) + rng.random((h, 3)) * (mx.astype(np.float64) - mn.astype(np.float64))
    miss = rng.random(h) < 0.4
    tgt[miss] += rng.normal(size=(int(miss.sum()), 3)) * 3.0 * ext[miss]
    d = _unit(tgt - o.astype(np.float64)).astype(f32)
    parts.append((_rays(o, d), mn, mx))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _subnormals(rng, n):
    """boxes and origins with subnormal coordinates; directions ordinary, and a share with a subnormal component"""
    tiny = np.ldexp(rng.uniform(0.5, 1.0, (n, 3)), rng.integers(-149, -126, (n, 3))).astype(f32)
    mn, mx = (-tiny).astype(f32), np.ldexp(rng.uniform(0.5, 1.0, (n, 3)), rng.integers(-149, -126, (n, 3))).astype(f32)
    wide = rng.random((n, 3)) < 0.4
    mn = np.where(wide, f32(-0.5), mn).astype(f32)
    mx = np.where(wide, f32(0.5), mx).astype(f32)
    o = (_unit(rng.normal(size=(n, 3))) * rng.uniform(0.5, 2, (n, 1))).astype(f32)
    so = rng.random((n, 3)) < 0.3
    o = np.where(so, tiny * rng.choice([-1, 1], (n, 3)), o).astype(f32)
    tgt = rng.normal(size=(n, 3)) * 0.2 * (rng.random((n, 1)) < 0.45)
    d = tgt - o.astype(np.float64)
    d = _unit(np.where(np.abs(d).sum(1, keepdims=True) > 0, d, 1.0)).astype(f32)
    sd = rng.random(n) < 0.2
    d[sd, rng.integers(0, 3, int(sd.sum()))] = np.ldexp(0.75, -140)
    return _rays(o, d), mn, mx


def _all_ones(rng, n):
    """every significand all ones (0x..7fffff): directions, origins and box planes -- quotients that round at the last bit"""
    def ones(shape, elo, ehi):
        e = rng.integers(elo + 127, ehi + 127, shape).astype(np.uint32)
        s = rng.integers(0, 2, shape).astype(np.uint32)
        return ((s << np.uint32(31)) | (e << np.uint32(23)) | np.uint32(0x7fffff)).view(f32)
    mn, mx = tsf._boxes(rng, n, 2.0)
    o, d = _aimed(rng, mn, mx, 1.0, inside=0.65)
    m = rng.random((n, 3)) < 0.7
    d = np.where(m, (d.view(np.uint32) | np.uint32(0x7fffff)).view(f32), d)
    m = rng.random((n, 3)) < 0.5
    o = np.where(m, (o.view(np.uint32) | np.uint32(0x7fffff)).view(f32), o)
    lo = np.minimum(ones((n, 3), -3, 2), mx)
    m = rng.random((n, 3)) < 0.3
    mn = np.where(m & (lo <= mx), lo, mn).astype(f32)
    return _rays(o, d), mn, mx


def _nonfinite(rng, n, what):
    """NaN / +-inf in the origin, the direction or the box (one to three components of one of them)"""
    mn, mx = tsf._boxes(rng, n, 2.0)
    o, d = _aimed(rng, mn, mx, 1.0, inside=0.8)
    vals = np.array([np.nan] if what == "nan" else [np.inf, -np.inf], f32)
    who = rng.integers(0, 4, n)
    for j, arr in enumerate((o, d, mn, mx)):
        m = (who == j)[:, None] & (rng.random((n, 3)) < 0.45)
        arr[m] = vals[rng.integers(0, len(vals), int(m.sum()))]
    return _rays(o, d), mn, mx


def _zero_direction(rng, n):
    """d = (+-0, +-0, +-0): every axis parallel -- the box passes iff it holds the origin"""
    mn, mx = tsf._boxes(rng, n, 2.0)
    o = (mn.astype(np.float64) + rng.uniform(-0.4, 1.4, (n, 3)) * (mx.astype(np.float64) - mn.astype(np.float64))).astype(f32)
    d = np.where(rng.random((n, 3)) < 0.5, f32(0.0), f32(-0.0)).astype(f32)
    return _rays(o, d), mn, mx


def _unnormalised(rng, n):
    r, mn, mx = _corners_edges_faces(rng, max(1, n // 24))
    r2, mn2, mx2 = _ordinary(rng, n // 6)
    r, mn, mx = np.concatenate([r, r2]), np.concatenate([mn, mn2]), np.concatenate([mx, mx2])
    s = np.where(rng.random(len(r)) < 0.5, f32(2.0 ** 10), f32(2.0 ** -10)).astype(f32)
    r[:, 3:] *= s[:, None]
    return r, mn, mx


BOX_FAMILIES = {
    # name: (generator, pairs, seed)
    "ordinary": (lambda rng: _ordinary(rng, 10000), 101),
    "corners edges faces": (lambda rng: _corners_edges_faces(rng, 2000), 102),
    "flat boxes": (lambda rng: _flat(rng, 20000), 103),
    "origin inside or on a face": (lambda rng: _origin_inside(rng, 20000), 104),
    "far from the origin": (lambda rng: _far(rng, 20000), 105),
    "direction at EPSILON": (lambda rng: _eps_dirs(rng, 20000), 106),
    "direction +-0": (lambda rng: _zero_dirs(rng, 20000), 107),
    "direction at 2^20": (lambda rng: _big_dirs(rng, 20000), 108),
    "magnitudes at 2^-70 and 2^60": (lambda rng: _guard_magnitudes(rng, 20000), 109),
    "subnormals": (lambda rng: _subnormals(rng, 20000), 110),
    "all-ones significands": (lambda rng: _all_ones(rng, 20000), 111),
    "NaN": (lambda rng: _nonfinite(rng, 12000, "nan"), 112),
    "inf": (lambda rng: _nonfinite(rng, 12000, "inf"), 113),
    "d = 0": (lambda rng: _zero_direction(rng, 8000), 114),
    "un-normalised": (lambda rng: _unnormalised(rng, 24000), 115),
}
ORDINARY_BOX_FAMILY = "ordinary"          # the family whose share of undecided pairs is bounded (tests/test_slab_filter.py: < 1e-4)
UNDECIDED_BOUND = 1e-4


def box_pairs():
    """name -> (rays[n, 6], mn[n, 3], mx[n, 3]) float32"""
    out = {}
    for name, (gen, seed) in BOX_FAMILIES.items():
        r, mn, mx = gen(np.random.default_rng(seed))
        out[name] = tuple(np.ascontiguousarray(v, f32) for v in (r, mn, mx))
    return out


# ---------------------------------------------------------------- (ray, triangle) pairs

def _tri_grazing(rng, n):
    o, d, a, b, c = tcb._adversarial_batch(rng, n)
    return _rays(o, d), np.concatenate([a, b, c], 1)


def _random_tris(rng, n):
    a = rng.normal(size=(n, 3)) * 10 ** rng.uniform(-1, 1.5, (n, 1))
    size = 10 ** rng.uniform(-2, 0.5, (n, 1))
    b = a + _unit(rng.normal(size=(n, 3))) * size
    c = a + _unit(rng.normal(size=(n, 3))) * size * rng.uniform(0.2, 1.0, (n, 1))
    return a.astype(f32), b.astype(f32), c.astype(f32)


def _through(rng, a, b, c, lam1, lam2, jitter_share=0.45):
    """rays through the point a + lam1 (b - a) + lam2 (c - a) (formed in float64 from the float32 vertices), a share of them moved
    off it by a few 1e-7 of the triangle's size (onto either side of the edge)"""
    n = len(a)
    a6, b6, c6 = (x.astype(np.float64) for x in (a, b, c))
    p = a6 + lam1[:, None] * (b6 - a6) + lam2[:, None] * (c6 - a6)
    size = np.linalg.norm(b6 - a6, axis=1, keepdims=True)
    jit = rng.random(n) < jitter_share
    p[jit] += rng.normal(size=(int(jit.sum()), 3)) * size[jit] * 10 ** rng.uniform(-7.5, -5, (int(jit.sum()), 1))
    nrm = _unit(np.cross(b6 - a6, c6 - a6) + 1e-300)
    d = _unit(nrm * rng.choice([-1, 1], (n, 1)) * rng.uniform(0.2, 1, (n, 1)) + _unit(rng.normal(size=(n, 3))) * 0.6)
    t0 = 10 ** rng.uniform(-1, 1.5, (n, 1))
    # a power-of-two distance on a part: o = p - t0 d rounds less
    t0 = np.where(rng.random((n, 1)) < 0.5, 2.0 ** np.round(np.log2(t0)), t0)
    o = (p - d * t0).astype(f32)
    d = _unit(p - o.astype(np.float64)).astype(f32)       # re-aimed from the rounded origin
    return _rays(o, d), np.concatenate([a, b, c], 1)


def _tri_vertices_edges(rng, n):
    a, b, c = _random_tris(rng, n)
    kind = rng.integers(0, 6, n)
    lam = rng.random(n)
    l1 = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [0.0, 1.0, 0.0, lam, 0.0], lam)         # a, b, c, edge ab (v = 0), edge ac (u = 0), edge bc
    l2 = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [0.0, 0.0, 1.0, 0.0, lam], 1.0 - lam)
    r, g = _through(rng, a, b, c, l1, l2)
    # rays ALONG an edge (in the triangle's plane: the determinant vanishes) on a part
    along = rng.random(n) < 0.15
    m = int(along.sum())
    e = (b[along].astype(np.float64) - a[along].astype(np.float64))
    r[along, 3:] = _unit(e).astype(f32)
    r[along, :3] = (a[along].astype(np.float64) - e * rng.uniform(0.5, 2, (m, 1))).astype(f32)
    return r, g


def _tri_exact_edges(rng, n):
    """the unit right triangle in a coordinate plane, scaled by a power of two, and rays whose products are exact: u = 0, v = 0,
    u + v = 1 and their float neighbours, exactly"""
    s = (2.0 ** rng.integers(-3, 4, n)).astype(f32)
    perm = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]])[rng.integers(0, 3, n)]
    idx = np.arange(n)[:, None]
    A = np.zeros((n, 3), f32); B = np.zeros((n, 3), f32); C = np.zeros((n, 3), f32)
    B[:, 0] = s; C[:, 1] = s
    # target point in the plane: (x, y) on the lattice of eighths, a share moved by one ulp
    gx = rng.integers(0, 9, n); gy = rng.integers(0, 9, n)
    on_hyp = rng.random(n) < 0.3
    gy = np.where(on_hyp, 8 - gx, gy)
    x = (gx / 8.0).astype(f32) * s; y = (gy / 8.0).astype(f32) * s
    nudge = rng.integers(-1, 2, (n, 2))
    x = np.where(nudge[:, 0] > 0, _up(x), np.where(nudge[:, 0] < 0, _down(x), x)).astype(f32)
    y = np.where(nudge[:, 1] > 0, _up(y), np.where(nudge[:, 1] < 0, _down(y), y)).astype(f32)
    # straight down the normal (d = (0, 0, -1) scaled by a power of two) from a power-of-two height: every product exact
    h = (2.0 ** rng.integers(-2, 3, n)).astype(f32)
    o = np.stack([x, y, h], 1)
    d = np.zeros((n, 3), f32); d[:, 2] = -(2.0 ** rng.integers(-2, 3, n)).astype(f32)
    up = rng.random(n) < 0.3                               # from below, going up
    o[up, 2] *= -1; d[up, 2] *= -1
    P = lambda v: np.take_along_axis(v, np.argsort(perm, 1), 1)      # the same permutation of the axes for all of them
    return _rays(P(o), P(d)), np.concatenate([P(A), P(B), P(C)], 1)


def _tri_plane_origins(rng, n):
    """origins in the triangle's plane and within a few ulp of it; t around EPSILON: o = p - t0 d with t0 = 0, a few ulp of |p|,
    EPSILON and its neighbours -- on axis-aligned triangles (t is then exact or nearly so) and on general ones"""
    a, b, c = _random_tris(rng, n)
    axis = rng.random(n) < 0.5                             # in the plane z = a.z: t = (a.z - o.z) / d.z up to the rounding of f
    b[axis, 2] = a[axis, 2]; c[axis, 2] = a[axis, 2]
    a6, b6, c6 = (x.astype(np.float64) for x in (a, b, c))
    r1, r2 = rng.uniform(0.05, 0.9, n), rng.uniform(0.05, 0.9, n)
    m = r1 + r2 > 0.95
    r1[m], r2[m] = 0.95 - r1[m], 0.95 - r2[m]
    r1, r2 = np.abs(r1), np.abs(r2)
    p = a6 + r1[:, None] * (b6 - a6) + r2[:, None] * (c6 - a6)
    nrm = _unit(np.cross(b6 - a6, c6 - a6) + 1e-300)
    d = _unit(nrm * rng.choice([-1, 1], (n, 1)) + rng.normal(size=(n, 3)) * 0.3)
    d[axis] = np.array([0.0, 0.0, 1.0]) * rng.choice([-1, 1], (int(axis.sum()), 1))
    e = float(EPS)
    t0 = rng.choice([0.0, e, float(_down(EPS)), float(_up(EPS)), float(_up(EPS, 3)), float(_down(EPS, 3)), 2 * e, e / 2, -e, 1e-5, 3e-7], n)
    o = (p - d * t0[:, None])
    o32 = o.astype(f32)
    # axis-aligned: o.z = a.z - t0 d.z formed in float32 arithmetic so that a.z - o.z is t0 to the last bits (small |a.z| on a part)
    small = axis & (rng.random(n) < 0.6)
    a[small, 2] = 0.0; b[small, 2] = 0.0; c[small, 2] = 0.0
    o32[axis, 2] = (a[axis, 2] - (t0[axis] * d[axis, 2]).astype(f32)).astype(f32)
    return _rays(o32, d.astype(f32)), np.concatenate([a, b, c], 1)


def _tri_det_cutoff(rng, n):
    """det within a few ulp of +-1e-6.  Half exact: the unit right triangle in the plane z = 0 has det = -d.z, so d.z = +-EPSILON and
    its float neighbours put det exactly there; half general: a grazing direction whose tilt is corrected (three secant steps on the
    float32 determinant) until det sits at the cut-off, then moved by 0 .. 3 ulp"""
    h = n // 2
    A = np.zeros((h, 3), f32); B = np.zeros((h, 3), f32); C = np.zeros((h, 3), f32)
    B[:, 0] = 1; C[:, 1] = 1
    dz = np.array([EPS, _down(EPS), _up(EPS), _down(EPS, 2), _up(EPS, 2), 2 * EPS, EPS / 2], f32)[rng.integers(0, 7, h)] * rng.choice([-1, 1], h).astype(f32)
    ang = rng.uniform(0, 2 * np.pi, h)
    d = np.stack([np.cos(ang), np.sin(ang), dz], 1).astype(f32)
    p = np.stack([rng.uniform(0.05, 0.45, h), rng.uniform(0.05, 0.45, h), np.zeros(h)], 1)
    t0 = 2.0 ** rng.integers(-2, 2, (h, 1))
    o = (p - d.astype(np.float64) * t0).astype(f32)
    parts = [(_rays(o, d), np.concatenate([A, B, C], 1))]
    m = n - h
    a, b, c = _random_tris(rng, m)
    a6, b6, c6 = (x.astype(np.float64) for x in (a, b, c))
    nrm = _unit(np.cross(b6 - a6, c6 - a6) + 1e-300)
    e1 = _unit(b6 - a6)
    inpl = _unit(e1 * np.cos(ang[:m, None]) + np.cross(nrm, e1) * np.sin(ang[:m, None]))
    area2 = np.linalg.norm(np.cross(b6 - a6, c6 - a6), axis=1)
    want = float(EPS) * rng.choice([-1, 1], m)
    tilt = -want / np.maximum(area2, 1e-30)

    def det_of(tl):
        dd = (inpl + tl[:, None] * nrm).astype(f32)
        return tcb.moller_trumbore_f32(np.zeros_like(dd), dd, a, b, c)[2].astype(np.float64), dd

    t_prev, d_prev = tilt * 0.5, det_of(tilt * 0.5)[0]
    for _ in range(3):
        det, _dd = det_of(tilt)
        with np.errstate(all="ignore"):
            step = (want - det) * (tilt - t_prev) / (det - d_prev)
        t_prev, d_prev = tilt, det
        tilt = np.where(np.isfinite(step), tilt + step, tilt)
    _det, dd = det_of(tilt)
    p = a6 + 0.3 * (b6 - a6) + 0.3 * (c6 - a6)
    o = (p - dd.astype(np.float64) * 10 ** rng.uniform(-1, 1, (m, 1))).astype(f32)
    parts.append((_rays(o, dd), np.concatenate([a, b, c], 1)))
    return tuple(np.concatenate([q[k] for q in parts]) for k in range(2))


def _tri_degenerate(rng, n):
    """zero-area (collinear) and repeated-vertex triangles: never hit"""
    a, b, c = _random_tris(rng, n)
    kind = rng.integers(0, 4, n)
    b = np.where((kind == 0)[:, None], a, b)
    c = np.where((kind == 1)[:, None], b, c)
    c = np.where((kind == 2)[:, None], a, c)
    col = kind == 3
    c[col] = (a[col] + (b[col] - a[col]) * f32(2.0)).astype(f32)
    r, g = _through(rng, a, b, c, rng.random(n), np.zeros(n), jitter_share=0.3)
    return r, g


def _tri_nan_vertex(rng, n):
    a, b, c = _random_tris(rng, n)
    r, g = _through(rng, a, b, c, rng.uniform(0.1, 0.4, n), rng.uniform(0.1, 0.4, n), jitter_share=0.0)
    g[np.arange(n), rng.integers(0, 9, n)] = np.nan
    return r, g


TRI_FAMILIES = {
    "grazing, slivers, far, un-normalised": (lambda rng: _tri_grazing(rng, 30000), 201),
    "vertices and edges": (lambda rng: _tri_vertices_edges(rng, 30000), 202),
    "exact u = 0, v = 0, u + v = 1": (lambda rng: _tri_exact_edges(rng, 20000), 203),
    "origin in the plane, t at EPSILON": (lambda rng: _tri_plane_origins(rng, 30000), 204),
    "det at the cut-off": (lambda rng: _tri_det_cutoff(rng, 30000), 205),
    "degenerate": (lambda rng: _tri_degenerate(rng, 8000), 206),
    "NaN vertex": (lambda rng: _tri_nan_vertex(rng, 4000), 207),
}
TRI_ALL_MISS = ("degenerate", "NaN vertex")          # by construction


def triangle_pairs():
    """name -> (rays[n, 6], abc[n, 9]) float32"""
    out = {}
    for name, (gen, seed) in TRI_FAMILIES.items():
        r, g = gen(np.random.default_rng(seed))
        out[name] = (np.ascontiguousarray(r, f32), np.ascontiguousarray(g, f32))
    return out


# ---------------------------------------------------------------- rays against a scene, from its own node and triangle arrays

def _leaves(nodes):
    return np.flatnonzero(nodes["isLeaf"] == 1)


def scene_rays(nodes, triangles, seed=301):
    """name -> rays[n, 6].  `nodes` / `triangles`: the uploaded records (layout.BVH_NODE / layout.TRIANGLE)."""
    rng = np.random.default_rng(seed)
    mn, mx = nodes["min"].astype(f32), nodes["max"].astype(f32)
    A, B, C = (triangles[k].astype(f32) for k in ("aPosition", "bPosition", "cPosition"))
    fin = np.isfinite(mn).all(1) & np.isfinite(mx).all(1)
    lo, hi = mn[fin].min(0).astype(np.float64), mx[fin].max(0).astype(np.float64)
    centre, radius = (lo + hi) / 2, max(float(np.linalg.norm(hi - lo)) / 2, 1e-3)
    leaves = _leaves(nodes)
    nt = len(A)
    out = {}

    # 4096 incoherent rays: no two neighbours share an origin or a direction; two thirds aimed at a triangle of the scene
    n = 4096
    o = centre + rng.normal(size=(n, 3)) * radius * rng.choice([0.3, 1.0, 2.5], (n, 1))
    ti = rng.integers(0, nt, n)
    w = rng.dirichlet((1, 1, 1), n)
    tgt = A[ti] * w[:, :1] + B[ti] * w[:, 1:2] + C[ti] * w[:, 2:]
    tgt = np.where(rng.random((n, 1)) < 0.67, tgt, centre + rng.normal(size=(n, 3)) * radius)
    out["incoherent"] = _rays(o.astype(f32), _unit(tgt - o.astype(f32).astype(np.float64)).astype(f32))

    # axis-parallel rays, the origin ON real node planes (two coordinates from planes of the node, the third outside the scene)
    n = 1536
    nd = rng.integers(0, len(nodes), n)
    ax = rng.integers(0, 3, n)
    o = (mn[nd].astype(np.float64) + rng.random((n, 3)) * (mx[nd].astype(np.float64) - mn[nd].astype(np.float64))).astype(f32)
    for k in range(3):                                   # per other axis: on the min plane, on the max plane, or inside
        pick = rng.integers(0, 3, n)
        o[:, k] = np.where(pick == 0, mn[nd, k], np.where(pick == 1, mx[nd, k], o[:, k]))
    sign = rng.choice([-1.0, 1.0], n)
    idx = np.arange(n)
    start_out = rng.random(n) < 0.7
    o[idx, ax] = np.where(start_out, (centre[ax] - sign * radius * 1.5), o[idx, ax]).astype(f32)
    d = np.zeros((n, 3), f32)
    d[idx, ax] = sign
    d = np.where((d == 0) & (rng.random((n, 3)) < 0.3), f32(-0.0), d)
    out["axis-parallel on node planes"] = _rays(o, d)

    # aimed at real leaf-box corners, and at shared triangle edges / vertices
    n = 1024
    lf = leaves[rng.integers(0, len(leaves), n)]
    corner = np.where(rng.random((n, 3)) < 0.5, mn[lf], mx[lf])
    o = (centre + _unit(rng.normal(size=(n, 3))) * radius * rng.uniform(1.2, 3, (n, 1))).astype(f32)
    rays_c = _rays(o, _unit(corner.astype(np.float64) - o.astype(np.float64)).astype(f32))
    ti = rng.integers(0, nt, n)
    lam = rng.random((n, 1))
    which = rng.integers(0, 4, (n, 1))
    V = [A[ti], B[ti], C[ti]]
    tgt = np.select([which == 0, which == 1, which == 2], [V[0] + lam * (V[1] - V[0]), V[1] + lam * (V[2] - V[1]), V[2] + lam * (V[0] - V[2])],
                    np.where(lam < 0.33, V[0], np.where(lam < 0.66, V[1], V[2])))
    o = (centre + _unit(rng.normal(size=(n, 3))) * radius * rng.uniform(1.2, 3, (n, 1))).astype(f32)
    rays_e = _rays(o, _unit(tgt.astype(np.float64) - o.astype(np.float64)).astype(f32))
    out["leaf-box corners, triangle edges and vertices"] = np.concatenate([rays_c, rays_e])

    # origins ON triangle centroids: out along the normal (both ways), and in the triangle's plane
    n = 1024
    ti = rng.integers(0, nt, n)
    cen = ((A[ti].astype(np.float64) + B[ti] + C[ti]) / 3).astype(f32)
    nrm = np.cross(B[ti].astype(np.float64) - A[ti], C[ti].astype(np.float64) - A[ti])
    ok = np.linalg.norm(nrm, axis=1) > 0
    nrm = np.where(ok[:, None], nrm, [0.0, 1.0, 0.0])
    nrm = _unit(nrm) * rng.choice([-1, 1], (n, 1))
    e = _unit(np.where(ok[:, None], B[ti].astype(np.float64) - A[ti], [1.0, 0.0, 0.0]))
    inpl = _unit(e * np.cos(ang := rng.uniform(0, 2 * np.pi, (n, 1))) + np.cross(nrm, e) * np.sin(ang))
    d = np.where(rng.random((n, 1)) < 0.5, nrm, inpl).astype(f32)
    out["from triangle centroids"] = _rays(cen, d)

    # origins inside leaf boxes
    n = 1024
    lf = leaves[rng.integers(0, len(leaves), n)]
    o = (mn[lf].astype(np.float64) + rng.random((n, 3)) * (mx[lf].astype(np.float64) - mn[lf].astype(np.float64))).astype(f32)
    o = np.clip(o, mn[lf], mx[lf])
    out["from inside leaf boxes"] = _rays(o, _unit(rng.normal(size=(n, 3))).astype(f32))

    # the guard range: direction components at EPSILON / 2^20 and their neighbours, origins at 2^-70 / 2^60, all-ones significands,
    # subnormals, un-normalised by 2^+-10 -- on rays that do go at the scene
    n = 1024
    base = out["incoherent"][rng.integers(0, 4096, n)].copy()
    kind = rng.integers(0, 6, n)
    k = rng.integers(0, 3, n)
    idx = np.arange(n)
    sgn = rng.choice([-1, 1], n).astype(f32)
    ev = np.array([EPS, _down(EPS), _up(EPS), 0.0], f32)[rng.integers(0, 4, n)]
    m = kind == 0
    base[idx[m], 3 + k[m]] = ev[m] * sgn[m]
    m = kind == 1
    bv = np.array([BIG_D, _down(BIG_D), _up(BIG_D)], f32)[rng.integers(0, 3, n)]
    s = bv / np.maximum(np.abs(base[idx, 3 + k]), f32(1e-3))
    base[m, 3:] = (base[m, 3:] * s[m, None]).astype(f32)
    m = kind == 2
    ov = np.array([LO, _down(LO), _up(LO), np.ldexp(0.75, -140), HI, _up(HI), _down(HI)], f32)[rng.integers(0, 7, n)]
    base[idx[m], k[m]] = ov[m] * sgn[m]
    m = kind == 3
    base[m] = (base[m].view(np.uint32) | np.uint32(0x7fffff)).view(f32)
    m = kind == 4
    base[m, 3:] *= np.where(rng.random((int(m.sum()), 1)) < 0.5, f32(1024.0), f32(1.0 / 1024.0)).astype(f32)
    # (kind 5: left as they are)
    out["guard range"] = base

    # NaN, +-inf and the zero direction: all-miss by construction (NaN, d = 0) or whatever the reference says (inf)
    n = 192
    base = out["incoherent"][rng.integers(0, 4096, n)].copy()
    base[np.arange(n), rng.integers(0, 6, n)] = np.nan
    out["NaN"] = base
    base = out["incoherent"][rng.integers(0, 4096, n)].copy()
    base[np.arange(n), rng.integers(0, 6, n)] = np.where(rng.random(n) < 0.5, f32(np.inf), f32(-np.inf))
    out["inf"] = base
    base = out["from inside leaf boxes"][rng.integers(0, 1024, n)].copy()
    base[:, 3:] = np.where(rng.random((n, 3)) < 0.5, f32(0.0), f32(-0.0))
    out["d = 0"] = base
    return {k: np.ascontiguousarray(v, f32) for k, v in out.items()}


# all-miss by construction: with a NaN, an infinity or a zero direction among the operands every acceptance test of the triangle
# (raytrace.wgsl:78-116) is false -- det is 0 (d = 0) or the barycentrics are NaN / infinite
SCENE_RAYS_ALL_MISS = ("NaN", "inf", "d = 0")
WAVE_COUNTS = (1, 63, 65)                         # ray counts around one wave of the shipped first-hit walk


# ---------------------------------------------------------------- the scenes

def _scaled(sc_nodes, sc_tris, s=1.0, shift=(0.0, 0.0, 0.0)):
    """the tree and the triangles scaled by a power of two and translated: positions and boxes transformed in float32.  A power of two
    keeps every box a bound of its triangles bit for bit; a translation rounds, so the boxes are re-fitted from the moved vertices,
    bottom-up (children have larger indices than their parent)."""
    nodes, tris = sc_nodes.copy(), sc_tris.copy()
    shift = np.asarray(shift, f32)
    for k in ("aPosition", "bPosition", "cPosition"):
        tris[k] = (tris[k] * f32(s) + shift).astype(f32)
    if not shift.any():
        nodes["min"] = (nodes["min"] * f32(s)).astype(f32)
        nodes["max"] = (nodes["max"] * f32(s)).astype(f32)
        return nodes, tris
    for i in range(len(nodes) - 1, -1, -1):
        if nodes["isLeaf"][i] == 1:
            t = tris[nodes["triangleIndex"][i]]
            p = np.stack([t["aPosition"], t["bPosition"], t["cPosition"]])
            nodes["min"][i], nodes["max"][i] = p.min(0), p.max(0)
        else:
            l, r = nodes["left"][i], nodes["right"][i]
            nodes["min"][i] = np.minimum(nodes["min"][l], nodes["min"][r])
            nodes["max"][i] = np.maximum(nodes["max"][l], nodes["max"][r])
    return nodes, tris


def broken_boxes(nodes):
    """tests/test_gpu_culling.py: test_boxes_that_do_not_bound_their_triangles_are_never_skipped"""
    raw = nodes.view(np.uint8).reshape(len(nodes), 48).copy()
    f = raw.view(f32).reshape(len(nodes), 12)
    rng = np.random.default_rng(5)
    pick = rng.choice(np.arange(1, len(nodes)), 400, replace=False)
    f[pick, 0:3] += rng.uniform(0.0, 0.05, (400, 3)).astype(f32)
    f[pick, 4:7] += rng.uniform(-0.02, 0.05, (400, 3)).astype(f32)
    return raw.view(nodes.dtype).reshape(len(nodes))


SHIPPED_WALK_REFUSED = ("demo, broken boxes",)      # mi3pt_debug_intersect_shipped must answer with the state error there
TIE_SCENE = "coincident sheets"


def scenes():
    """name -> (nodes, triangles, material bytes), the reference's layouts"""
    import test_gpu_culling as cull
    import test_gpu_parity as parity
    from mi3pt_host import layout, scenes as S
    out = {}
    demo = S.demo_scene()
    demo.build_bvh()
    out["demo"] = (demo.nodes, demo.triangles, demo.material_bytes)
    for name in ("slivers", "tiny next to huge"):
        sc = cull._soup(**dict(cull.SOUPS[name], n=2000))
        out[name] = (sc.nodes, sc.triangles, sc.material_bytes)
    ball = S.flatten_mesh(S.sphere_geometry(0.4, 24, 16), S.compose_matrix(position=(0.0, 0.4, 0.0)), 0)
    sphere = S.Scene(ball[0], ball[1], ball[2], [S.WHITE], "sphere")
    sphere.build_bvh()
    out["sphere"] = (sphere.nodes, sphere.triangles, sphere.material_bytes)
    tie = parity._coincident_sheets_scene()
    out[TIE_SCENE] = (tie.nodes, tie.triangles, tie.material_bytes)
    tris, mats, nodes = cull._comb_scene(40)
    out["comb 40"] = (nodes, tris, mats)
    for label, s in (("demo x 2^-6", 2.0 ** -6), ("demo x 2^6", 2.0 ** 6)):
        n2, t2 = _scaled(demo.nodes, demo.triangles, s)
        out[label] = (n2, t2, demo.material_bytes)
    n2, t2 = _scaled(demo.nodes, demo.triangles, 1.0, (1000.0, 1000.0, 1000.0))
    out["demo + (1000, 1000, 1000)"] = (n2, t2, demo.material_bytes)
    out["demo, broken boxes"] = (broken_boxes(demo.nodes), demo.triangles, demo.material_bytes)
    import micro_geometry as mg                      # packets that are tiny AND close to the origin: empty slots pass the box test there
    for name in mg.SCENES:
        sc = mg.scene(name)
        out[name] = (sc.nodes, sc.triangles, sc.material_bytes)
    return out


def scene_rays_of(name, nodes, triangles):
    """scene_rays, and for a micro-geometry scene its rays aimed into the clusters from 0.5, 5 and 500 units as one more family"""
    import micro_geometry as mg
    fam = scene_rays(nodes, triangles)
    if name in mg.SCENES:
        fam["aimed into the clusters"] = mg.aimed_rays(mg.scene(name))
    return fam
