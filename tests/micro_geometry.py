"""Micro-geometry: small deterministic scenes whose packets are tiny AND close to the origin, seen from far away -- where the box test of
the compressed-packet walks (kernel variants 13 and 14) accepts EMPTY child slots (PROOFS.md 4a).  numpy only, fixed seeds, no device;
no test lives here.  tests/test_packet_walk_reference.py shows on the CPU that the condition is met; tests/test_gpu_micro_geometry.py and
tests/test_gpu_walk_probes.py run the kernels on them.

Every scene stands on a coarse floor (y = -1) and has one ordinary box beside the clusters, so that paths bounce.

  dust              clusters of 3, 5, 6, 9 and 17 triangles (odd counts: packets with empty slots in both walks), of size 1e-6 .. 1e-9,
                    centres within 1e-3 of the origin
  collapsed         the same + 24 zero-area triangles with all nine coordinates exactly 0 (extent 0, largest coordinate 0: the cell at
                    its 2^-100 floor) + 12 collapsed onto (1e-20, 0, -1e-20)
  flat dust         clusters in the plane y = 0 with zero extent on y: only that axis's grid degenerates
  dust + 0.02, dust + 1      the dust scene translated: the CONTROLS (the cell is floored at 2^-20 of the largest coordinate)
  tail              a hand-made proper tree, boxes nested: in its 8-ary collapse the LAST packet that owns records is a micro cluster at
                    the origin with leaves in its lowest slots only -- build_cw8's records end right behind them
"""
import numpy as np

from mi3pt_host import capi, layout, scenes

f32 = np.float32
CLUSTER_COUNTS = (3, 5, 6, 9, 17)
CLUSTER_SIZES = (1e-6, 1e-7, 1e-8, 1e-9)
CAMERA = dict(position=(0.0, 3.0, 4.0), target=(0.0, 0.0, 0.0), fov=45.0, focalDistance=5.0, aperture=0.0)      # 5 units from the origin
MATERIALS = [scenes.WHITE, scenes.RED, dict(color=(0.9, 0.8, 0.3), roughness=0.3, metalness=0.8, specularColor=(1.0, 1.0, 1.0))]
SCENES = ("dust", "collapsed", "flat dust", "dust + 0.02", "dust + 1", "tail")
CONTROLS = ("dust + 0.02", "dust + 1")


def _stage():
    q = scenes.quaternion_from_axis_angle((1.0, 0.0, 0.0), -np.pi / 2)
    floor = scenes.flatten_mesh(scenes.plane_geometry(8, 8), scenes.compose_matrix(position=(0.0, -1.0, 0.0), quaternion=q), 0)
    box = scenes.flatten_mesh(scenes.box_geometry(0.8, 0.8, 0.8), scenes.compose_matrix(position=(1.6, -0.6, 0.3)), 1)
    return floor, box


def _clusters(rng, flat=False, reps=3):
    """(positions (n, 3, 3) float64, centres (m, 3), sizes (m,))"""
    pos, centres, sizes = [], [], []
    for _ in range(reps):
        for size in CLUSTER_SIZES:
            for count in CLUSTER_COUNTS:
                c = rng.normal(size=3)
                c = c / np.linalg.norm(c) * rng.uniform(0.0, 1e-3)
                if flat:
                    c[1] = 0.0
                p = c + rng.uniform(-0.5, 0.5, (count, 3, 3)) * size
                if flat:
                    p[:, :, 1] = 0.0
                pos.append(p); centres.append(c); sizes.append(size)
    return np.concatenate(pos), np.array(centres), np.array(sizes)


def _scene(parts, name, shift=0.0):
    pos = np.concatenate([p[0] for p in parts]) + shift
    nrm = np.concatenate([p[1] for p in parts])
    mat = np.concatenate([p[2] for p in parts])
    sc = scenes.Scene(pos, nrm, mat, MATERIALS, name)
    sc.nodes = capi.host_build_bvh(sc.triangles)
    sc.camera = dict(CAMERA, position=tuple(np.array(CAMERA["position"]) + shift), target=(shift, shift, shift))
    return sc


def _dust_part(pos):
    e1, e2 = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    nrm = np.cross(e1, e2)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), [0.0, 1.0, 0.0])
    return pos, np.repeat(nrm[:, None, :], 3, 1), np.full(len(pos), 2, np.int64)


def _tail():
    """root = (Ta, (Tb, (Tc, M))): Ta / Tb / Tc balanced subtrees over five, five and four ordinary triangles (the floor and the box), M = ((t0, t1), t2)
    three triangles of size 1e-8 at the origin that lie towards (-x, -y), (+x, -y), (-x, +y) of M's centre and share one z range."""
    floor, box = _stage()
    u = 1e-8
    micro = np.array([[[-u, -u, 0.0], [-0.5 * u, -u, 0.0], [-u, -0.5 * u, 0.25 * u]],
                      [[u, -u, 0.0], [0.5 * u, -u, 0.0], [u, -0.5 * u, 0.25 * u]],
                      [[-u, u, 0.0], [-0.5 * u, u, 0.0], [-u, 0.5 * u, 0.25 * u]]])
    parts = [floor, box, _dust_part(micro)]
    pos = np.concatenate([p[0] for p in parts])
    sc = scenes.Scene(pos, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), MATERIALS, "tail")
    p32 = pos.astype(f32)

    def balanced(ts):
        return ("leaf", ts[0]) if len(ts) == 1 else (balanced(ts[:len(ts) // 2]), balanced(ts[len(ts) // 2:]))

    tree = (balanced(list(range(0, 5))), (balanced(list(range(5, 10))), (balanced(list(range(10, 14))), ((("leaf", 14), ("leaf", 15)), ("leaf", 16)))))
    nodes = np.zeros(2 * len(pos) - 1, layout.BVH_NODE)
    count = [0]

    def put(t):                                               # pre-order: children after their parent
        i = count[0]
        count[0] += 1
        if t[0] == "leaf":
            nodes[i]["min"], nodes[i]["max"] = p32[t[1]].min(0), p32[t[1]].max(0)
            nodes[i]["isLeaf"], nodes[i]["left"], nodes[i]["right"], nodes[i]["triangleIndex"] = 1, -1, -1, t[1]
        else:
            l = put(t[0]); r = put(t[1])
            nodes[i]["min"], nodes[i]["max"] = np.minimum(nodes[l]["min"], nodes[r]["min"]), np.maximum(nodes[l]["max"], nodes[r]["max"])
            nodes[i]["isLeaf"], nodes[i]["left"], nodes[i]["right"], nodes[i]["triangleIndex"] = 0, l, r, -1
        return i

    put(tree)
    assert count[0] == len(nodes)
    sc.nodes = nodes
    sc.camera = dict(CAMERA)
    sc.cluster_centres, sc.cluster_sizes = np.zeros((1, 3)), np.array([2e-8])
    sc.closeup_target = (0.0, 0.0, 0.0)
    return sc


def build(name):
    """name -> scenes.Scene with .nodes, .camera, .cluster_centres, .cluster_sizes"""
    if name == "tail":
        return _tail()
    floor, box = _stage()
    rng = np.random.default_rng(7101)
    flat = name == "flat dust"
    pos, centres, sizes = _clusters(rng, flat=flat)
    parts = [floor, box, _dust_part(pos)]
    if name == "collapsed":
        zero = np.zeros((24, 3, 3))
        near = np.tile(np.array([1e-20, 0.0, -1e-20]), (12, 3, 1))
        parts += [_dust_part(zero), _dust_part(near)]
        centres = np.concatenate([centres, [[0.0, 0.0, 0.0], [1e-20, 0.0, -1e-20]]])
        sizes = np.concatenate([sizes, [0.0, 0.0]])
    shift = {"dust + 0.02": 0.02, "dust + 1": 1.0}.get(name, 0.0)
    sc = _scene(parts, name, shift)
    sc.cluster_centres, sc.cluster_sizes = centres + shift, sizes
    # the close-up looks at the 24 collapsed triangles where there are some, else at the first cluster of five triangles of size 1e-8
    pick = len(CLUSTER_COUNTS) * CLUSTER_SIZES.index(1e-8) + CLUSTER_COUNTS.index(5)
    sc.closeup_target = (0.0, 0.0, 0.0) if name == "collapsed" else tuple(sc.cluster_centres[pick])
    return sc


_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = build(name)
    return _cache[name]


def aimed_rays(sc, n=2000, seed=7201):
    """n rays from random points on spheres of radius 0.5, 5 and 500 around the clusters' middle, aimed into the clusters"""
    rng = np.random.default_rng(seed)
    mid = sc.cluster_centres.mean(0)
    k = rng.integers(0, len(sc.cluster_centres), n)
    tgt = sc.cluster_centres[k] + rng.uniform(-0.5, 0.5, (n, 3)) * sc.cluster_sizes[k, None]
    radius = np.array([0.5, 5.0, 500.0])[np.arange(n) % 3]
    v = rng.normal(size=(n, 3))
    o = (mid + v / np.linalg.norm(v, axis=1, keepdims=True) * radius[:, None]).astype(f32)
    d = tgt - o.astype(np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    return np.ascontiguousarray(np.concatenate([o, d], 1), f32)


CLOSE_UP_WIDTH = 1e-5          # what the close-up view spans at its target, 5 units away: every ray passes within 5e-6 of the cluster


def views(sc):
    """name -> keyword arguments of ptcommon.rt_uniforms: the whole scene from 5 units (the clusters are far smaller than a pixel: its
    paths meet the floor and the box), and a close-up of ONE cluster from the same distance through a fov of 1.1e-4 degrees -- its camera
    rays, and the paths that bounce between the cluster's triangles, are the ones that pass tiny packets from far away"""
    cam = sc.camera
    whole = np.array(CAMERA["position"], np.float64)
    # (no direction component near 0: a slot is only accepted when the ray passes its packet within 2^-20 |d_i| of the distance on EVERY axis)
    off = np.array((2.4, 3.0, 3.2))
    tgt = np.asarray(sc.closeup_target, np.float64)
    return {"whole": dict(position=cam["position"], direction=tuple(-whole / 5.0), fov=cam["fov"]),
            "close-up": dict(position=tuple(tgt + off), direction=tuple(-off / 5.0), fov=float(np.degrees(CLOSE_UP_WIDTH / 5.0)))}


def camera_rays(sc, orc, w=64, h=48, view="whole"):
    """the un-jittered camera rays of a w x h view (tests/aov_reference.py's camera), texel by texel"""
    import aov_reference as ar
    import ptcommon as pc
    u = pc.rt_uniforms(sc, w, h, focal=sc.camera["focalDistance"], **views(sc)[view]).tobytes()
    out = np.zeros((h * w, 6), f32)
    for y in range(h):
        for x in range(w):
            o, d = ar._ray(orc, u, x, y)
            out[y * w + x, :3], out[y * w + x, 3:] = o, d
    return out


def probe_rays(sc, orc):
    """name -> rays[n, 6]: the camera rays, tests/walk_probe_inputs.py's families on this scene, and the aimed rays"""
    import walk_probe_inputs as wpi
    out = {"camera 64 x 48": camera_rays(sc, orc), "camera 64 x 48, close-up": camera_rays(sc, orc, view="close-up")}
    out.update(wpi.scene_rays(sc.nodes, sc.triangles))
    out["aimed into the clusters"] = aimed_rays(sc)
    return out
