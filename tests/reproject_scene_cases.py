"""Moved variants of the demo scene for the tests of mi3pt_reproject_scene, and the triangle index of the oracle's first hits.  The demo
scene has 1998 triangles: 0 - 1 the ground, 2 - 13 the red box, 14 - 1997 the sphere; a variant keeps count and order (index i names the
same surface element), so the demo scene's records are the kept geometry of every variant.  No test lives in this file."""
import math

import numpy as np

import aov_reference as ar
from mi3pt_host import scenes

GROUND, BOX, SPHERE = slice(0, 2), slice(2, 14), slice(14, 1998)
TRANSLATION = (0.5, 0.25, -1.0)


def _variant(demo, positions, normals):
    sc = scenes.Scene(positions, normals, demo.material_index, demo.materials)
    sc.build_bvh()
    sc.camera = dict(demo.camera)
    return sc


def _turn_y(v, degrees, pivot=(0.0, 0.0, 0.0)):
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    p = np.asarray(pivot, np.float64)
    d = v - p
    return np.stack([c * d[..., 0] + s * d[..., 2], d[..., 1], -s * d[..., 0] + c * d[..., 2]], axis=-1) + p


def box_moved(demo, shift=(0.15, 0.0, 0.0), degrees=10.0):
    """the box turned by `degrees` about the vertical axis through its centre, then moved by `shift`; ground and sphere as they are"""
    pos, nrm = np.array(demo.positions, np.float64), np.array(demo.normals, np.float64)
    centre = pos[BOX].reshape(-1, 3).mean(axis=0)
    pos[BOX] = _turn_y(pos[BOX], degrees, centre) + np.asarray(shift, np.float64)
    nrm[BOX] = _turn_y(nrm[BOX], degrees)
    return _variant(demo, pos, nrm)


def box_moved_sphere_squashed(demo):
    """box_moved, and the sphere's heights times 0.9 (a deformation: its normals are left as they are, as a skinning host might)"""
    moved = box_moved(demo)
    pos, nrm = np.array(moved.positions, np.float64), np.array(moved.normals, np.float64)
    pos[SPHERE, :, 1] *= 0.9
    return _variant(demo, pos, nrm)


def translated(demo, t=TRANSLATION):
    """the whole scene moved by t: every triangle is `moved`; the camera that sees the same picture is the demo's moved by t too"""
    pos = np.array(demo.positions, np.float64) + np.asarray(t, np.float64)
    return _variant(demo, pos, np.array(demo.normals, np.float64))


def triangle_indices(orc, sc, uniforms96, feat, w, h):
    """word 0 of the ids image of the oracle's features (aov_reference.reference leaves -2): per texel the lowest triangle index whose
    own (hit, t) equals the scene record's bitwise, from ONE ray_triangle_n call over all texel x triangle pairs.  Returns the ids image
    with word 0 filled in (misses keep -1)."""
    rays = np.zeros((h * w, 6), np.float32)
    for y in range(h):
        for x in range(w):
            o, d = ar._ray(orc, bytes(uniforms96), x, y)
            rays[y * w + x, :3], rays[y * w + x, 3:] = o, d
    tris = sc.triangles
    abc = np.concatenate([tris["aPosition"], tris["bPosition"], tris["cPosition"]], axis=1).astype(np.float32)      # (n, 9)
    n = len(abc)
    out = orc.ray_triangle_n(np.repeat(rays, n, axis=0), np.tile(abc, (h * w, 1))).reshape(h * w, n, 4)
    t_scene = np.ascontiguousarray(feat["position"][..., 3]).reshape(-1).view(np.int32)
    same = (out[..., 0] == 1.0) & (np.ascontiguousarray(out[..., 1]).view(np.int32) == t_scene[:, None])
    hit = np.asarray(feat["hit"]).reshape(-1)
    assert same[hit].any(axis=1).all(), "a hit texel without a triangle that reproduces its record"
    ids = np.array(feat["ids"], np.int32)
    ids[..., 0] = np.where(hit, same.argmax(axis=1), -1).reshape(h, w)
    return ids
