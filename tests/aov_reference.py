"""Reference for the first-hit feature images (mi3pt_render_aovs), from the oracle's own functions.

Per texel of a rank's rows: uv = (x / resolution.x, gy / resolution.y) as fp32 quotients, the oracle's camera ray for that uv
(pt_oracle.camera_ray: cameraToRay without jitter or lens) and its closest hit (pt_oracle.ray_scene: raySceneIntersect).  Nothing here
looks at the device.  No test lives in this file.
"""
import numpy as np

from mi3pt_host import capi

MISS_T = np.float32(1e20)          # the miss record's t (raytrace.wgsl:155, INF)


def _resolution(uniforms96):
    r = np.frombuffer(bytes(uniforms96), np.float32, 2, 0)
    return np.float32(r[0]), np.float32(r[1])


def _ray(orc, uniforms96, x, gy):
    res_x, res_y = _resolution(uniforms96)
    uvx = float(np.float32(x) / res_x)
    uvy = float(np.float32(gy) / res_y)
    r = orc.camera_ray(uniforms96, uvx, uvy)
    return r[:3].copy(), r[3:].copy()


def global_rows(h, rank, nranks, block_rows):
    """image row of every local row of `rank`'s compact image"""
    rows = capi.tile_local_rows(h, rank, nranks, block_rows)
    return [capi.tile_global_row(ly, rank, nranks, block_rows) for ly in range(rows)]


def reference(orc, scene, uniforms96, w, h, rank=0, nranks=1, block_rows=8, pixels=None):
    """The four images of `rank`'s rows of a w x h texture (rows x w x 4 each), as a dict:
    albedo, normal, position (float32), ids (int32: [-2, material, hit, 0] -- the oracle's record has no triangle index, -2 says so;
    misses [-1, -1, 0, 0]), computed (bool rows x w: texels that were evaluated -- all of them unless `pixels`, a list of
    (local row, x), names a subset), inside (bool: texel inside `resolution`), hit (bool), overflows (rays the 64-entry abort ended).
    scene: pt_oracle.OracleScene.  Texels outside `resolution` hold the miss values."""
    uniforms96 = bytes(uniforms96)
    res_x, res_y = _resolution(uniforms96)
    lim_x, lim_y = int(res_x), int(res_y)              # u32(resolution), raytrace.wgsl:425-427
    gys = global_rows(h, rank, nranks, block_rows)
    rows = len(gys)
    mats = np.frombuffer(np.ascontiguousarray(scene.mats).tobytes(), np.float32).reshape(-1, 16)
    out = {
        "albedo": np.zeros((rows, w, 4), np.float32), "normal": np.zeros((rows, w, 4), np.float32),
        "position": np.zeros((rows, w, 4), np.float32), "ids": np.zeros((rows, w, 4), np.int32),
        "computed": np.zeros((rows, w), bool), "inside": np.zeros((rows, w), bool), "hit": np.zeros((rows, w), bool),
        "overflows": 0,
    }
    out["position"][..., 3] = MISS_T
    out["ids"][..., 0] = -1
    out["ids"][..., 1] = -1
    todo = pixels if pixels is not None else [(ly, x) for ly in range(rows) for x in range(w)]
    for ly, x in todo:
        gy = gys[ly]
        out["computed"][ly, x] = True
        if not (x < lim_x and gy < lim_y and gy < h):
            continue
        out["inside"][ly, x] = True
        o, d = _ray(orc, uniforms96, x, gy)
        rec, cnt = orc.ray_scene(scene, o, d)
        out["overflows"] += cnt["stack_overflows"]
        if rec[0] == 0.0:
            assert rec[1] == MISS_T, "the oracle's miss t"
            continue
        mi = int(rec[8])
        out["hit"][ly, x] = True
        out["albedo"][ly, x] = (mats[mi, 0], mats[mi, 1], mats[mi, 2], 1.0)
        out["normal"][ly, x] = (rec[5], rec[6], rec[7], 0.0)
        out["position"][ly, x] = (rec[2], rec[3], rec[4], rec[1])
        out["ids"][ly, x] = (-2, mi, 1, 0)
    return out


def _tri_records(scene):
    recs = getattr(scene, "_aov_records", None)          # (a view of the scene's own bytes, made once: 97 MB for the large scene)
    if recs is None:
        recs = scene._aov_records = np.ascontiguousarray(scene.tris).reshape(-1).view(np.uint8).reshape(-1, 112)
    return recs


def triangle_matches(orc, scene, uniforms96, x, gy, tri_id):
    """The single-triangle condition that pins the triangle index: the oracle's test of the texel's ray against record [tri_id]
    returns the scene record's first eight values (hit, t, position, normal) bit for bit, and that triangle's materialIndex is the
    record's material.  Returns (meets the condition, the triangle's own t equals the scene record's t bit for bit)."""
    recs = _tri_records(scene)
    o, d = _ray(orc, bytes(uniforms96), x, gy)
    rec, _ = orc.ray_scene(scene, o, d)
    one = orc.ray_triangle(o, d, recs[tri_id])
    same_t = one[0] == 1.0 and one[1:2].tobytes() == rec[1:2].tobytes()
    mat = int(recs[tri_id, 92:96].copy().view(np.int32)[0])
    return bool(one[:8].tobytes() == rec[:8].tobytes() and mat == int(rec[8])), bool(same_t)


def check_ids(orc, scene, uniforms96, got_ids, ref, h, rank=0, nranks=1, block_rows=8):
    """The device's ids image against the reference, on every computed texel: material / hit / zero words equal the oracle's, a
    miss holds [-1, -1, 0, 0], and the triangle index of a hit meets the single-triangle condition (triangle_matches)."""
    got_ids = np.asarray(got_ids)
    assert got_ids.dtype == np.int32 and got_ids.shape == ref["ids"].shape
    sel = ref["computed"]
    assert np.array_equal(got_ids[..., 1:][sel], ref["ids"][..., 1:][sel]), "material / hit / reserved words of the ids image"
    miss = sel & ~ref["hit"]
    assert (got_ids[..., 0][miss] == -1).all(), "triangle index of a miss"
    ntris = len(_tri_records(scene))
    gys = global_rows(h, rank, nranks, block_rows)
    for ly, x in np.argwhere(sel & ref["hit"]):
        tid = int(got_ids[ly, x, 0])
        assert 0 <= tid < ntris, f"texel ({ly}, {x}): triangle index {tid}"
        ok, _ = triangle_matches(orc, scene, uniforms96, int(x), gys[ly], tid)
        assert ok, f"texel ({ly}, {x}): triangle {tid} does not reproduce the oracle's record"


def tie_census(orc, scene, uniforms96, ref, h, stride=37):
    """Of every `stride`-th hit texel of a whole-image reference (rank 0 of 1): (triangles whose own t equals the record's bit for bit,
    triangles that meet the single-triangle condition), by testing EVERY triangle of the scene."""
    ntris = len(_tri_records(scene))
    out = []
    for ly, x in np.argwhere(ref["hit"])[::stride]:
        same = meets = 0
        for t in range(ntris):
            ok, same_t = triangle_matches(orc, scene, uniforms96, int(x), int(ly), t)
            same += same_t
            meets += ok
        out.append((same, meets))
    return out


def assert_images(pc, got, ref, what=""):
    """got: dict name -> device image.  Every computed texel of every image equal, bit for bit (ids: material / hit / zero words;
    the triangle index is check_ids' business)."""
    sel = ref["computed"]
    for name in ("albedo", "normal", "position"):
        assert got[name].dtype == np.float32 and got[name].shape == ref[name].shape, f"{what} {name}: shape / type"
        assert pc.same_bits(got[name][sel], ref[name][sel]), f"{what} {name}: " + pc.describe_diff(got[name][sel], ref[name][sel])
    assert np.array_equal(got["ids"][..., 1:][sel], ref["ids"][..., 1:][sel]), f"{what} ids"
    assert (got["ids"][..., 0][sel & ~ref["hit"]] == -1).all(), f"{what} ids of misses"
    assert (got["ids"][..., 0][sel & ref["hit"]] >= 0).all(), f"{what} ids of hits"
