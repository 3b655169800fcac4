"""tests/shading_cases.py on the CPU: the inversion of rand() that forces a draw, and the oracle's statistics of every
case of tests/test_gpu_shading.py against that case's condition -- a case that has drifted into vacuity (a scene, a
camera or a table changed under it) fails here, without a GPU."""
import numpy as np
import pytest

import ptcommon as pc
import shading_cases as sh
from mi3pt_host import capi, layout


def test_forced_frame_inverts_rand(orc):
    """draws 1, 2, 6, 11, 18; hash outputs 0 -> 0.0, 2^32 - 1 and 2^32 - 128 -> 1.0 (the conversion to f32 rounds them to
    2^32), 2^32 - 129 -> 0.99999994 (the largest value below 1); first, forced and last pixel of the 64 x 48 image."""
    assert sh.INVERSION_VALUES[sh.OUT_BELOW_ONE] == float(np.nextafter(np.float32(1), np.float32(0)))
    for draw, result in sh.INVERSION_CHECKS:
        for index in (0, sh.FORCED_PIXEL[0] + sh.FORCED_PIXEL[1] * sh.W, sh.W * sh.H - 1):
            frame = sh.forced_frame(draw, result, index)
            assert 0 <= frame <= sh.M32
            values, _ = orc.rand_sequence(sh.pixel_seed(frame, index), draw)
            assert values[-1] == np.float32(sh.INVERSION_VALUES[result]), (draw, result, index, values[-1])
    for state in (0, 1, 0x0FFFFFFF, 0x80000000, 0xDEADBEEF, sh.M32):           # every shift of the output function
        assert sh.state_for_output(sh.hash_output(state)) == state


def test_palette_scene_is_as_the_table_says(demo):
    sc = sh.palette_scene()
    assert len(sh.PALETTE) == 14 and np.array_equal(sc.triangles["aPosition"], demo.triangles["aPosition"])
    index = sc.triangles["materialIndex"]
    assert index[0] == 0 and index[1] == 0 and index[2] == (2 * 7919) % 14 and index[1997] == (1997 * 7919) % 14
    assert index.min() == 0 and index.max() == 13 and len(set(index[14:].tolist())) == 14       # inside the table, all of it used
    m = np.frombuffer(sc.material_bytes.tobytes(), layout.MATERIAL)
    assert np.isnan(m[7]["metalness"]) and m[4]["roughness"] == -1 and m[11]["emissionStrength"] == np.float32(1e10)
    assert 1e30 * 1e10 > float(np.finfo(np.float32).max) and m[13]["emissionColor"][2] < np.finfo(np.float32).tiny


def test_edge_environment_is_as_the_issue_says(env):
    e = sh.edge_env()
    assert e.shape == env.shape and np.array_equal(e[:180], env[:180]) and np.array_equal(e[300:], env[300:])
    assert np.array_equal(e[..., 3], env[..., 3])
    for r, c in ((180, 0), (183, 7), (184, 8), (299, 1023), (250, 500)):
        want = sh.EDGE_TEXELS[((c // 8) + r // 4) % 6]
        assert pc.same_bits(e[r, c, :3], np.full(3, want, np.float32)), (r, c)
    assert 0 < sh.EDGE_TEXELS[4] < np.finfo(np.float32).tiny


def test_palette_statistics(orc, env):
    sc = sh.palette_scene()
    stats = [sh.image_stats(sh.palette_reference(orc, sc, env, f16)[0]) for f16 in (False, True)]
    sh.check_palette_stats(*stats)


def test_edge_environment_statistics(orc, env):
    sc = sh.palette_scene()
    img, cnt, _ = sh.oracle_run(orc, pc.oracle_scene(orc, sc, sh.edge_env()), sc, (sh.EDGE_FRAME,), bounces=sh.EDGE_BOUNCES)
    sh.check_edge_env_stats(sh.image_stats(img))
    # the streaming kernel of MI3PT_OPT_SKY_TILES has tiles to shade in these views, and they look into the edge texels
    for name, kw in sh.SKY_CAMERAS.items():
        u = pc.rt_uniforms(sc, sh.W, sh.H, frame=sh.EDGE_FRAME, bounces=sh.EDGE_BOUNCES, **kw)
        empty = capi.host_sky_tiles(sc.nodes, u.tobytes(), sh.W, sh.H)
        img, cnt, _ = sh.oracle_run(orc, pc.oracle_scene(orc, sc, sh.edge_env()), sc, (sh.EDGE_FRAME,), bounces=sh.EDGE_BOUNCES, **kw)
        sky = np.repeat(np.repeat(empty.astype(bool), 8, 0), 8, 1)[:sh.H, :sh.W]
        odd = int((~np.isfinite(img[..., :3]).all(-1) & sky).sum())
        print(f"{name}: {int(empty.sum())} of {empty.size} tiles see no geometry, {odd} non-finite pixels in them, {cnt['hits']} hits")
        assert (empty.sum() >= 4 and odd >= 50) if not kw else (empty.sum() >= 24 and odd >= 500 and cnt["hits"] >= 100)


def test_pole_cameras(orc, env):
    """cameraToRay looking straight up and down (the |w . up| > 0.99999 branch takes another up vector): finite rays."""
    sc = sh.palette_scene()
    for d in sh.POLE_DIRECTIONS:
        u = pc.rt_uniforms(sc, sh.W, sh.H, frame=sh.EDGE_FRAME, bounces=sh.EDGE_BOUNCES, position=sh.POLE_POSITION, direction=d)
        rays = np.array([orc.camera_ray(u.tobytes(), x, y) for x, y in ((0.0, 0.0), (0.5, 0.5), (0.984375, 0.979))])
        print(f"camera direction {d}: centre ray {rays[1, 3:]}, corner ray {rays[0, 3:]}")
        assert np.isfinite(rays).all() and pc.same_bits(rays[1, 3:], np.array(d, np.float32))
    # looking up every pixel is sky, looking down the image is full of geometry
    osc = pc.oracle_scene(orc, sc, env)
    for d in sh.POLE_DIRECTIONS:
        img, cnt, _ = sh.oracle_run(orc, osc, sc, (sh.EDGE_FRAME,), bounces=sh.EDGE_BOUNCES, position=sh.POLE_POSITION, direction=d)
        print(f"camera direction {d}: {sh.image_stats(img)}, {cnt['hits']} hits, {cnt['misses']} misses")
        assert (cnt["hits"] == 0 and cnt["misses"] == sh.W * sh.H) if d[1] > 0 else cnt["hits"] > 1000


def test_environment_settings(orc, env):
    """Without environment light the emission is what is left: the negative and the underflowing one are live."""
    sc = sh.palette_scene()
    osc = pc.oracle_scene(orc, sc, env)
    for intensity, rotation in sh.ENV_SETTINGS:
        img, _, _ = sh.oracle_run(orc, osc, sc, (sh.EDGE_FRAME,), bounces=sh.EDGE_BOUNCES, intensity=intensity, rotation=rotation)
        print(f"envMapIntensity {intensity} envMapRotation {rotation}: {sh.image_stats(img)}")
        if intensity == 0.0:
            sh.check_dark_env_stats(sh.image_stats(img))
    assert sh.ENV_SETTINGS[0][0] == 0.0


@pytest.mark.parametrize("name", list(sh.FORCED_CASES))
def test_forced_draw_conditions(orc, env, name):
    sh.forced_reference(orc, env, name)


@pytest.mark.parametrize("name", list(sh.WRAP_CASES))
def test_wrap_conditions(orc, demo, env, name):
    sh.wrap_reference(orc, demo, env, name)
