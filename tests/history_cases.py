"""The use case of the held history (mi3pt_hold_history, mi3pt_merge_history) on the CPU: the demo scene sampled for 64 frames, a change of
the scene under a fixed camera, mi3pt_reproject_scene's reference, then K fresh frames of the new scene -- merged at once (the call's own
behaviour), held / validated / merged (history_reference.merge_history), or alone.  Every frame is the oracle's.  tests/
test_history_reference.py asserts orderings on it; profiles/history.py --cpu prints the table of DESIGN.md section 3.  No test lives in this file."""
import numpy as np

import aov_reference as ar
import history_reference as hr
import ptcommon as pc
import reproject_reference as rr
import reproject_scene_cases as cases
import reproject_scene_reference as rs
from mi3pt_host import scenes

F = np.float32
W, H = 48, 32
HISTORY_FRAMES, TRUTH_FRAMES = 64, 1024
CHANGES = ("nothing", "repaint", "slide", "dimmed")


def _uniforms(sc, frame):
    return pc.rt_uniforms(sc, W, H, frame=frame, bounces=4)


def _features(orc, sc, osc):
    u = _uniforms(sc, 0).tobytes()
    feat = ar.reference(orc, osc, u, W, H)
    feat["ids"] = cases.triangle_indices(orc, sc, u, feat, W, H)
    return feat


def repainted(demo, color=(0.05, 1.0, 0.05)):
    """the demo scene with the box's material (index 1, red) given another colour; geometry and order as they are"""
    materials = [dict(m) for m in demo.materials]
    materials[1]["color"] = tuple(color)
    sc = scenes.Scene(demo.positions, demo.normals, demo.material_index, materials)
    sc.build_bvh()
    sc.camera = dict(demo.camera)
    return sc


def changed(demo, change):
    """(scene, environment) after `change`"""
    env = scenes.synthetic_env(sun_radiance=0.0)
    if change == "repaint":
        return repainted(demo), env
    if change == "slide":
        return cases.box_moved(demo, shift=(0.6, 0.0, 0.0), degrees=0.0), env
    if change == "dimmed":
        env = env.copy()
        env[..., :3] *= F(0.5)
        return demo, env
    return demo, env


def tone_rmse(x, truth, sel):
    a = np.asarray(x, np.float64)[..., :3][sel]
    b = np.asarray(truth, np.float64)[..., :3][sel]
    return float(np.sqrt((((a / (1 + a)) - (b / (1 + b))) ** 2).mean()))


class UseCase:
    """the old scene's history, computed once; measure(change, ...) leaves it unchanged"""

    def __init__(self, orc, demo):
        self.orc, self.demo = orc, demo
        self.osc = pc.oracle_scene(orc, demo, scenes.synthetic_env(sun_radiance=0.0))
        mean, moments = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
        for k in range(HISTORY_FRAMES):
            mean, moments = rr.by_count_step(mean, moments, orc.raytrace(self.osc, _uniforms(demo, 2 + k).tobytes(), W, H)[0])
        self.mean, self.moments = mean, moments
        self.features = _features(orc, demo, self.osc)
        self.f0 = rr.view_frame(_uniforms(demo, 0).tobytes())
        self._new = {}

    def new_scene(self, change):
        """(scene, oracle scene, features, the 1024-frame yardstick, the carried (mean, moments)) of `change`, computed once"""
        if change not in self._new:
            orc = self.orc
            sc, env = changed(self.demo, change)
            osc = pc.oracle_scene(orc, sc, env)
            truth = np.zeros((H, W, 4), np.float64)
            for f in range(1000, 1000 + TRUTH_FRAMES):
                truth += orc.raytrace(osc, _uniforms(sc, f).tobytes(), W, H)[0]
            truth /= TRUTH_FRAMES
            feat = _features(orc, sc, osc)
            a, m, _ = rs.reproject_scene(self.mean, self.moments, self.f0, (F(W), F(H)), feat, self.features, (W, H), sc.triangles,
                                         self.demo.triangles)
            self._new[change] = (sc, osc, feat, truth, (a, m))
        return self._new[change]

    def measure(self, change, frames=4, radius=1, z_keep=2.0, z_drop=4.0):
        """dict(alone, at_once, validated: tone-mapped RMSE over the new scene's hit texels against the yardstick; kept: the share of
        carried samples the validated merge kept)"""
        sc, osc, feat, truth, carried = self.new_scene(change)
        hit = feat["hit"]
        fresh = [self.orc.raytrace(osc, _uniforms(sc, 2 + HISTORY_FRAMES + k).tobytes(), W, H)[0] for k in range(frames)]
        alone = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
        at_once = carried
        for c in fresh:
            alone = rr.by_count_step(*alone, c)
            at_once = rr.by_count_step(*at_once, c)
        a, m, _ = hr.merge_history(alone[0], alone[1], carried[0], carried[1], (W, H), radius, z_keep, z_drop)
        return {"alone": tone_rmse(alone[0], truth, hit), "at_once": tone_rmse(at_once[0], truth, hit), "validated": tone_rmse(a, truth, hit),
                "kept": hr.kept_share(alone[1], m, carried[1], hit)}
