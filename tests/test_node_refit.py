"""The Node host's `refit = true` loop against its rebuild loop: render_demo.js --slide 3 --step 0.1 --spp 3 at 64 x 48, four bounces, once
with --refit and once without.  The tree decides nothing but which of two hits at exactly the same t is kept, so the two loops render
the same mean wherever the oracle, run on both trees, says the tree does not matter -- and the records the refit loop held in every
step are the law's (tests/refit_reference.py), with a cost ratio of at least 1."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptcommon as pc
import refit_reference as rr
from mi3pt_host import capi, layout
from test_node_convergence import JS
from test_node_reproject_scene import _slid

STEPS, SPP, SLIDE = 3, 3, 0.1
# (render_demo.js --slide only translates the box, and a translation leaves every box's area what it was up to the fp32 rounding of its
# bounds: the cost ratio is 1 within 1e-9 on EITHER side -- a slide of 0.3 reads 0.999 999 999.  Slides of 0.1 and 0.2, the steps below,
# read 1 and 1.000 000 001; the test holds the reported ratios to the figure computed here bit for bit, so another STEPS or SLIDE is held
# just as firmly, but may need the `>= 1` below looked at)
W, H = 64, 48


def _demo_loop(node, tmp_path, env, name, *more):
    out = str(tmp_path / name)
    r = subprocess.run([node, os.path.join(JS, "tools", "render_demo.js"), "--env", str(tmp_path / "env.f32"), "--width", str(W), "--height", str(H),
                        "--bounces", "4", "--out", out, "--slide", str(STEPS), "--step", str(SLIDE), "--spp", str(SPP)] + list(more),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    images = [np.frombuffer(open(f"{out}_step{k}.acc.f32", "rb").read(), np.float32).reshape(H, W, 4) for k in range(STEPS)]
    blocks = [open(f"{out}_step{k}.uniforms.bin", "rb").read() for k in range(STEPS)]
    return out, summary, images, blocks, r.stderr


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_node_refit_loop_renders_what_the_rebuild_loop_renders(built, orc, demo, env, tmp_path):
    node = shutil.which("node")
    (tmp_path / "env.f32").write_bytes(env.tobytes())
    out, summary, refit, blocks, log = _demo_loop(node, tmp_path, env, "refit", "--refit")
    _, plain, rebuilt, blocks_plain, _ = _demo_loop(node, tmp_path, env, "rebuild")
    assert blocks == blocks_plain and "refit" not in plain
    assert summary["status"] == "idle" and summary["frame"] == SPP + 1 and summary["stats"] == plain["stats"]
    assert summary["stats"]["Triangles"] == 1998 and summary["stats"]["BVH Nodes"] == 3995
    # what happened per step: the first is built, the others are re-fitted, at a cost of at least the build's
    ratios = summary["refit"]
    assert len(ratios) == STEPS and ratios[0] is None and all(r is not None and r >= 1.0 for r in ratios[1:])
    assert log.count("--refit: step") == STEPS and "cost ratio" in log
    assert pc.same_bits(refit[0], rebuilt[0])                     # the first step is the same build in both loops
    for k in range(STEPS):
        sc = demo if k == 0 else _slid(demo, k * SLIDE)
        held = np.frombuffer(open(f"{out}_step{k}.nodes.bin", "rb").read(), layout.BVH_NODE)
        want = rr.refit_vectorised(demo.nodes, sc.triangles)       # the first build's topology, this step's boxes
        assert rr.first_difference(held, want) is None, f"step {k}: " + str(rr.first_difference(held, want))
        if k > 0:
            assert ratios[k] == capi.host_bvh_cost(want) / capi.host_bvh_cost(demo.nodes)
        # where does the tree matter?  the oracle on both trees, every frame of the step
        sc.build_bvh()
        on_refit = orc.OracleScene(sc.triangles, sc.material_bytes, want, env)
        on_built = orc.OracleScene(sc.triangles, sc.material_bytes, sc.nodes, env)
        same = np.ones((H, W), bool)
        for frame in range(2, SPP + 2):
            u = bytearray(blocks[k])
            u[12:16] = np.uint32(frame).tobytes()
            a, _ = orc.raytrace(on_refit, bytes(u), W, H)
            b, _ = orc.raytrace(on_built, bytes(u), W, H)
            same &= (np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)).all(-1)
        assert same.mean() > 0.99, f"step {k}: the oracle sees the tree in {(~same).sum()} texels"
        got, ref = refit[k].view(np.uint32), rebuilt[k].view(np.uint32)
        differ = (got != ref).any(-1) & same
        assert not differ.any(), f"step {k}: {differ.sum()} texels differ between the two loops where the tree does not matter"
        assert np.isfinite(refit[k]).all() and refit[k][..., :3].max() > 0
