"""What a refit costs in tree quality (CPU only: the oracle and the host builder; no device).

The demo scene with its box slid by 0.1 ... 0.6 along x, and turned by 2 ... 45 degrees about y.  For every step the tree of the
UNMOVED scene re-fitted to the moved triangles (tests/refit_reference.py: the law of mi3pt_device_refit_bvh) against the tree built
for the moved triangles (mi3pt_host_build_bvh_f64): mi3pt_host_bvh_cost of both over the unmoved build's -- the figure
renderer.refitCostLimit is compared with -- and the oracle's box and triangle tests per ray on both, one 160 x 96 frame, four bounces.
The table of DESIGN.md section 4 is this script's output.

    python profiles/refit_cost.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "webgpu-pathtracer_amd", "py"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import __graft_entry__ as ge          # noqa: E402

W, H = 160, 96


def main():
    ge.build()
    import pt_oracle as orc
    import ptcommon as pc
    import refit_reference as rr
    from mi3pt_host import capi, scenes

    env = scenes.synthetic_env()
    base = scenes.demo_scene()
    base.build_bvh()
    cost0 = capi.host_bvh_cost(base.nodes)
    print(f"demo scene, {len(base.triangles)} triangles, {len(base.nodes)} nodes, host_bvh_cost {cost0:.3f}; oracle {W} x {H}, 4 bounces, frame 2")
    print("| move | cost ratio, re-fitted | cost ratio, rebuilt | box tests / ray, re-fitted | rebuilt | triangle tests / ray, re-fitted | rebuilt |")
    print("|---|---|---|---|---|---|---|")
    moves = [("slid %.1f" % s, s, 0.0) for s in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6)] + [("turned %d deg" % d, 0.0, float(d)) for d in (2, 5, 10, 20, 30, 45)]
    moves.append(("slid 0.6, turned 30 deg", 0.6, 30.0))
    for name, slide, turn in moves:
        sc = rr.moved_demo(slide, turn)
        refitted = rr.refit_vectorised(base.nodes, sc.triangles)
        sc.build_bvh()
        u = pc.rt_uniforms(sc, W, H, frame=2, bounces=4).tobytes()
        row = []
        images = []
        for nodes in (refitted, sc.nodes):
            img, cnt = orc.raytrace(orc.OracleScene(sc.triangles, sc.material_bytes, nodes, env), u, W, H)
            images.append(img)
            row.append((capi.host_bvh_cost(nodes) / cost0, cnt["box_tests"] / cnt["rays"], cnt["tri_tests"] / cnt["rays"]))
        assert pc.same_bits(images[0], images[1]), "the two trees rendered different images"
        (ca, ba, ta), (cb, bb, tb) = row
        print(f"| {name} | {ca:.3f} | {cb:.3f} | {ba:.1f} | {bb:.1f} | {ta:.2f} | {tb:.2f} |")


if __name__ == "__main__":
    main()
