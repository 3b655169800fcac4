"""What does the clustering builder (mi3pt_device_build_bvh_ex, method 1; csrc/pt_ploc.hip) cost, and what are its trees worth?
(needs a HIP device)

One process per scene -- scenes.dragon_class_scene() (869 882 triangles) or scenes.forest_scene() (about 10 M) -- the sides alternating,
medians of --runs (5) after one warm-up each:

    build    build_ms (device events) and wall time (queue flush, allocation, device work, the copy of the records to the host, the free)
             of the linear build, of the clustering at radius 8 / 16 / 32, and the wall time of capi.host_build_bvh_f64 on --threads
             threads; search_iterations and forced_iterations of the clustering
    tree     capi.host_bvh_cost, the depth, and words 4, 5, 6, 15, 18, 19 of mi3pt_host_scene_compile (tree_proper, walk_stack_worst,
             cull_stack_ok, cwide_ok, wide_stack_worst, auto_wide_variant) of every tree
    frames   on every tree, uploaded in turn: the time of a batch of --batch (16) 1920 x 1080, 8-bounce frames after a warm-up batch,
             the box and triangle tests per ray from the counters, and what MI3PT_OPT_LAST_BUILD says the launch ran

Nothing here is a pass / fail check but one: every clustering tree must be a proper tree over the triangles (lbvh_reference.check_tree,
structure only).  The trees are held to the law, word for word, by tests/test_gpu_ploc.py.

    python profiles/ploc.py --scene dragon|forest [--runs 5] [--frame-runs 5] [--log profiles/ploc.log]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "webgpu-pathtracer_amd", "py"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np                    # noqa: E402

import __graft_entry__ as ge          # noqa: E402

W, H, BOUNCES = 1920, 1080, 8
COMPILE_WORDS = ("tree_proper", "walk_stack_worst", "cull_stack_ok", "cwide_ok", "wide_stack_worst", "auto_wide_variant")      # words 4, 5, 6, 15, 18, 19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("dragon", "forest"), default="dragon")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--frame-runs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ploc.log"))
    args = ap.parse_args()
    ge.build()
    import lbvh_reference as lr
    import ptcommon as pc
    from mi3pt_host import capi, scenes

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
        with open(args.log, "w") as f:                     # (kept current: a run cut short still leaves what it measured)
            f.write("\n".join(lines) + "\n")

    t0 = time.perf_counter()
    sc = scenes.dragon_class_scene() if args.scene == "dragon" else scenes.forest_scene()
    say(f"== {sc.name}: {len(sc.triangles)} triangles (generated in {time.perf_counter() - t0:.1f} s); {W} x {H}, {BOUNCES} bounces, "
        f"batches of {args.batch} frames; host build on {args.threads} threads")
    env = scenes.synthetic_env()
    med = lambda v: float(np.median(v))
    sides = [("lbvh", ("lbvh",)), ("ploc r8", ("ploc", 8)), ("ploc r16", ("ploc", 16)), ("ploc r32", ("ploc", 32))]
    with capi.Context(0) as ctx:
        say(capi.device_name(0))
        ctx.upload_triangles(sc.triangles)
        ctx.upload_materials(sc.material_bytes)
        ctx.upload_environment(env)
        trees, info_of = {}, {}
        for name, a in sides:                              # warm-up (code objects, first allocations); these are the trees kept
            trees[name], info_of[name] = ctx.device_build_bvh(*a)
        trees["host sah"] = capi.host_build_bvh_f64(sc.positions, args.threads)
        wall, dev = {k: [] for k in trees}, {k: [] for k in trees}
        for run in range(args.runs):
            for name, a in sides:
                t0 = time.perf_counter()
                _, info = ctx.device_build_bvh(*a)
                wall[name].append((time.perf_counter() - t0) * 1e3)
                dev[name].append(info.build_ms)
            t0 = time.perf_counter()
            capi.host_build_bvh_f64(sc.positions, args.threads)
            wall["host sah"].append((time.perf_counter() - t0) * 1e3)
            say(f"build run {run}: " + "   ".join(f"{k} {wall[k][-1]:.1f} ms" + (f" (device {dev[k][-1]:.2f})" if dev[k] else "") for k in trees))
        say("-- build, medians of %d: wall ms [min .. max], build_ms [min .. max], search + forced iterations" % args.runs)
        for k in trees:
            d = f"{med(dev[k]):9.2f} [{min(dev[k]):.2f} .. {max(dev[k]):.2f}]" if dev[k] else "        -"
            it = f"{info_of[k].search_iterations} + {info_of[k].forced_iterations}" if k.startswith("ploc") else "-"
            say(f"{k:9s} wall {med(wall[k]):9.1f} [{min(wall[k]):.1f} .. {max(wall[k]):.1f}]   build_ms {d}   iterations {it}")
        say("-- trees: host_bvh_cost, depth, " + ", ".join(COMPILE_WORDS))
        ok = True
        for k, nodes in trees.items():
            comp = capi.host_scene_compile(nodes, sc.triangles)
            say(f"{k:9s} cost {capi.host_bvh_cost(nodes):8.3f}   depth {lr.depth(nodes):3d}   " + "  ".join(f"{w} {comp[w]}" for w in COMPILE_WORDS))
            if k.startswith("ploc"):
                try:
                    lr.check_tree(nodes, sc.triangles, boxes=False)
                except AssertionError as e:
                    ok = False
                    say(f"{k}: NOT A PROPER TREE: {e}")
        ctx.set_tile(0, 1, 8)
        ctx.resize(W, H)

        def batch(first):
            for f in range(first, first + args.batch):
                pc.gpu_frame(ctx, pc.rt_uniforms(sc, W, H, frame=f, bounces=BOUNCES), pc.acc_uniforms(W, H, f),
                             capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE)
            ctx.sync()

        ms, upload, tests, ran = {k: [] for k in trees}, {k: [] for k in trees}, {}, {}
        for run in range(args.frame_runs):
            for k, nodes in trees.items():
                t0 = time.perf_counter()
                ctx.upload_bvh(nodes)
                upload[k].append(time.perf_counter() - t0)
                ctx.reset()
                batch(2)                                   # warm-up: the scene analysis, the kernel build for this tree
                ctx.reset_counters()
                t0 = time.perf_counter()
                batch(2 + args.batch)
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.batch)
                c = ctx.counters()
                tests[k] = (c["box_tests"] / c["rays"], c["tri_tests"] / c["rays"], c["stack_overflows"], c["rays"])
                ran[k] = ctx.last_launch()
            say(f"frame run {run}: " + "   ".join(f"{k} {ms[k][-1]:.3f} ms" for k in trees))
        say("-- frames, medians of %d: ms per frame [min .. max], Mrays/s, box + triangle tests per ray (the counters of the walk that ran, "
            "named under `launch`), upload_bvh s, the launch" % args.frame_runs)
        for k in trees:
            box, tri, aborts, rays = tests[k]
            say(f"{k:9s} {med(ms[k]):8.3f} [{min(ms[k]):.3f} .. {max(ms[k]):.3f}]   {rays / args.batch / med(ms[k]) / 1e3:7.0f} Mrays/s   "
                f"{box:6.2f} + {tri:5.2f}   aborts {aborts}   upload {med(upload[k]):.2f} s   {ran[k]}")
        base = med(ms["host sah"])
        say("frame time over the host SAH tree's: " + "   ".join(f"{k} {med(ms[k]) / base:.3f}" for k in trees if k != "host sah"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
