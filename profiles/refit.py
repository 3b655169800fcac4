"""Is the device refit faster than the host build it replaces?  (needs a HIP device)

One process, scenes.dragon_class_scene() (869 882 triangles) with every vertex of the model moved (the ground plane stays): per side
five timings, the sides alternating, after one warm-up each:

    refit   wall time of Context.device_refit_bvh() -- queue flush, allocation, the device work, the copy of nnodes x 48 B to the host,
            the free -- and its own device time (refit_ms: device events around the copy, the parent table, the zeroing and the fit)
    build   wall time of capi.host_build_bvh_f64 on the same positions: what RaytracePass.updateScene runs without `refit`

Both leave 48-byte records on the host, ready for upload_bvh; the upload itself (its host compile and the scene analysis) is the same on
both sides and is not timed.  The re-fitted records are held to the law (tests/refit_reference.py) once, outside the timed window.
The claim to confirm is only that the call is faster than the build by more than the spread of the runs.

    python profiles/refit.py [--runs 5] [--log profiles/refit.log]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--segments", type=int, default=660)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "0")),
                    help="builder threads of the host build (0: the hardware concurrency, what the hosts pass; default: OMP_NUM_THREADS when "
                         "set -- a machine that grants fewer CPUs than it shows says so there, and a pool sized by what it shows only slows the build down)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "refit.log"))
    args = ap.parse_args()
    ge.build()
    import refit_reference as rr
    from mi3pt_host import capi, layout, scenes

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    sc = scenes.dragon_class_scene(args.segments)
    t0 = time.perf_counter()
    sc.build_bvh()
    say(f"{sc.name}: {len(sc.triangles)} triangles, {len(sc.nodes)} nodes; first build {time.perf_counter() - t0:.3f} s")
    # every vertex of the model moved: a rigid turn about y by 10 degrees plus a bend along y (the ground plane, triangles 0 and 1, stays)
    pos = np.array(sc.positions)
    model = pos[2:]
    a = np.radians(10.0) + 0.3 * model[..., 1]
    x, z = model[..., 0].copy(), model[..., 2].copy()
    model[..., 0], model[..., 2] = np.cos(a) * x + np.sin(a) * z + 0.05, -np.sin(a) * x + np.cos(a) * z
    moved = layout.pack_triangles(pos, sc.normals, sc.material_index)
    want = rr.refit_vectorised(sc.nodes, moved)
    with capi.Context(0) as ctx:
        say(capi.device_name(0))
        ctx.upload_bvh(sc.nodes)
        ctx.upload_triangles(sc.triangles)
        ctx.upload_materials(sc.material_bytes)
        ctx.upload_triangles(moved)
        nodes, _ = ctx.device_refit_bvh()                  # warm-up (code object, first allocation), and the check
        diff = rr.first_difference(nodes, want)
        say("re-fitted records equal the law's word for word" if diff is None else "RE-FITTED RECORDS DIFFER FROM THE LAW: " + diff)
        rebuilt = capi.host_build_bvh_f64(pos, args.threads)              # warm-up (thread pool, page faults)
        say(f"host_bvh_cost: first build {capi.host_bvh_cost(sc.nodes):.3f}, re-fitted {capi.host_bvh_cost(nodes):.3f}, rebuilt {capi.host_bvh_cost(rebuilt):.3f}")
        refit_wall, refit_dev, build_wall = [], [], []
        for run in range(args.runs):
            t0 = time.perf_counter()
            nodes, ms = ctx.device_refit_bvh()             # (blocks until the records are on the host)
            refit_wall.append((time.perf_counter() - t0) * 1e3)
            refit_dev.append(ms)
            t0 = time.perf_counter()
            capi.host_build_bvh_f64(pos, args.threads)
            build_wall.append((time.perf_counter() - t0) * 1e3)
            say(f"run {run}: refit wall {refit_wall[-1]:9.3f} ms (device {ms:7.3f} ms)   host build wall {build_wall[-1]:9.3f} ms")
    med = lambda v: float(np.median(v))
    say(f"refit wall  ms: median {med(refit_wall):.3f}, min {min(refit_wall):.3f}, max {max(refit_wall):.3f}")
    say(f"refit device ms: median {med(refit_dev):.3f}, min {min(refit_dev):.3f}, max {max(refit_dev):.3f}")
    say(f"host build  ms: median {med(build_wall):.3f}, min {min(build_wall):.3f}, max {max(build_wall):.3f}  ({os.cpu_count()} host CPUs visible, builder threads: {args.threads or 'hardware concurrency'})")
    say(f"ratio host build / refit wall: median {med(build_wall) / med(refit_wall):.1f} x; slowest refit against fastest build: "
        f"{min(build_wall) / max(refit_wall):.1f} x")
    traffic = len(sc.triangles) * 112 + len(sc.nodes) * (48 * 3 + 4 * 3)
    say(f"device traffic of the fit, counted from shapes: {traffic / 1e6:.1f} MB -> {traffic / 1e6 / med(refit_dev):.1f} GB/s over the device time")
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if diff is None else 1


if __name__ == "__main__":
    sys.exit(main())
