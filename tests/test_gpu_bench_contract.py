"""bench.py end to end: the one JSON line the driver reads (metric / value / unit / n_gpus / steps /
warmup / ms_per_step / higher_is_better / scaling / vs_baseline / dtype / data / config; with --full
also roofline + cpu_baseline), for N = 1 and -- as a rehearsal of the multi-GPU path on one device, two ranks
over gloo -- for N = 2."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _line(out):
    """ONE line on stdout, the JSON one (round 6: gloo's "[Gloo] Rank 0 is connected ..." used to share rank 0's stdout with it -- bench.py now
    keeps the real stdout aside and points file descriptor 1 at stderr while it runs)."""
    assert out.strip().count("\n") == 0, out[-2000:]
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def test_single_gpu_line():
    """The driver's own arguments (--steps 20 --warmup 5; a step = 16 frames, up to sixteen steps per launch): the headline is
    the ~870k-triangle scene the target is quoted on; the roofline fraction comes from counter passes
    of this very command line and is a fraction; the launch statistics are consistent with the wall clock."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5", "--full"],
                       capture_output=True, text=True, timeout=1100, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _line(r.stdout)
    assert j["metric"] == "Mrays/s" and j["unit"] == "Mrays/s" and j["higher_is_better"] is True
    assert (j["n_gpus"], j["steps"], j["warmup"]) == (1, 20, 5) and j["vs_baseline"] is None
    assert j["scaling"] == "strong" and j["dtype"] == "f32" and j["data"] == "synthetic"
    assert "workload" in j["config"] and "model" not in j["config"] and j["config"]["image"] == [1920, 1080]
    assert j["config"]["triangles"] > 800_000 and "dragon-class" in j["config"]["workload"] and j["config"]["frames_per_step"] == 16
    assert j["value"] > 1000 and abs(j["value"] - j["config"]["rays_per_step"] / j["ms_per_step"] / 1e3) / j["value"] < 0.01
    roof = j["roofline"]
    # the roof that binds: vector-ALU lane-operations (round-2 verdict: not "hbm" for a scene that fits the Infinity Cache)
    assert roof["bound"] == "valu" and roof["unit"] == "Tlane-op/s" and abs(roof["peak"] - 78.643) < 0.01
    # the 320 timed frames are two EQUAL launches of 160 (round-5 verdict: 256 + 64 ran two different builds of the kernel and every
    # per-launch figure averaged the two): one instantiation, named with its waves per SIMD, one block per launch
    assert roof["kernel_ms"] > 0 and roof["launches_timed"] == 2 and roof["frames_per_launch"] == 160.0
    assert len(roof["launches"]) == 2 and all(b["frames"] == 160.0 and b["waves_per_simd"] == 6 for b in roof["launches"])
    assert roof["launches"][0]["instantiation"] == roof["launches"][1]["instantiation"]
    assert roof["launches"][0]["instantiation"] == "k_raytrace_sm<true,true,true,true,true,false,false,false,true,32,6>"       # as rocprofv3 prints it (MI3PT_OPT_LAST_BUILD)
    assert "false,false,false,true,44,6>" in j["forest"]["roofline"]["launches"][0]["instantiation"]                         # the deep-tree build, three-axis culling
    assert "6 waves per SIMD" in roof["real_bound"] and "5 waves" not in roof["real_bound"]
    # three fractions by three rules, at top level: what binds (VALU), north_star's counter-based HBM side (requested bytes, and the
    # upper bound if every request moved its 128-byte class), SURVEY 8(d)'s algorithmic bytes over the HBM peak (cache-served: > 1)
    by = roof["frac_by_rule"]
    assert by["valu"] == roof["frac"] and by["hbm_counter"] == roof["hbm"]["frac"] and set(by["rules"]) == {"valu", "hbm_counter", "hbm_counter_upper", "survey_8d_algorithmic"}
    assert 0 < by["hbm_counter"] <= by["hbm_counter_upper"] <= 1 and by["survey_8d_algorithmic"] > 1
    assert abs(by["hbm_counter_upper"] - roof["hbm"]["upper_frac"]) < 1e-9
    req = roof["fabric_read_requests"]
    assert req and req["requests_128B"] > 0 and req["requests_32B"] + req["requests_64B"] + req["requests_128B"] <= 1.01 * req["requests"]
    assert roof["traffic"] < roof["traffic_if_every_request_moves_its_size_class"] <= 2.05 * roof["traffic"]
    # the non-overlapped kernel time per frame cannot exceed the wall clock per frame
    assert roof["kernel_ms_exclusive"] / 10 <= j["ms_per_step"] * 1.02         # (a launch per ten steps, on average)
    assert roof["kernel_ms_exclusive"] <= roof["kernel_ms"] * 1.02
    # the average over every launch of the process (what `rocprofv3 --stats` averages): the warm-up's 80 frames are one launch
    assert roof["launches_all"] == 3 and 0 < roof["kernel_ms_all_launches"] < roof["kernel_ms"]
    # measured by this run (rocprofv3 is on the box): the issue figures, HBM-side traffic, L2 requests -- all fractions
    assert 0 < roof["frac"] <= 1 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 2e-3
    assert 0 < roof["valu_issue_frac"] < 1 and 0 < roof["lane_utilisation"] <= 1
    assert abs(roof["frac"] - roof["valu_issue_frac"] * roof["lane_utilisation"]) < 2e-3
    assert roof["traffic"] is not None and roof["traffic"] > 0, roof.get("pmc_log")
    assert roof["hbm"]["peak"] == 8000.0 and 0 < roof["hbm"]["frac"] <= 1
    assert abs(roof["hbm"]["achieved"] - roof["traffic"] / (roof["kernel_ms_exclusive"] * 1e-3) / 1e9) / roof["hbm"]["achieved"] < 1e-3
    assert 0 < roof["l2"]["frac"] <= 1 and 0 < roof["l2"]["hit_rate"] < 1
    assert roof["algorithmic_GBps"] > 0 and roof["box_tests_per_ray"] > 1
    assert j["also"]["demo"]["value"] > 1000
    # the whole render() per frame (raytrace + accumulate + fullscreen): slower than the two passes alone, and more than a quarter of it
    assert j["also"]["demo"]["value"] / 4 < j["also"]["demo_presenting_every_frame"]["value"] < j["also"]["demo"]["value"]
    # the same scene from close up: every pixel's walk goes deep into the 870 k-triangle tree (the stated view is dominated
    # by sky and floor segments: 16 box tests per ray there, ~65 here)
    close = j["also"]["closeup"]
    assert close["value"] > 1000 and close["rays_per_pixel"] > 2.0 and close["box_tests_per_ray"] > 2 * roof["box_tests_per_ray"]
    # config 5's scene, the one larger than the Infinity Cache: its own counter passes
    forest = j["forest"]
    assert forest["value"] > 100 and forest["scene_bytes"] > 1.5e9 and "forest" in forest["workload"]
    fr = forest["roofline"]
    assert fr["traffic"] is not None and fr["traffic"] > 0, fr.get("pmc_log")
    assert 0 < fr["hbm"]["frac"] <= 1 and 0 < fr["frac"] <= 1 and 0 < fr["l2"]["hit_rate"] < 1
    cpu = j["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["unit"] == "Mrays/s" and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"]
    assert "1" in cpu["thread_scaling_Mrays_per_s"] and cpu["value"] == max(cpu["thread_scaling_Mrays_per_s"].values())


def test_plain_line_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """Without --full the line carries the headline and nothing measured beside it, and the run spends less than 30 s outside its
    steps (build check, torch, the ~870k-triangle scene and its BVH, uploads); --dump-outputs writes what the last timed step left
    for a caller (the accumulation image, the ray counts of the timed steps), the same bits from run to run."""
    dumps = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        t0 = time.monotonic()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        wall = time.monotonic() - t0
        assert r.returncode == 0, r.stderr[-2000:]
        j = _line(r.stdout)
        assert "dragon-class" in j["config"]["workload"] and wall - (3 + 1) * j["ms_per_step"] / 1e3 < 30.0, wall
        assert (j["metric"], j["unit"], j["higher_is_better"], j["dtype"], j["steps"], j["warmup"]) == ("Mrays/s", "Mrays/s", True, "f32", 3, 1)
        assert j["value"] > 100 and abs(j["value"] - j["config"]["rays_per_step"] / j["ms_per_step"] / 1e3) / j["value"] < 0.01
        assert not {"roofline", "also", "forest", "cpu_baseline", "gather_check"} & set(j)
        assert sorted(os.listdir(d)) == ["accumulation.npy", "ray_counts.npy"]
        img, counts = np.load(d / "accumulation.npy"), np.load(d / "ray_counts.npy")
        assert img.dtype == np.float32 and img.shape == (1080, 1920, 4) and np.isfinite(img).all() and img[..., :3].max() > 0
        assert counts.dtype == np.float64 and counts[0] // 3 == j["config"]["rays_per_step"] and counts[0] == counts[1] + counts[2]
        assert counts[3] == 1920 * 1080 * 3 * 16
        dumps.append((img, counts))
    assert np.array_equal(dumps[0][0].view(np.uint32), dumps[1][0].view(np.uint32)) and np.array_equal(dumps[0][1], dumps[1][1])


PLAIN = [sys.executable, os.path.join(ROOT, "bench.py")]          # `python bench.py --gpus N`: bench.py launches its own ranks (round-5 verdict, next #1)
TORCHRUN = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
            "--master-port", "29533", os.path.join(ROOT, "bench.py")]   # the launcher form of the contract: keeps working


@pytest.mark.parametrize("launcher,scaling,image", [(PLAIN, "strong", [1920, 1080]), (TORCHRUN, "weak", [1920, 2160])],
                         ids=["plain-strong", "torchrun-weak"])
def test_two_rank_rehearsal_line(launcher, scaling, image):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["MI3PT_BENCH_REHEARSAL"] = "1"
    r = subprocess.run([*launcher, "--gpus", "2", "--steps", "4", "--warmup", "1", "--scaling", scaling, "--workload", "demo", "--full"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _line(r.stdout)
    assert (j["n_gpus"], j["steps"], j["scaling"]) == (2, 4, scaling) and j["config"]["image"] == image and "cpu_baseline" not in j
    assert "tile-split x2" in j["config"]["parallelism"] and j["value"] > 100
    assert j["config"]["frames_per_launch"] == 64.0         # 4 steps = 64 frames: one launch (a rank of a 2-way split batches up to 512)
    # per rank: wall time, host time until everything was launched, GPU-clock span of the raytrace launches, its part of the gather
    ranks = j["config"]["per_rank"]
    assert len(ranks) == 2 and sum(r["rows"] for r in ranks) == image[1]
    for r in ranks:
        assert 0 < r["submit_ms"] < r["elapsed_ms"] and 0 < r["launch_span_ms"] < r["elapsed_ms"] and r["gather_ms"] > 0
    assert j["config"]["host_threads_per_rank"] >= 1
    # the gathered image is the right image: rank 0 rendered rank 1's share again and compared (round-4 verdict, next #2b)
    assert j["gather_verified"] is True and j["gather_check"]["ranks_rerendered"] == [1] and j["gather_check"]["own_rows_identical"] is True
    assert j["gather_check"]["frames"] == 5 * 16 and j["gather_check"]["rows"] == [ranks[1]["rows"]]


def test_two_rank_rehearsal_of_the_headline_job_carries_a_roofline():
    """The line the driver's SCALE run will print for N = 2 (its arguments, the headline scene), rehearsed with both ranks on
    this box's one GPU: `roofline` must not be empty for N > 1 (round-4 verdict, next #2a) -- its counters come from the
    committed measurement of the same split rendered rank by rank on one GPU (profiles/traffic.json, n_gpus 2), its kernel
    time from rank 0's live HIP events -- and the gathered image is verified."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["MI3PT_BENCH_REHEARSAL"] = "1"
    r = subprocess.run([*PLAIN, "--gpus", "2", "--steps", "20", "--warmup", "5", "--full"],          # exactly the BENCH record's command shape, N = 2
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _line(r.stdout)
    assert (j["n_gpus"], j["steps"], j["warmup"], j["scaling"]) == (2, 20, 5, "strong") and "dragon-class" in j["config"]["workload"]
    assert j["gather_verified"] is True and j["gather_check"]["frames"] == 400
    roof = j["roofline"]
    assert roof["frames_per_launch"] == 320.0 and roof["launches_timed"] == 1
    assert roof["frac"] is not None and roof["frac"] > 0 and roof["traffic"] is not None and roof["traffic"] > 0
    assert roof["hbm"]["frac"] is not None and roof["lane_utilisation"] > 0.3
    assert "rank-of-2 shape measured on one GPU" in roof["traffic_source"] and "ONE GPU of the 2" in roof["scope"]
    assert "cpu_baseline" not in j and "forest" not in j


def test_rccl_path_with_a_world_of_one():
    """What a one-GPU box can run of the REAL multi-GPU path: torch.distributed over RCCL ('nccl'), the gather of the device-resident
    accumulation image on the context's stream inside the timed region, the reductions of timings and counters -- with a world of one
    (two ranks on one GPU are refused by RCCL: the N = 2 rehearsals above go over gloo).  Same job, same rays, same image as the plain
    single-GPU run."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["MI3PT_BENCH_RCCL_SELFTEST"] = "1"
    args = ["--steps", "4", "--warmup", "1", "--workload", "demo", "--no-pmc", "--no-cpu-baseline", "--no-also", "--no-forest"]
    r = subprocess.run([*PLAIN, *args, "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _line(r.stdout)
    assert "RCCL" in j["rccl_selftest"] and j["n_gpus"] == 1
    assert j["gather_verified"] is True and j["gather_check"]["own_rows_identical"] is True and j["gather_check"]["ranks_rerendered"] == []
    rank0 = j["config"]["per_rank"][0]
    assert rank0["gather_ms"] is not None and rank0["gather_ms"] > 0 and rank0["rows"] == 1080
    plain = subprocess.run([*PLAIN, *args], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert _line(plain.stdout)["config"]["rays_per_step"] == j["config"]["rays_per_step"]


def test_device_group_rehearsal_line():
    """`bench.py --gpus 2 --group`: one process, the library's own tile split and peer-copy gather (mi3pt_create_group) -- here
    with both members on the box's one GPU.  Same job, same rays as two processes over torch.distributed."""
    env = dict(os.environ, MI3PT_BENCH_REHEARSAL="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--group", "--steps", "4", "--warmup", "1", "--workload", "demo",
                        "--no-pmc", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _line(r.stdout)
    assert (j["n_gpus"], j["steps"], j["scaling"]) == (2, 4, "strong") and j["config"]["image"] == [1920, 1080]
    assert "device group" in j["config"]["parallelism"] and j["value"] > 100
    assert j["gather_verified"] is True and j["gather_check"]["ranks_rerendered"] == [1]
    single = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--workload", "demo", "--no-pmc", "--no-cpu-baseline"],
                            capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert _line(single.stdout)["config"]["rays_per_step"] == j["config"]["rays_per_step"]


def test_strong_and_weak_scaling_agree_on_one_gpu():
    vals = {}
    for scaling in ("strong", "weak"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "1", "--scaling", scaling,
                            "--workload", "demo", "--no-pmc", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        j = _line(r.stdout)
        assert j["config"]["image"] == [1920, 1080] and j["scaling"] == scaling
        vals[scaling] = (j["value"], j["config"]["rays_per_step"])
    assert vals["strong"][1] == vals["weak"][1]                              # the same job
    assert abs(vals["strong"][0] - vals["weak"][0]) / vals["weak"][0] < 0.1  # the same speed (run-to-run noise)
