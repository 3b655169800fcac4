"""`python bench.py --gpus N` run plain (no torch.distributed.run around it) launches its own ranks: bench.self_launch.
Here, without a GPU: the launcher starts N children with the rendezvous variables set, relays their failure ("needs a HIP
device": there is no CPU fallback) as a non-zero exit code, and never prints the old "launch with: ..." refusal.
The GPU form of the same command is tests/test_gpu_bench_contract.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_multi_gpu_command_launches_its_own_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", MI3PT_BENCH_ECHO_RANK="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "demo"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode not in (0, None)
    assert "launch with" not in r.stderr and "launch with" not in r.stdout
    # both ranks started, each with its own RANK of WORLD_SIZE 2 and the same rendezvous on 127.0.0.1, and each failed loudly
    ranks = sorted(l for l in r.stderr.splitlines() if l.startswith("bench.py rank "))
    assert len(ranks) == 2 and ranks[0].startswith("bench.py rank 0/2 ") and ranks[1].startswith("bench.py rank 1/2 ")
    assert ranks[0].split("rendezvous ")[1] == ranks[1].split("rendezvous ")[1] and "127.0.0.1:" in ranks[0]
    assert r.stderr.count("needs a HIP device") == 2
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_launcher_env_of_a_wrapped_run_is_left_alone():
    """Under torch.distributed.run (WORLD_SIZE set) bench.py must not launch anything itself."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="1", LOCAL_RANK="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999",
               HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", MI3PT_BENCH_ECHO_RANK="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "demo"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and r.stderr.count("needs a HIP device") == 1
    assert [l for l in r.stderr.splitlines() if l.startswith("bench.py rank ")] == ["bench.py rank 1/2 local 1 rendezvous 127.0.0.1:29999"]


def test_dumped_outputs_stay_within_their_size_and_sample_the_same_pixels(tmp_path):
    """bench.write_outputs (--dump-outputs): an image above the limit becomes a seeded sample of its pixels with their indices,
    the same pixels on every run; small arrays are written whole."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    img = np.arange(4320 * 3840 * 4, dtype=np.float32).reshape(4320, 3840, 4)          # weak scaling at N = 8
    counts = np.array([5.0, 3.0, 2.0, 7.0])
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"accumulation": img, "ray_counts": counts})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["accumulation.npy", "accumulation_pixel_index.npy", "ray_counts.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    sample, index = np.load(tmp_path / "a" / "accumulation.npy"), np.load(tmp_path / "a" / "accumulation_pixel_index.npy")
    assert sample.dtype == np.float32 and index.dtype == np.float64 and len(sample) == len(index) > 1_000_000
    assert np.array_equal(sample, img.reshape(-1, 4)[index.astype(np.int64)]) and np.all(np.diff(index) > 0)
    for f in files:
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f
    assert np.array_equal(np.load(tmp_path / "a" / "ray_counts.npy"), counts)
    small = img[:1080, :1920]
    bench.write_outputs(str(tmp_path / "c"), {"accumulation": small, "ray_counts": counts})
    assert sorted(os.listdir(tmp_path / "c")) == ["accumulation.npy", "ray_counts.npy"]
    assert np.array_equal(np.load(tmp_path / "c" / "accumulation.npy"), small)


def test_dumped_outputs_are_finite_and_list_what_was_not(tmp_path):
    """A long run can leave NaN pixels in the accumulation image (the reference's log(0) when rand() returns 0, kept bit for bit):
    bench.write_outputs writes them as 0 and lists each one exactly -- flat element index, 1 = NaN, 2 = +inf, 3 = -inf."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    img = np.linspace(0.0, 2.0, 6 * 5 * 4, dtype=np.float32).reshape(6, 5, 4)
    img[1, 2, :3] = np.nan
    img[3, 4, 0] = np.inf
    img[0, 0, 1] = -np.inf
    bench.write_outputs(str(tmp_path), {"accumulation": img, "ray_counts": np.array([5.0, 3.0, 2.0, 7.0])})
    assert sorted(os.listdir(tmp_path)) == ["accumulation.npy", "accumulation_nonfinite.npy", "ray_counts.npy"]
    got, listed = np.load(tmp_path / "accumulation.npy"), np.load(tmp_path / "accumulation_nonfinite.npy")
    assert np.isfinite(got).all() and np.isfinite(listed).all() and listed.dtype == np.float64
    assert listed.tolist() == [[1.0, 3.0], [28.0, 1.0], [29.0, 1.0], [30.0, 1.0], [76.0, 2.0]]
    bad = ~np.isfinite(img)
    assert np.array_equal(got[~bad], img[~bad]) and (got[bad] == 0).all()
