"""Caller-owned streams and zero-copy pointers (include/mi3pt.h: mi3pt_set_stream, mi3pt_flush, the *_device_ptr entry points,
mi3pt_bind_accumulation) against the oracle, bit for bit.

Every other GPU test looks at the device after a blocking call, and a blocking call waits for everything: work the library put
on a wrong stream, or behind no event, still shows the right image.  Here a PyTorch host drives a context the way the header
promises it can: torch's stream is the context's stream, nothing blocks between the first enqueue and one
stream.synchronize(), and the results are torch tensors cloned ON that stream.

What makes a lost dependency show.  Each ordering scenario first puts a delay on the caller's stream (torch.cuda._sleep,
calibrated with two events), 20 x the device time the same job took without it (no less than 50 ms, no more than 500 ms: clear of
the 2000 ms after which a blocking call releases the launch gate from the host).  Work that escaped the stream then runs -- and
ends -- while the stream still sleeps: an ordered mean that ran elsewhere finds neither the checkpoint nor this job's radiance,
a clone that ran early finds the image of the run before.  The measuring runs use other random sequences (raytrace `frame` +
1000), so what they leave in the radiance slots and images is wrong for the run that counts.  Right after the last enqueue the
event behind the delay and the event at the very end must both be unfinished: the host did not wait and nothing had run yet.

torch and a context share a process only in a spawned child (torch's HIP runtime is loaded first); ONE child runs every
scenario and returns numpy arrays and flags, the tests below assert on them.  The reference is the oracle (sample frames, running
mean, canvas) and the numpy restatements beside this file (feature images, guided filter, moments), computed in the parent.  The
child also renders every job on an ordinary context -- own stream, blocking read-backs -- and that must equal the oracle too: a
scenario that fails while its ordinary twin passes has lost a dependency, not a bit.

Shape: demo scene, 100 x 52 (no multiple of 16, ragged 8 x 8 tiles), 3 bounces, frames 5 .. 14, MI3PT_OPT_BATCH 4: launches of 4,
4 and 2 frames on both internal raytrace streams, the third behind the slot set's acc_done event recorded on the caller's stream.
"""
import os
import queue as queue_mod
import sys
import time
import traceback

import numpy as np
import pytest

import aov_reference
import guided_reference as gr
import moments_reference as mr
import ptcommon as pc
from mi3pt_host import capi

pytestmark = pytest.mark.gpu

W, H, BOUNCES, FIRST, COUNT, BATCH = 100, 52, 3, 5, 10, 4
LEVELS, SIGMAS = 3, (4.0, 0.35, 0.1, 0.05)        # tests/test_gpu_guided.py: ALL_ON, three levels
OTHER_SEQUENCE = 1000                              # raytrace `frame` offset of the runs that only measure
DELAY_FACTOR, DELAY_MIN_MS, DELAY_MAX_MS = 20.0, 50.0, 500.0
RT_ACC = capi.SUBMIT_RAYTRACE | capi.SUBMIT_ACCUMULATE
NAMES = capi.AOV_NAMES


def _checkpoint():
    """the image a job continues from: seeded finite fp32 colours in [0, 4), alpha 1"""
    c = (np.random.default_rng(20261018).random((H, W, 4), dtype=np.float32) * np.float32(4)).astype(np.float32)
    c[..., 3] = np.float32(1)
    return c


def _fs_bytes():
    return pc.fs_uniforms(W, H, 1.0, 1, 1).tobytes()          # de-noise on, ACES


class _DeviceArray:
    """a device pointer as __cuda_array_interface__ (version 2): what torch.as_tensor wraps without a copy"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"version": 2, "shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "strides": None}


def _scenarios():
    """Runs in the spawned child.  Returns {name: numpy array | bool | number}."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (os.path.join(root, "webgpu-pathtracer_amd", "py"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ctypes

    import torch                                   # first: its HIP runtime is the process's
    from mi3pt_host import scenes

    out = {}
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    Event = torch.cuda.Event
    sc = scenes.demo_scene()
    sc.build_bvh(nthreads=2)
    env = scenes.synthetic_env()
    ckpt = _checkpoint()
    ckpt_t = torch.from_numpy(ckpt).to(dev)
    torch.cuda.synchronize()
    out["default_stream_handle"] = int(torch.cuda.default_stream().cuda_stream)

    # ---- the delay: torch.cuda._sleep spins for a number of clock ticks; two events say how long a tick is ----
    cal = torch.cuda.Stream()

    def timed_sleep(ticks):
        a, b = Event(enable_timing=True), Event(enable_timing=True)
        with torch.cuda.stream(cal):
            a.record()
            torch.cuda._sleep(int(ticks))
            b.record()
        cal.synchronize()
        return a.elapsed_time(b)

    timed_sleep(100_000)                                                    # (the kernel's first launch)
    coarse = max(timed_sleep(1_000_000), 1e-3)                              # ticks for about 20 ms, measured once more
    ticks = int(1_000_000 * 20.0 / coarse)
    ticks_per_ms = ticks / timed_sleep(ticks)
    out["ticks_per_ms"] = float(ticks_per_ms)
    print(f"streams: torch.cuda._sleep calibrated: {ticks_per_ms:.1f} ticks per ms ({ticks} ticks measured)", flush=True)

    def make_ctx():
        ctx = capi.Context(0)
        ctx.set_option(capi.OPT_BATCH, BATCH)
        pc.upload_scene(ctx, sc, env)
        ctx.resize(W, H)
        assert ctx.batch_capacity() == BATCH
        # (a whole job and a wait: the scene analysis blocks, and so does the first launch of a depth -- a slot set that grows is
        # freed, and hipFree waits for the whole device, sleeping streams of the caller's included: both belong in front of every delay)
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, W, H, frame=OTHER_SEQUENCE, bounces=BOUNCES).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, 1).tobytes())
        ctx.submit_frames(RT_ACC, COUNT)
        ctx.sync()
        return ctx

    def frames(ctx, rt_first, acc_first, n, mask=RT_ACC):
        ctx.set_uniforms(capi.PASS_RAYTRACE, pc.rt_uniforms(sc, W, H, frame=rt_first, bounces=BOUNCES).tobytes())
        ctx.set_uniforms(capi.PASS_ACCUMULATE, pc.acc_uniforms(W, H, acc_first).tobytes())
        ctx.submit_frames(mask, n)

    def ordered(name, stream, prepare, enqueue):
        """prepare(): the blocking set-up, before every run.  enqueue(rt_offset): the chain, nothing blocking in it.  Two runs without
        the delay (the second is timed: the first also allocates), then the run that counts."""
        for _ in range(2):
            prepare()
            torch.cuda.synchronize()
            t0, t1 = Event(enable_timing=True), Event(enable_timing=True)
            with torch.cuda.stream(stream):
                t0.record()
                enqueue(OTHER_SEQUENCE)
                t1.record()
            stream.synchronize()
        job_ms = t0.elapsed_time(t1)
        delay_ms = min(max(DELAY_FACTOR * job_ms, DELAY_MIN_MS), DELAY_MAX_MS)
        prepare()
        torch.cuda.synchronize()
        behind, end = Event(), Event()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(delay_ms * ticks_per_ms))
            behind.record()
            res = enqueue(0)
            end.record()
        behind_done, end_done = behind.query(), end.query()
        stream.synchronize()                                                # exactly once
        out[name + "_nothing_had_run"] = (not behind_done) and (not end_done)
        out[name + "_job_ms"], out[name + "_delay_ms"] = float(job_ms), float(delay_ms)
        print(f"streams: {name}: job {job_ms:.3f} ms without the delay, delay {delay_ms:.1f} ms = {int(delay_ms * ticks_per_ms)} ticks; "
              f"right after the last enqueue: event behind the delay done {behind_done}, end event done {end_done}", flush=True)
        return res

    def host(t):
        return t.cpu().numpy()

    S = torch.cuda.Stream()

    # ---- 1, 2, 4, 5: a bound torch tensor is the running mean ----
    ctx1 = make_ctx()
    accum = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx1.set_stream(S.cuda_stream)
    ctx1.bind_accumulation(accum.data_ptr(), accum.numel() * 4)

    def scrub():
        accum.fill_(-7.0)                                                   # neither zeros, nor the checkpoint, nor a mean

    def producer(off):
        accum.copy_(ckpt_t, non_blocking=True)
        frames(ctx1, FIRST + off, FIRST, COUNT)
        ctx1.flush()
        return accum.clone()

    out["s1_mean"] = host(ordered("s1", S, scrub, producer))

    def with_reset(off):
        ctx1.reset()
        frames(ctx1, 1 + off, 1, COUNT)
        ctx1.flush()
        return accum.clone()

    out["s2_mean"] = host(ordered("s2", S, lambda: accum.copy_(ckpt_t), with_reset))

    def presenting(off):
        snap = producer(off)
        ctx1.set_uniforms(capi.PASS_FULLSCREEN, _fs_bytes())
        ctx1.submit(capi.SUBMIT_FULLSCREEN)
        return snap

    out["s4_mean"] = host(ordered("s4", S, scrub, presenting))
    out["s4_canvas8"] = ctx1.read_canvas_rgba8()
    out["s4_canvas"] = ctx1.read_texture(capi.TEX_CANVAS)

    ctx1.set_pipelining(False)
    for variant in (2, 0):
        ctx1.set_kernel_variant(variant)
        out[f"s5_v{variant}_mean"] = host(ordered(f"s5_v{variant}", S, scrub, producer))
        out[f"s5_v{variant}_kind"] = ctx1.last_launch()["kind"]
    ctx1.set_kernel_variant(0)
    ctx1.set_pipelining(True)

    # ---- 8b: pass times on a caller's stream (ten presenting frames: every frame has its own mean and canvas) ----
    ctx1.enable_timing(True)
    ctx1.set_uniforms(capi.PASS_FULLSCREEN, _fs_bytes())
    frames(ctx1, FIRST, FIRST, COUNT, RT_ACC | capi.SUBMIT_FULLSCREEN)
    for k, name in ((capi.PASS_RAYTRACE, "raytrace"), (capi.PASS_ACCUMULATE, "accumulate"), (capi.PASS_FULLSCREEN, "fullscreen")):
        out["s8_time_" + name] = float(ctx1.pass_time_us(k))
    ctx1.enable_timing(False)
    ctx1.bind_accumulation(None, 0)
    ctx1.close()

    # ---- 3: consumer order through every zero-copy pointer ----
    ctx3 = make_ctx()
    ctx3.set_moments(True)
    ctx3.set_stream(S.cuda_stream)
    acc_ptr, acc_bytes = ctx3.accumulation_device_ptr()                     # valid from mi3pt_resize on
    mom_ptr, mom_bytes = ctx3.moments_device_ptr()                          # valid from mi3pt_set_moments on
    assert acc_bytes == mom_bytes == H * W * 16
    try:
        probe = torch.as_tensor(_DeviceArray(acc_ptr, (H, W, 4), "<f4"), device=dev)
        wraps = probe.data_ptr() == acc_ptr and probe.dtype == torch.float32 and tuple(probe.shape) == (H, W, 4)
        refusal = "" if wraps else "torch.as_tensor copied the array"
    except Exception as e:          # (this torch refuses the interface: the copies below go through the HIP runtime torch has mapped)
        wraps, refusal = False, repr(e)
    out["wrap_zero_copy"] = bool(wraps)
    print(f"streams: __cuda_array_interface__ wrapped without a copy: {wraps} {refusal}", flush=True)
    hip = None
    if not wraps:
        hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    def clone_of(ptr, typestr):
        """a copy of the image at `ptr`, made on the current stream"""
        if wraps:
            return torch.as_tensor(_DeviceArray(ptr, (H, W, 4), typestr), device=dev).clone()
        dst = torch.empty((H, W, 4), dtype=torch.int32 if typestr == "<i4" else torch.float32, device=dev)
        rc = hip.hipMemcpyAsync(dst.data_ptr(), ptr, H * W * 16, 3, torch.cuda.current_stream().cuda_stream)      # 3: device to device
        assert rc == 0, f"hipMemcpyAsync: {rc}"
        return dst

    def consumer(off):
        frames(ctx3, FIRST + off, FIRST, COUNT)
        ctx3.flush()
        ctx3.render_aovs(capi.AOV_ALL)
        ctx3.denoise_guided(LEVELS, *SIGMAS)
        got = {"accum": clone_of(acc_ptr, "<f4"), "moments": clone_of(mom_ptr, "<f4")}
        for k, name in enumerate(NAMES):
            ptr, n = ctx3.aov_device_ptr(k)                                 # valid once rendered
            assert n == H * W * 16
            got[name] = clone_of(ptr, "<i4" if k == capi.AOV_IDS else "<f4")
        ptr, n = ctx3.guided_device_ptr()                                   # valid until the next filter
        assert n == H * W * 16
        got["guided"] = clone_of(ptr, "<f4")
        return got

    def start_over():
        # mi3pt_write_texture blocks, copies the checkpoint and zeroes the moments: the state every run starts from.  The feature images
        # do not depend on the random sequence: what the run before left in them is scrubbed through the same zero-copy tensors
        ctx3.write_texture(capi.TEX_ACCUMULATION, ckpt)
        for k in range(capi.AOV_COUNT if wraps else 0):
            try:
                ptr, _ = ctx3.aov_device_ptr(k)
            except capi.Mi3ptError:
                break                                                       # (not rendered yet: the first run)
            torch.as_tensor(_DeviceArray(ptr, (H, W, 4), "<i4" if k == capi.AOV_IDS else "<f4"), device=dev).fill_(-7)

    for name, t in ordered("s3", S, start_over, consumer).items():
        out["s3_" + name] = host(t)
    ctx3.close()
    delay_ticks = int(out["s1_delay_ms"] * ticks_per_ms)

    # ---- 6: another stream in the middle of a job (mi3pt_set_stream blocks: it waits for the stream it leaves) ----
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    ctx6 = make_ctx()
    ctx6.enable_timing(True)                                                # (mi3pt_raytrace_launch_stats counts timed launches)
    ctx6.write_texture(capi.TEX_ACCUMULATION, ckpt)
    ctx6.raytrace_launch_stats(reset=True)
    ctx6.set_stream(A.cuda_stream)
    frames(ctx6, FIRST, FIRST, 5)                                           # four launched at capacity, one left queued
    behind, end = Event(), Event()
    with torch.cuda.stream(B):
        torch.cuda._sleep(delay_ticks)
        behind.record()
    ctx6.set_stream(B.cuda_stream)                                          # launches the queued frame on A, waits for A -- not for B
    frames(ctx6, FIRST + 5, FIRST + 5, 5)
    ctx6.flush()
    with torch.cuda.stream(B):
        end.record()
    out["s6_nothing_had_run_on_b"] = (not behind.query()) and (not end.query())
    ctx6.set_stream(None)                                                   # waits for B
    out["s6_b_done_after_leaving_it"] = bool(end.query())
    frames(ctx6, FIRST + 10, FIRST + 10, 5)
    out["s6_mean"] = ctx6.read_texture(capi.TEX_ACCUMULATION)
    _, launches, nframes = ctx6.raytrace_launch_stats()
    out["s6_launches"], out["s6_frames"] = int(launches), int(nframes)
    ctx6.close()

    # ---- 7: handle 0, torch's default stream ----
    ctx7 = make_ctx()
    ctx7.set_stream(S.cuda_stream)
    ctx7.set_stream(torch.cuda.default_stream().cuda_stream)                # 0 = NULL: back to the internal stream
    mark = Event()
    with torch.cuda.stream(S):
        torch.cuda._sleep(delay_ticks)
        mark.record()
    ctx7.reset()
    frames(ctx7, 1, 1, COUNT)
    out["s7_mean"] = ctx7.read_texture(capi.TEX_ACCUMULATION)               # blocking: waits for the CONTEXT's stream
    out["s7_read_did_not_wait_for_the_callers_stream"] = not mark.query()
    S.synchronize()
    ctx7.close()

    # ---- 8a: destroy with a caller's stream set ----
    ctx8 = make_ctx()
    D = torch.cuda.Stream()
    ctx8.set_stream(D.cuda_stream)
    end = Event()
    with torch.cuda.stream(D):
        torch.cuda._sleep(delay_ticks)
    frames(ctx8, FIRST, FIRST, COUNT)
    ctx8.flush()
    with torch.cuda.stream(D):
        end.record()
    out["s8_pending_before_destroy"] = not end.query()
    ctx8.close()
    out["s8_done_after_destroy"] = bool(end.query())
    with torch.cuda.stream(D):
        total = torch.arange(1000, device=dev, dtype=torch.int64).sum()
    D.synchronize()
    out["s8_stream_usable"] = int(total.item()) == 499500

    # ---- every job once more on an ordinary context: own stream, blocking read-backs ----
    plain = make_ctx()
    plain.write_texture(capi.TEX_ACCUMULATION, ckpt)
    frames(plain, FIRST, FIRST, COUNT)
    plain.set_uniforms(capi.PASS_FULLSCREEN, _fs_bytes())
    plain.submit(capi.SUBMIT_FULLSCREEN)
    out["plain_s1_mean"] = plain.read_texture(capi.TEX_ACCUMULATION)
    out["plain_s4_canvas8"] = plain.read_canvas_rgba8()
    out["plain_s4_canvas"] = plain.read_texture(capi.TEX_CANVAS)
    frames(plain, FIRST + COUNT, FIRST + COUNT, 5)
    out["plain_s6_mean"] = plain.read_texture(capi.TEX_ACCUMULATION)
    plain.reset()
    frames(plain, 1, 1, COUNT)
    out["plain_s2_mean"] = plain.read_texture(capi.TEX_ACCUMULATION)
    plain.set_pipelining(False)
    for variant in (2, 0):
        plain.set_kernel_variant(variant)
        plain.write_texture(capi.TEX_ACCUMULATION, ckpt)
        frames(plain, FIRST, FIRST, COUNT)
        out[f"plain_s5_v{variant}_mean"] = plain.read_texture(capi.TEX_ACCUMULATION)
    plain.set_kernel_variant(0)
    plain.set_pipelining(True)
    plain.set_moments(True)
    plain.write_texture(capi.TEX_ACCUMULATION, ckpt)
    frames(plain, FIRST, FIRST, COUNT)
    plain.render_aovs(capi.AOV_ALL)
    plain.denoise_guided(LEVELS, *SIGMAS)
    out["plain_s3_accum"] = plain.read_texture(capi.TEX_ACCUMULATION)
    out["plain_s3_moments"] = plain.read_moments()
    out["plain_s3_guided"] = plain.read_guided()
    for k, name in enumerate(NAMES):
        out["plain_s3_" + name] = plain.read_aov(k)
    plain.close()
    return out


def _child(outq):
    try:
        out = _scenarios()
    except BaseException:
        out = {"error": traceback.format_exc()}
    outq.put(out)


@pytest.fixture(scope="module")
def child(built):
    """every scenario, once, in one spawned process"""
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    p = mpc.Process(target=_child, args=(q,))
    p.start()
    res, deadline = None, time.monotonic() + 300
    while res is None:
        try:
            res = q.get(timeout=1.0)
        except queue_mod.Empty:
            if not p.is_alive():                    # (died without an answer: nothing more is started, nobody waits for the limit)
                try:
                    res = q.get(timeout=1.0)
                except queue_mod.Empty:
                    pytest.fail(f"the child ended with exit code {p.exitcode} and returned nothing")
            elif time.monotonic() > deadline:
                p.kill()
                pytest.fail("the child did not answer within 300 s")
    p.join(timeout=120)
    assert p.exitcode == 0, f"the child's exit code: {p.exitcode}"
    assert "error" not in res, res.get("error")
    for k in sorted(res):
        if k.endswith("_ms") or k.startswith("s8_time") or k in ("ticks_per_ms", "wrap_zero_copy", "s6_launches", "s6_frames"):
            print(f"streams: {k} = {res[k]}")
    return res


@pytest.fixture(scope="module")
def want(orc, demo, env):
    """the oracle's side of every scenario, computed once"""
    osc = pc.oracle_scene(orc, demo, env)
    ckpt = _checkpoint()

    def rt(f):
        return pc.rt_uniforms(demo, W, H, frame=f, bounces=BOUNCES).tobytes()

    def acc(f, enabled=1):
        return pc.acc_uniforms(W, H, f, enabled).tobytes()

    steps = [(f, f, 1) for f in range(FIRST, FIRST + COUNT)]
    mean, moments, _, _ = mr.oracle_steps(orc, osc, steps, W, H, rt, acc, mean=ckpt)
    out = {"mean": mean, "moments": moments, "osc": osc, "rt": rt(FIRST)}
    fifteen = mean
    for f in range(FIRST + COUNT, FIRST + COUNT + 5):
        img, _ = orc.raytrace(osc, rt(f), W, H)
        fifteen = orc.accumulate(acc(f), W, H, img, fifteen)
    out["fifteen"] = fifteen
    from_one = np.zeros((H, W, 4), np.float32)
    for f in range(1, 1 + COUNT):
        img, _ = orc.raytrace(osc, rt(f), W, H)
        from_one = orc.accumulate(acc(f), W, H, img, from_one)
    out["from_one"] = from_one
    out["canvas"], out["canvas8"] = orc.fullscreen(_fs_bytes(), mean)
    feat = aov_reference.reference(orc, osc, rt(FIRST), W, H)
    out["features"] = feat
    out["guided"], out["guided_stats"] = gr.guided(orc, mean, feat["normal"], feat["position"], feat["albedo"], feat["ids"], LEVELS, *SIGMAS)
    return out


def _same(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape}"
    assert pc.same_bits(got, ref), f"{what}: " + pc.describe_diff(got, ref)


def _localise(child, ref, *keys):
    """both outcomes in the test's output before anything is asserted: the ordinary context's and the caller's stream's"""
    for k in keys:
        print(f"{k}: {pc.describe_diff(child[k], ref) if child[k].shape == ref.shape else child[k].shape}")


def _ordered(child, name):
    """the condition that keeps a scenario from passing vacuously, and its figures"""
    print(f"{name}: job {child[name + '_job_ms']:.3f} ms, delay {child[name + '_delay_ms']:.1f} ms")
    assert DELAY_MIN_MS <= child[name + "_delay_ms"] <= DELAY_MAX_MS
    assert child[name + "_nothing_had_run"], \
        f"{name}: right after the last enqueue the stream had got past the delay: a call of the chain waited for the stream"


def test_the_checkpoint_is_no_mean_of_the_job(want):
    """what a lost dependency leaves behind differs from what is wanted, texel for texel almost everywhere"""
    ckpt = _checkpoint()
    assert np.isfinite(ckpt).all() and (ckpt[..., 3] == 1).all()
    assert (want["mean"][..., :3] != ckpt[..., :3]).mean() > 0.99
    assert (want["mean"][..., :3] != 0).mean() > 0.99
    # (the filter is no copy: of its 358 836 in-image taps the hit rule rejects some, and weights fall on both sides of 0.5 --
    # 2 % of them are thousands of taps each)
    st = want["guided_stats"]
    assert st["rejected"] >= 0.02 and st["below"] >= 0.02 and st["above"] >= 0.02, st
    assert (want["guided"][..., :3] != want["mean"][..., :3]).mean() > 0.9
    assert (want["moments"][..., 3] == COUNT).all() and (want["moments"][..., :3] > 0).mean() > 0.9


def test_producer_order_into_a_bound_tensor(child, want):
    """1: delay, accum.copy_(checkpoint), ten frames, flush, accum.clone() -- all on the caller's stream, the tensor bound as the
    running mean.  An ordered mean that ran off the stream leaves the bare checkpoint, a clone that ran early the scrubbed image."""
    _localise(child, want["mean"], "plain_s1_mean", "s1_mean")
    _same(child["plain_s1_mean"], want["mean"], "ordinary context")
    _ordered(child, "s1")
    _same(child["s1_mean"], want["mean"], "the clone behind the job")


def test_reset_in_the_chain(child, want):
    """2: delay, reset, ten frames from frame 1, flush, clone: the mark the raytrace streams wait for is recorded behind the delay"""
    _localise(child, want["from_one"], "plain_s2_mean", "s2_mean")
    _same(child["plain_s2_mean"], want["from_one"], "ordinary context")
    _ordered(child, "s2")
    _same(child["s2_mean"], want["from_one"], "the clone behind the job")


def test_consumer_order_through_every_zero_copy_pointer(child, want, orc):
    """3: no bound tensor; the context's images wrapped as torch tensors over their device pointers (__cuda_array_interface__; a
    device-to-device copy on the stream where torch refuses it) and cloned on the stream behind ten frames with moments, the feature
    images and the guided filter."""
    print("wrapped without a copy:", child["wrap_zero_copy"])
    _localise(child, want["mean"], "plain_s3_accum", "s3_accum")
    _localise(child, want["moments"], "plain_s3_moments", "s3_moments")
    _localise(child, want["guided"], "plain_s3_guided", "s3_guided")
    feat, ids_ref = want["features"], want["features"]["ids"]
    for src in ("plain_s3_", "s3_"):
        if src == "s3_":
            _ordered(child, "s3")
        _same(child[src + "accum"], want["mean"], src + "accumulation image")
        _same(child[src + "moments"], want["moments"], src + "moments image")
        got = {name: child[src + name] for name in NAMES}
        assert got["ids"].dtype == np.int32 and ids_ref.dtype == np.int32
        aov_reference.assert_images(pc, got, feat, src + "feature images:")
        _same(child[src + "guided"], want["guided"], src + "filtered image")
    aov_reference.check_ids(orc, want["osc"], want["rt"], child["s3_ids"], feat, H)


def test_presentation_on_the_callers_stream(child, want):
    """4: scenario 1 followed by a fullscreen submit (PRESENT_EXACT, de-noise on, ACES); then blocking reads of the canvas"""
    _localise(child, want["canvas"], "plain_s4_canvas", "s4_canvas")
    _same(child["plain_s4_canvas"], want["canvas"], "ordinary context: canvas")
    assert np.array_equal(child["plain_s4_canvas8"], want["canvas8"]), "ordinary context: RGBA8 canvas"
    _ordered(child, "s4")
    _same(child["s4_mean"], want["mean"], "the clone behind the job")
    _same(child["s4_canvas"], want["canvas"], "canvas")
    assert child["s4_canvas8"].shape == want["canvas8"].shape and np.array_equal(child["s4_canvas8"], want["canvas8"]), "RGBA8 canvas"


@pytest.mark.parametrize("variant", [2, 0])
def test_the_route_without_pipelining(child, want, variant):
    """5: scenario 1 with pipelining off: every frame launched inside mi3pt_submit on the context's stream -- the fused per-pixel
    kernel (variant 2), the state-machine kernel and a mean of its own (auto)"""
    _localise(child, want["mean"], f"plain_s5_v{variant}_mean", f"s5_v{variant}_mean")
    _same(child[f"plain_s5_v{variant}_mean"], want["mean"], "ordinary context")
    _ordered(child, f"s5_v{variant}")
    assert child[f"s5_v{variant}_kind"] == (0 if variant == 2 else 1), "the kernel the last launch ran"
    _same(child[f"s5_v{variant}_mean"], want["mean"], "the clone behind the job")


def test_changing_streams_in_the_middle_of_a_job(child, want):
    """6: five frames on stream A, set_stream(B) with a delay already on B, five frames, set_stream(NULL), five frames; launches of
    4 + 1 each.  mi3pt_set_stream launches what is queued on the stream it leaves and waits for THAT stream; the slot sets' events are
    forgotten twice; the frames sent to B stay behind B's delay."""
    _localise(child, want["fifteen"], "plain_s6_mean", "s6_mean")
    _same(child["plain_s6_mean"], want["fifteen"], "ordinary context")
    assert child["s6_nothing_had_run_on_b"], "set_stream(B) or the frames sent to B waited for B"
    assert child["s6_b_done_after_leaving_it"], "set_stream(NULL) returned before the stream it left had finished"
    assert (child["s6_launches"], child["s6_frames"]) == (6, 15), "a frame was lost or repeated"
    _same(child["s6_mean"], want["fifteen"], "the mean of fifteen frames")


def test_handle_zero_restores_the_internal_stream(child, want):
    """7: torch's default stream is handle 0, and mi3pt_set_stream(ctx, 0) is mi3pt_set_stream(ctx, NULL): the context goes back to
    its own stream.  Pinned without a race: the call succeeds, a job afterwards equals the oracle through a blocking read, and that
    read -- which waits for the context's stream -- returned while the stream the caller had set before was still asleep (were it
    still the context's stream, the read would have waited for it)."""
    assert child["default_stream_handle"] == 0
    _same(child["s7_mean"], want["from_one"], "ten frames after set_stream(0)")
    assert child["s7_read_did_not_wait_for_the_callers_stream"]


def test_life_cycle_on_a_callers_stream(child):
    """8: mi3pt_destroy with a caller's stream set returns after that stream's work and leaves the stream usable; with timing enabled
    the three pass times of a ten-frame presenting job are positive.  (A group refuses mi3pt_set_stream: tests/test_gpu_group.py.)"""
    assert child["s8_pending_before_destroy"], "the job was not behind the delay"
    assert child["s8_done_after_destroy"], "mi3pt_destroy returned before the caller's stream had finished"
    assert child["s8_stream_usable"]
    for name in ("raytrace", "accumulate", "fullscreen"):
        print(f"{name}: {child['s8_time_' + name]:.1f} us")
        assert child["s8_time_" + name] > 0.0
