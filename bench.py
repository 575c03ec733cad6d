"""Benchmark of the MHAHeadDim64 hot path on MI355X (one JSON line on rank 0).

Metric (BASELINE.json): attention-calls/sec & ms/call, 1x4x1024x1024 d=64 fp16; % MFMA peak.

A step is ONE MHAHeadDim64 call — the plugin's enqueue() on a [1,4,1024,64] fp16 Q/K/V
(BASELINE configs[1]) — exactly what the TensorRT engine does per attention node. The K timed
steps are K independent calls captured into one hipGraph (the reference's demo also replays a
CUDA graph, demo/lightglue_trt.cpp:347-366) and replayed once between barriers, inputs resident
in HBM. value = calls/s over all ranks (replicas: each GPU runs its own stream of calls, no
collective on the data path; the only collective is the max-over-ranks of the timer).

A plain run sets up, runs the W warm-up steps, times the K steps and prints the line (metric, value,
unit, ms_per_step, ...). `--dump-outputs DIR` also writes the O of the last timed step as DIR/out.npy
(float32; the inputs are seeded, so two builds can be compared output for output).

`--full` adds everything else the benchmark measures or checks, each in runs of its own after the
headline: the same calls in 2000-step graphs, the cross-rank output digest, the roofline of the
dominant kernel (main attention kernel; duration from HIP events on the launch stream), isolated
single-call latency, the batched-launch throughput (several calls stacked in one launch), the
variants, concurrent streams, the matcher figures and the CPU baseline (the reference's PyTorch
attention restated in oracle/oracle.py, timed on this host's cores on a bounded sample). `--full
--quick` keeps only the first two of those.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd")
for _p in (REPO, PKG_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

METRIC = "attention-calls/sec & ms/call, 1×1024×1024 d=64 fp16; % MFMA peak"
# MI355X peaks (/opt/skills/guides/MI355X_MICROARCH.md, chip-level parameters): dense fp16 MFMA
# ~2.5 PFLOP/s (not the 2:1-sparse figure), HBM3E 8 TB/s.
PEAK_F16_TFLOPS = 2500.0
# Measured ceilings of the head_dim-64 attention instruction mix on MI355X (see roofline.attainable)
ATTAINABLE = {
    "mix_tflops": 1330.0, "mix_frac": 0.532,
    "mix_source": "profiles/r03/mfma_shape_microbench.txt: v_mfma_f32_32x32x16_f16 with the head_dim-64 softmax "
                  "density beside every MFMA (2 v_exp_f32 + 1 pack + 1 v_max3), 2 waves per SIMD, registers only: "
                  "1315-1340 TFLOP/s at the 1.56-1.71 GHz the chip holds for this mix",
    "full_step_tflops": 1010.0, "full_step_frac": 0.404,
    "full_step_source": "profiles/r04/mb_step.txt row h: the streaming kernel's whole 32-row x 64-key step (MFMAs, "
                        "exponentials, packs, row max, LDS fragment reads, LDS-DMA refill, barrier) in isolation, "
                        "two waves per SIMD: 997-1013 TFLOP/s",
}
PEAK_HBM_GBS = 8000.0


def call_flops(b, h, nq, nkv, d=64):
    """Algorithmic FLOPs of one call: QK^T and PV, 2 flops per MAC."""
    return 4 * b * h * nq * nkv * d


def matcher_flops(n0, n1, pairs=1, layers=9, d=256, heads=4):
    """Algorithmic FLOPs of one LightGlue forward as the reference computes it
    (lightglue_pytorch_no_plugin/lightglue.py:88-233, 328-353; 2 flops per MAC; LayerNorm, GELU,
    softmax and rotary not counted): per layer every Linear of the self block (Wqkv d->3d, out_proj
    d->d, FFN 2d->2d and 2d->d) and the cross block (to_qk, to_v, to_out d->d, FFN) on both images'
    M = pairs (n0 + n1) rows, = 38 M d^2, plus the four attention calls 4 H n_q n_kv 64 (self n0^2 +
    n1^2, cross 2 n0 n1); then the head's final_proj and matchability on all rows and the similarity
    2 n0 n1 d. (The fused path folds out_proj / to_out into the FFN's first weight: it does less work
    than this count, which is the reference algorithm's.)"""
    m = pairs * (n0 + n1)
    att = 4 * heads * 64 * pairs * (n0 * n0 + n1 * n1 + 2 * n0 * n1)
    head = 2 * m * d * d + 2 * m * d + 2 * pairs * n0 * n1 * d
    return layers * (38 * m * d * d + att) + head


def matcher_roofline(flops, ms):
    tf = flops / (ms * 1e-3) / 1e12
    return {"gflop_per_forward": round(flops / 1e9, 3), "tflops": round(tf, 2), "frac": round(tf / PEAK_F16_TFLOPS, 4)}


def call_bytes(b, h, nq, nkv, in_bytes=2, out_bytes=2, d=64):
    return b * h * d * (nq * in_bytes + 2 * nkv * in_bytes + nq * out_bytes)


# ----------------------------------------------------------------------------------------
# distributed timing (replicas); testable on CPU with gloo
# ----------------------------------------------------------------------------------------
def dist_env():
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    return ws, rank, local


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_devices():
    """GPU count inside a rank process (which initialises HIP itself right after)."""
    import torch

    return torch.cuda.device_count()


def probe_device_count(python=sys.executable, timeout=600):
    """GPU count for the LAUNCHER, from a throwaway child process, so the parent that spawns the
    ranks never initialises HIP itself (torch's device count falls back to hipGetDeviceCount when
    amdsmi fails). The child sees the same *_VISIBLE_DEVICES environment as the ranks will.
    Returns None when the child gives no answer (the launcher then refuses to start ranks)."""
    import subprocess

    try:
        r = subprocess.run([python, "-c", "import torch; print(torch.cuda.device_count())"],
                           capture_output=True, text=True, timeout=timeout)
        return int(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None
    except (subprocess.SubprocessError, ValueError, IndexError, OSError):
        return None


def launch_replicas(n, argv, count_devices=probe_device_count, python=sys.executable, script=None, poll_s=0.2):
    """`bench.py --gpus N` without a torchrun environment: start N rank processes (RANK,
    LOCAL_RANK, WORLD_SIZE, MASTER_ADDR/PORT set; rank r drives device r) from a parent that has
    not touched the GPU, and return the first non-zero exit status (0 if all passed). All ranks are
    polled together: the first rank to fail ends the others at once (a rank that dies before the
    gloo rendezvous would otherwise leave the rest waiting in it). Fewer than N visible devices, or
    no device count at all, is an error (exit 2), not a silent N=1 run (one pair
    stream per GPU, the reference's pair loop demo/demo_mono.cpp:194-418 replicated)."""
    import subprocess

    share = os.environ.get("BENCH_SHARE_DEVICE") == "1"
    have = count_devices()
    if have is None:
        print(f"bench.py: --gpus {n}: could not count the visible GPUs (device-count probe failed)",
              file=sys.stderr, flush=True)
        return 2
    if have < n and not (share and have >= 1):
        print(f"bench.py: --gpus {n} needs {n} visible GPUs, found {have}", file=sys.stderr, flush=True)
        return 2
    port = str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([python, script or os.path.abspath(__file__)] + list(argv), env=env))
    status = 0
    live = list(procs)
    while live:
        for p in list(live):
            c = p.poll()
            if c is None:
                continue
            live.remove(p)
            if c != 0 and status == 0:
                status = c
                for q in live:  # the first failure ends the job
                    q.terminate()
        if live:
            time.sleep(poll_s)
    for p in procs:
        p.wait()
    return status


def timed_region(run_steps, barrier, sync, reduce_max):
    """barrier + sync, run the K steps, sync + barrier; return max-over-ranks seconds."""
    barrier()
    sync()
    t0 = time.perf_counter()
    run_steps()
    sync()
    dt = time.perf_counter() - t0
    barrier()
    return reduce_max(dt)


def timed_replays(torch, replay, stream, barrier, reduce_max, replays, local=None):
    """The headline's timed region: barrier + synchronize, then `replays` repetitions of the K steps
    (`replay()`: K plugin enqueues, or one replay of a K-step graph) back to back on the launch
    stream with a HIP event pair around each (events on the stream the kernels run on),
    synchronize + barrier. Returns (max over ranks of the median replay time,
    max over ranks of the host wall time per replay), in seconds; `local` (a dict), if given,
    receives this rank's own median under "median_s".

    The event pair times exactly the K steps on the GPU. A sleep kernel queued ahead of the replays
    holds the stream while the host submits them (sized from an untimed rehearsal of the host's
    submission time), so the GPU runs them back to back: the host's submission cost (~10 us per
    enqueue here, twice a call's GPU time; ~0.1 ms per 20-node graph replay) stays out of the events
    instead of starving the GPU between calls. The second value is the host's own submission time
    per repetition (the K steps + two event records), measured around the submission loop alone: the sleep
    kernel's artificial backlog is not in it."""
    starts = [torch.cuda.Event(enable_timing=True) for _ in range(replays)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(replays)]

    def submit():
        t = time.perf_counter()
        with torch.cuda.stream(stream):
            for i in range(replays):
                starts[i].record(stream)
                replay()
                ends[i].record(stream)
        return time.perf_counter() - t

    # untimed rehearsal: host submission time, and the sleep kernel's rate on this device
    host_s = submit()
    torch.cuda.synchronize()
    cycles_per_s = sleep_cycles_per_s(torch, stream)

    barrier()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(cycles_per_s * (1.5 * host_s + 2e-3)))
    host = submit() / replays
    torch.cuda.synchronize()
    barrier()
    med = statistics.median(s.elapsed_time(e) for s, e in zip(starts, ends)) * 1e-3
    if local is not None:
        local["median_s"] = med
    return reduce_max(med), reduce_max(host)


def sleep_cycles_per_s(torch, stream):
    """The sleep kernel's rate on this device (cycles per second), from one 1e7-cycle sleep between events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        torch.cuda._sleep(int(1e7))
        e1.record(stream)
    torch.cuda.synchronize()
    return 1e7 / max(1e-6, e0.elapsed_time(e1) * 1e-3)


def split_steps(steps, chunk=2000):
    """`steps` as chunks of at most `chunk` steps (the last one takes the remainder)."""
    return [chunk] * (steps // chunk) + ([steps % chunk] if steps % chunk else [])


def timed_chunks(torch, run_chunk, chunks, stream, barrier, reduce_max, round_steps=6000, local=None):
    """The timed region for more steps than one backlog holds: the K steps are issued ONCE, as
    `chunks` (split_steps) with a HIP event pair around each chunk (`run_chunk(n)` issues n steps),
    and the chunk times are summed. The chunks go out in rounds of at most `round_steps` steps, each
    round queued behind a sleep kernel sized from an untimed rehearsal of the first chunk, as
    timed_replays does for its replays, so the host's submission stays out of the events; the stream
    is drained between rounds. The cost of the run grows with K alone (no repetitions of the K
    steps). Returns (max over ranks of the summed chunk times, max over ranks of the host's
    submission time), in seconds; `local`, if given, receives this rank's own sum under "median_s"."""
    t = time.perf_counter()
    with torch.cuda.stream(stream):
        run_chunk(chunks[0])
    host_per_step = (time.perf_counter() - t) / chunks[0]
    torch.cuda.synchronize()
    cycles_per_s = sleep_cycles_per_s(torch, stream)

    barrier()
    torch.cuda.synchronize()
    total_ms, host, i = 0.0, 0.0, 0
    while i < len(chunks):
        group = [chunks[i]]
        i += 1
        while i < len(chunks) and sum(group) + chunks[i] <= round_steps:
            group.append(chunks[i])
            i += 1
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in group]
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(cycles_per_s * (1.25 * host_per_step * sum(group) + 2e-3)))
            t = time.perf_counter()
            for (s, e), n in zip(events, group):
                s.record(stream)
                run_chunk(n)
                e.record(stream)
            host += time.perf_counter() - t
        torch.cuda.synchronize()
        total_ms += sum(s.elapsed_time(e) for s, e in events)
    barrier()
    if local is not None:
        local["median_s"] = total_ms * 1e-3
    return reduce_max(total_ms * 1e-3), reduce_max(host)


def claim_stdout(ws):
    """Rank 0's ONE JSON line is the only thing a bench process writes to stdout. With several
    ranks, file descriptor 1 is pointed at stderr (the gloo library prints its connection messages
    to the C-level stdout of every rank) and the returned stream, a private copy of the original
    stdout, carries the line. One rank: sys.stdout, untouched."""
    if ws <= 1:
        return sys.stdout
    sys.stdout.flush()
    out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    return out


def make_collectives(torch, dist, device=None):
    """Barrier and max-reduce over ranks on a CPU (gloo) group: the replicas exchange nothing on
    the data path, so no RCCL communicator is created (north_star: no collectives needed)."""
    if dist is None or not dist.is_initialized():
        return (lambda: None), (lambda x: x)

    def barrier():
        dist.barrier()

    def reduce_max(x):
        t = torch.tensor([x], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    return barrier, reduce_max


def gather(dist, obj):
    """Every rank's `obj`, in rank order (a list of one when single-process)."""
    if dist is None or not dist.is_initialized():
        return [obj]
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, obj)
    return out


def cpu_share():
    """CPUs this process may use: the affinity mask, capped by a cgroup v2 CPU quota and by
    OMP_NUM_THREADS when the environment sets it (a gpurun box reports the whole host's CPUs in
    os.cpu_count() and in the affinity mask but grants this job a share of them, stated there as
    OMP_NUM_THREADS=16). Returns (threads to use, affinity count, cgroup quota or None)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, period = f.read().split()[:2]
        if q != "max":
            quota = max(1, int(int(q) // int(period)))
    except (OSError, ValueError):
        pass
    use = min(n, quota) if quota else n
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:  # the box's stated CPU share for this job
        use = min(use, int(omp))
    return use, n, quota


# ----------------------------------------------------------------------------------------
# GPU measurement helpers
# ----------------------------------------------------------------------------------------
def event_durations_ms(torch, launch, n, stream):
    """Per-launch GPU durations from HIP events recorded on the launch stream.

    A long sleep kernel is queued first so that every (event, launch, event) triple is
    already enqueued when the GPU reaches it: the events then time the kernel(s), not
    the host's launch latency."""
    starts = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(40e6))
        for i in range(n):
            starts[i].record(stream)
            launch()
            ends[i].record(stream)
    stream.synchronize()
    return [s.elapsed_time(e) for s, e in zip(starts, ends)]


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def graphs_interleaved_ms(torch, launches, stream, k=50, rounds=7):
    """Per-launch times of several forms of the same work: each captured as a graph of `k`
    back-to-back launches, then replayed round-robin (A, B, A, B, ...) `rounds` times; medians."""
    graphs = []
    for launch in launches:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            launch()
        stream.synchronize()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(k):
                launch()
        g.replay()
        stream.synchronize()
        graphs.append(g)
    times = [[] for _ in graphs]
    for _ in range(rounds):
        for i, g in enumerate(graphs):
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record(stream)
            with torch.cuda.stream(stream):
                g.replay()
            e_.record(stream)
            stream.synchronize()
            times[i].append(s_.elapsed_time(e_) / k)
    return tuple(statistics.median(t) for t in times)


def graph_per_launch_ms(torch, launch, stream, k=200, reps=5):
    """Per-launch time of `k` back-to-back launches captured in one graph (median of `reps` replays)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        launch()
    stream.synchronize()
    with torch.cuda.graph(g, stream=stream):
        for _ in range(k):
            launch()
    g.replay()
    stream.synchronize()
    out = []
    for _ in range(reps):
        s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_.record(stream)
        with torch.cuda.stream(stream):
            g.replay()
        e_.record(stream)
        stream.synchronize()
        out.append(s_.elapsed_time(e_) / k)
    return statistics.median(out)


def cpu_baseline(seconds=10.0, nq=1024, nkv=1024):
    """Reference PyTorch CPU attention (lightglue_pytorch_no_plugin/lightglue.py:82-84, restated
    in oracle/oracle.py) on this host, fp32, bounded sample of ~`seconds` at the metric shape
    with every CPU this process is granted (cpu_share(): affinity mask capped by the cgroup quota;
    SURVEY §8(d) asks for os.cpu_count(), which on a shared GPU box counts the whole host); plus
    the SURVEY §8(d) grid (1 thread / all granted threads x 256^2 / 1024^2, 20 warm-ups then the
    median of >= 50 calls)."""
    import torch

    from lightglue_amd import synth
    from oracle import oracle

    threads, affinity, quota = cpu_share()
    torch.set_num_threads(threads)

    def median_ms(n_q, n_kv, nthreads, min_calls, budget_s):
        torch.set_num_threads(nthreads)
        qn, kn, vn = synth.qkv(2, n_q, n_kv)
        q, k, v = (torch.from_numpy(x) for x in (qn, kn, vn))
        for _ in range(20):
            oracle.attention_torch(q, k, v)
        times = []
        t0 = time.perf_counter()
        while len(times) < min_calls or time.perf_counter() - t0 < budget_s:
            t1 = time.perf_counter()
            oracle.attention_torch(q, k, v)
            times.append(time.perf_counter() - t1)
            if len(times) >= min_calls and time.perf_counter() - t0 > 4 * budget_s:
                break
        return statistics.median(times) * 1e3, len(times)

    med, n = median_ms(nq, nkv, threads, 50, seconds)
    grid = {}
    for (a_, b_) in ((256, 256), (nq, nkv)):
        for t in (1, threads):
            ms, cnt = median_ms(a_, b_, t, 50, 0.5)
            grid[f"{a_}x{b_}_{t}T_ms"] = round(ms, 4)
    torch.set_num_threads(threads)
    return {"value": round(1e3 / med, 2), "unit": "calls/s", "cores": threads, "kind": "port",
            "ms_per_call": round(med, 3),
            "sample": f"{n} calls of 1x4x{nq}x{nkv} d=64 fp32, torch CPU matmul-softmax-matmul "
                      f"(reference Attention.forward math), median per call, {threads} threads, ~{seconds:.0f}s",
            "grid": grid, "cpu_model": _cpu_model(), "host_logical_cpus": os.cpu_count(),
            "affinity_cpus": affinity, "cgroup_cpu_quota": quota,
            "threads_note": (f"{threads} threads = the CPUs granted to this process (affinity {affinity}, "
                             f"cgroup quota {quota}, OMP_NUM_THREADS {os.environ.get('OMP_NUM_THREADS')}); "
                             f"os.cpu_count() = {os.cpu_count()} counts the whole host, which other jobs share"),
            "single_thread_ms_per_call": grid.get(f"{nq}x{nkv}_1T_ms")}


def load_traffic(tag):
    """HBM bytes per launch of the main kernel from the committed rocprofv3 PMC pass (or None)."""
    path = os.path.join(REPO, "profiles", "traffic.json")
    if not os.path.exists(path):
        return None
    try:
        with open(path) as f:
            d = json.load(f)
        return d.get(tag)
    except Exception:
        return None


def variants(torch, lightglue_amd, device, stream, q, k, v, raw, flops):
    """BASELINE configs[2] and the plugin's Float boundary at the metric shape: fp16 in -> fp32 out
    (the reference's fp16in_fp32out kernel) and fp32 Q/K/V -> fp32 O (a TensorRT fp32 engine's
    call: one launch, the inputs rounded to fp16 inside the 16-row kernel). Per-call time from a
    graph of 200 back-to-back calls, and the max-abs error against a PyTorch fp32 attention on the
    GPU (lightglue_pytorch_no_plugin/lightglue.py:82-84; north_star tolerance 1e-2) of the inputs
    each path receives: the fp16 Q/K/V for fp16in_fp32out, and for the Float boundary the RAW fp32
    Q/K/V (`raw`, not fp16-representable), so its in-kernel RNE rounding is part of the error."""
    qf, kf, vf = (t.float() for t in (q, k, v))
    ref16 = torch.softmax((qf @ kf.transpose(-1, -2)) * 0.125, -1) @ vf
    qr, kr, vr = (torch.from_numpy(x).to(device).contiguous() for x in raw)
    ref32 = torch.softmax((qr @ kr.transpose(-1, -2)) * 0.125, -1) @ vr
    o32 = torch.empty(q.shape, dtype=torch.float32, device=device)
    of = torch.empty_like(qr)
    res = {}
    for name, fn, o, ref in (("fp16in_fp32out", lambda: lightglue_amd.mha_hd64_batched(
                                  q, k, v, out_dtype=torch.float32, out=o32), o32, ref16),
                             ("float_boundary", lambda: lightglue_amd.mha_hd64(qr, kr, vr, out=of), of, ref32)):
        o.fill_(float("nan"))
        with torch.cuda.stream(stream):
            fn()
        stream.synchronize()
        err = float((o - ref).abs().max())
        t = graph_per_launch_ms(torch, fn, stream)
        res[name] = {"us_per_call": round(t * 1e3, 3), "calls_per_s": round(1e3 / t, 1),
                     "tflops": round(flops / (t * 1e-3) / 1e12, 2), "max_abs_vs_torch_fp32": err}
    return res


def concurrent_streams(torch, lightglue_amd, device, nq, nkv, rank, flops, per_stream=500):
    """Independent calls of the metric shape issued on S streams at once (S image pairs in flight,
    each stream its own Q/K/V/O and its own graph of `per_stream` dependent enqueues): whole-GPU
    calls/s. Without a hint a call fills all 256 CUs (16-row blocks), so streams barely overlap;
    with the concurrency hint set to S (mha_hd64_set_concurrency_hint) the planner gives each call
    32-row blocks on half the CUs (S = 2) or in the two-per-CU form (S >= 3)."""
    from lightglue_amd import synth

    out = {}
    for S in (2, 4):
        for hinted in (False, True):
            prev = lightglue_amd.set_concurrency_hint(S if hinted else 1)
            streams = [torch.cuda.Stream(device) for _ in range(S)]
            graphs = []
            for i, st in enumerate(streams):
                qn, kn, vn = synth.qkv(500 + 17 * rank + i, nq, nkv)
                q, k, v = (torch.from_numpy(x).to(device).half().contiguous() for x in (qn, kn, vn))
                o = torch.empty_like(q)
                with torch.cuda.stream(st):
                    lightglue_amd.mha_hd64(q, k, v, out=o)  # per-stream workspace, outside capture
                    torch.cuda.synchronize(device)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=st):
                        for _ in range(per_stream):
                            lightglue_amd.mha_hd64(q, k, v, out=o)
                graphs.append((g, st, (q, k, v, o)))
            lightglue_amd.set_concurrency_hint(prev)
            for g, st, _ in graphs:  # warm
                with torch.cuda.stream(st):
                    g.replay()
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for g, st, _ in graphs:
                with torch.cuda.stream(st):
                    g.replay()
            torch.cuda.synchronize(device)
            dt = time.perf_counter() - t0
            calls = S * per_stream
            out[f"{S}" + ("_hinted" if hinted else "")] = {
                "calls_per_s": round(calls / dt, 1), "us_per_call": round(dt * 1e6 / calls, 3),
                "tflops": round(calls * flops / dt / 1e12, 2)}
    return out


def overlapped_batched(torch, lightglue_amd, device, nq, nkv, rank, flops, B=16, S=2, launches=20):
    """S streams, each replaying a graph of `launches` back-to-back B-call batched launches, all at
    once: whole-GPU calls/s (best of 3 replays, host clock around all streams)."""
    from lightglue_amd import synth

    graphs = []
    for i in range(S):
        st = torch.cuda.Stream(device)
        q, k, v = (torch.from_numpy(x).to(device).half().contiguous() for x in synth.qkv(700 + 13 * rank + i, nq, nkv,
                                                                                             batch=B))
        o = torch.empty_like(q)
        with torch.cuda.stream(st):
            lightglue_amd.mha_hd64_batched(q, k, v, out=o)
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                for _ in range(launches):
                    lightglue_amd.mha_hd64_batched(q, k, v, out=o)
        graphs.append((g, st, (q, k, v, o)))
    best = None
    for rep in range(4):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for g, st, _ in graphs:
            with torch.cuda.stream(st):
                g.replay()
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
        if rep:  # the first replay warms
            best = dt if best is None else min(best, dt)
    calls = S * launches * B
    return {"streams": S, "calls_per_launch": B, "calls_per_s_per_gpu": round(calls / best, 1),
            "tflops": round(calls * flops / best / 1e12, 2), "frac": round(calls * flops / best / 1e12 / PEAK_F16_TFLOPS, 4)}


def cold_inputs(torch, lightglue_amd, stream, q, k, v, barrier, reduce_max, ws, pool_mib=640):
    """The headline's calls again, each on its own copy of Q/K/V from a pool larger than every cache.

    The headline re-reads one Q/K/V, and an XCD's L2 keeps a launch's lines for the next launch on
    the stream (tools/mb_l2_retention.hip: a dependent load costs 220 cycles in the next launch,
    740 after a 256 MiB scrub; profiles/r02/l2_retention.txt). Here consecutive calls read
    different buffers and a buffer comes round again only after pool_mib MiB (> the 256 MiB MALL +
    8 x 4 MiB L2), so every call fetches its inputs from HBM: what a producer that streams fresh
    pairs through the plugin sees when its Q/K/V are no longer in any cache."""
    per_set = 3 * q.numel() * q.element_size()
    sets = max(2, -(-(pool_mib << 20) // per_set))
    pool = [(q.clone(), k.clone(), v.clone(), torch.empty_like(q)) for _ in range(sets)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        for (a, b, c, o) in pool:
            lightglue_amd.mha_hd64(a, b, c, out=o)
    graph.replay()
    stream.synchronize()
    ok = all(torch.equal(o, pool[0][3]) for (_, _, _, o) in pool[1:])
    elapsed, _ = timed_replays(torch, graph.replay, stream, barrier, reduce_max, 5)
    del graph, pool
    return {"calls_per_graph": sets, "pool_mib": round(sets * per_set / 2**20, 1),
            "calls_per_s": round(sets * ws / elapsed, 1), "us_per_call": round(elapsed / sets * 1e6, 3),
            "outputs_identical_to_each_other": ok,
            "how": ("each call on its own copy of the headline's Q/K/V (pool larger than MALL + L2), one graph of "
                    "all calls, median of 5 replays") if pool_mib > 300 else
                   ("each call on its own copy of the headline's Q/K/V from a pool larger than the eight 4 MiB L2s "
                    "but inside the 256 MiB MALL (Infinity Cache): inputs from the MALL, as in the matcher, whose "
                    "Q/K/V are the projection kernel's fresh outputs; one graph of all calls, median of 5 replays")}


def sweep(torch, lib, device, stream, nq, nkv):
    """Main-kernel (+combine) time for every compiled workgroup shape and KV split, single call and
    batched; one JSON object per line on stderr (tuning aid for plan_call)."""
    from lightglue_amd import synth

    ws_buf = torch.empty(256 << 20, dtype=torch.uint8, device=device)
    for batch in [int(b) for b in os.environ.get("SWEEP_BATCHES", "1,2,8").split(",")]:
        qn, kn, vn = synth.qkv(7, nq, nkv, batch=batch)
        q, k, v = (torch.from_numpy(x).to(device).half().contiguous() for x in (qn, kn, vn))
        o = torch.empty_like(q)
        for qw, kw in ((0, 0), (4, 1), (2, 2), (1, 2), (4, 2), (2, 4), (1, 8), (21, 0), (22, 0)):
            for splits in ((0,) if qw >= 21 or qw == 0 or kw >= 4 else (1, 2, 4, 8, 16)):
                def run(mask=3):
                    return lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), batch,
                                                      4, nq, nkv, 0, 0, qw, kw, splits, ws_buf.data_ptr(),
                                                      ws_buf.numel(), stream.cuda_stream, mask)
                if run() != 0:
                    continue
                t_all = statistics.median(event_durations_ms(torch, run, 60, stream)[10:])
                t_main = statistics.median(event_durations_ms(torch, lambda: run(1), 60, stream)[10:])
                fl = call_flops(batch, 4, nq, nkv)
                print(json.dumps({"sweep": 1, "batch": batch, "q_waves": qw, "kv_waves": kw, "splits": splits,
                                  "main_us": round(t_main * 1e3, 2), "total_us": round(t_all * 1e3, 2),
                                  "main_tflops": round(fl / (t_main * 1e-3) / 1e12, 1)}), file=sys.stderr,
                      flush=True)


def matcher_attention(torch, device, stream, rank, sizes=(512, 1024, 2048), layers=9, reps=20, separate=False):
    """BASELINE configs[3] (attention share): the 36 MHAHeadDim64 calls of a 9-layer LightGlue
    matcher (per layer self0, self1, cross0->1, cross1->0; lightglue.py:216-226) at N0 = N1 = N,
    captured in one graph, as 36 plugin enqueues vs 18 grouped launches (self pair + cross pair)."""
    import lightglue_amd
    from lightglue_amd import synth

    res = {}
    for n in sizes:
        d = []
        for i in range(4):
            qn, kn, vn = synth.qkv(500 + 10 * rank + i + n, n, n)
            d.append(tuple(torch.from_numpy(x).to(device).half().contiguous() for x in (qn, kn, vn)))
        (q0, k0, v0), (q1, k1, v1) = d[0], d[1]
        outs = [torch.empty_like(q0) for _ in range(4)]
        calls = [(q0, k0, v0), (q1, k1, v1), (q0, k1, v1), (q1, k0, v0)]

        def separate_calls():
            for _ in range(layers):
                for c, o in zip(calls, outs):
                    lightglue_amd.mha_hd64(*c, out=o)

        def grouped():
            for _ in range(layers):
                lightglue_amd.mha_hd64_grouped(calls[:2], outs=outs[:2])
                lightglue_amd.mha_hd64_grouped(calls[2:], outs=outs[2:])

        times = {}
        modes = (("separate", separate_calls), ("grouped", grouped)) if separate else (("grouped", grouped),)
        for name, fn in modes:
            with torch.cuda.stream(stream):
                fn()
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                fn()
            g.replay()
            stream.synchronize()
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record(stream)
            with torch.cuda.stream(stream):
                for _ in range(reps):
                    g.replay()
            e_.record(stream)
            stream.synchronize()
            times[name] = s_.elapsed_time(e_) / reps  # ms per matcher pass (36 calls)
        fl = 4 * layers * call_flops(1, 4, n, n)
        res[str(n)] = {"calls": 4 * layers, "launches": 2 * layers,
                       "grouped_ms": round(times["grouped"], 4),
                       "grouped_tflops": round(fl / (times["grouped"] * 1e-3) / 1e12, 1),
                       "grouped_frac": round(fl / (times["grouped"] * 1e-3) / 1e12 / PEAK_F16_TFLOPS, 4)}
        if "separate" in times:
            res[str(n)]["separate_ms"] = round(times["separate"], 4)
    return res


def graph_ms(torch, g, st, reps=10, rounds=5, warm_ms=60.0):
    """ms per replay of a captured graph in steady state: replays for >= warm_ms first (the replays right
    after a capture, with the GPU idle during the host's capture work, ran ~12 % slow: bench's single
    10-replay sample read 2.38 ms for a P = 16 forward that runs 2.13 ms steady on the same box,
    profiles/r06/bench_pairs_probe.jsonl), then the median of `rounds` rounds of `reps` back-to-back
    replays between HIP events on the graph's stream."""
    import statistics

    t0 = time.perf_counter()
    n = 0
    while True:
        with torch.cuda.stream(st):
            g.replay()
        st.synchronize()
        n += 1
        if (time.perf_counter() - t0) * 1e3 >= warm_ms and n >= 3:
            break
    out = []
    for _ in range(rounds):
        s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s_.record(st)
        with torch.cuda.stream(st):
            for _ in range(reps):
                g.replay()
        e_.record(st)
        st.synchronize()
        out.append(s_.elapsed_time(e_) / reps)
    return statistics.median(out)


def matcher_e2e(torch, device, stream, rank, sizes=(512, 1024, 2048), reps=10, dtype=None):
    """BASELINE configs[3]: end-to-end LightGlue matcher latency (9 layers + final assignment,
    seeded synthetic weights, N0 = N1 = N keypoints), one forward captured in a graph. fp16 (default):
    every kernel ours; fp32 (the reference's fp32-engine mode, lightglue_attention_plugin.cpp:222-267):
    attention through the Float boundary, projections on the framework's fp32 GEMMs."""
    from lightglue_amd import matcher

    dtype = dtype or torch.float16
    model = matcher.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(matcher.seeded_state_dict(7, 9), strict=True)
    model = model.to(device, dtype)
    res = {}
    for n in sizes:
        k0, k1, d0, d1 = (t.to(device, dtype) for t in matcher.synthetic_pair(40 + rank, n, n))
        with torch.no_grad():
            with torch.cuda.stream(stream):
                for _ in range(2):
                    model(k0, k1, d0, d1)          # warm: workspace + allocator outside the capture
            stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                out = model(k0, k1, d0, d1)
        ms = graph_ms(torch, g, stream, reps)
        assert torch.isfinite(out[2]).all()
        res[str(n)] = {"ms": round(ms, 4), "pairs_per_s": round(1e3 / ms, 1), **matcher_roofline(matcher_flops(n, n), ms)}
    return res


def matcher_batched_pairs(torch, device, stream, rank, n=1024, pairs=(1, 4, 8, 16, 32), reps=10, streams=2):
    """BASELINE configs[4] on one GPU: P image pairs stacked in the batch dimension of ONE forward
    (every projection and glue kernel runs once on all P pairs' rows; each layer's self and cross
    attention is one grouped launch of P-batch calls), fp16, N0 = N1 = n; one captured forward
    replayed back to back. Also `streams` such graphs of P pairs each replayed on that many streams
    at once. pairs/s of the whole GPU."""
    from lightglue_amd import matcher

    model = matcher.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(matcher.seeded_state_dict(7, 9), strict=True)
    model = model.to(device, torch.float16)
    res = {}
    for P in pairs:
        graphs = []
        for si in range(streams):
            st = stream if si == 0 else torch.cuda.Stream(device)
            ps = [matcher.synthetic_pair(80 + 31 * rank + 7 * si + i, n, n) for i in range(P)]
            batch = tuple(torch.cat([p[j] for p in ps], 0).to(device, torch.float16) for j in range(4))
            with torch.no_grad():
                with torch.cuda.stream(st):
                    for _ in range(2):
                        model(*batch)  # warm: workspace + allocator outside the capture
                st.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=st):
                    out = model(*batch)
            graphs.append((g, st, batch, out))
        # one stream: events around `reps` back-to-back replays, in steady state (graph_ms)
        g0, st0 = graphs[0][0], graphs[0][1]
        ms = graph_ms(torch, g0, st0, reps)
        row = {"ms_per_forward": round(ms, 4), "pairs_per_s": round(P * 1e3 / ms, 1), **matcher_roofline(matcher_flops(n, n, P), ms)}
        # `streams` graphs of P pairs at once (host clock, best of reps rounds)
        best = None
        for rep in range(reps + 1):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for g, st, _, _ in graphs:
                with torch.cuda.stream(st):
                    g.replay()
            torch.cuda.synchronize(device)
            dt = time.perf_counter() - t0
            if rep:
                best = dt if best is None else min(best, dt)
        row[f"pairs_per_s_{streams}_streams"] = round(streams * P / best, 1)
        assert all(bool(torch.isfinite(o[2]).all()) for _, _, _, o in graphs)
        res[str(P)] = row
        del graphs
    return res


def matcher_pair_streams(torch, lightglue_amd, device, rank, n=1024, streams=(1, 2, 4, 8), reps=10):
    """BASELINE configs[4] on one GPU: a stream of independent image pairs through the end-to-end
    fp16 matcher, S pairs in flight (S streams, each replaying its own captured forward; the
    concurrency hint set to S while capturing, so each attention call leaves room for the other
    streams). Whole-GPU pairs/s (host clock around all streams, best of `reps` rounds)."""
    from lightglue_amd import matcher

    model = matcher.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(matcher.seeded_state_dict(7, 9), strict=True)
    model = model.to(device, torch.float16)
    res = {}
    for S in streams:
        prev = lightglue_amd.set_concurrency_hint(S)
        try:
            graphs = []
            for i in range(S):
                st = torch.cuda.Stream(device)
                pair = tuple(t.to(device, torch.float16) for t in matcher.synthetic_pair(60 + 7 * rank + i, n, n))
                with torch.no_grad():
                    with torch.cuda.stream(st):
                        for _ in range(2):
                            model(*pair)  # warm: this stream's workspace + allocator outside the capture
                    st.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=st):
                        out = model(*pair)
                graphs.append((g, st, pair, out))
        finally:
            lightglue_amd.set_concurrency_hint(prev)
        best = None
        for rep in range(reps + 1):
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            for g, st, _, _ in graphs:
                with torch.cuda.stream(st):
                    g.replay()
            torch.cuda.synchronize(device)
            dt = time.perf_counter() - t0
            if rep:
                best = dt if best is None else min(best, dt)
        assert all(bool(torch.isfinite(o[2]).all()) for _, _, _, o in graphs)
        res[str(S)] = {"pairs_per_s": round(S / best, 1), "ms_per_round": round(best * 1e3, 4)}
        del graphs
    return res


def profile_driver(torch, args, device):
    """Eager launches of one workload (for rocprofv3 --kernel-trace / --pmc passes)."""
    import lightglue_amd
    from lightglue_amd import synth

    B = 1 if args.only == "call" else args.batched
    qn, kn, vn = synth.qkv(11, args.nq, args.nkv, batch=B)
    q, k, v = (torch.from_numpy(x).to(device).half().contiguous() for x in (qn, kn, vn))
    o = torch.empty_like(q)
    fn = (lambda: lightglue_amd.mha_hd64(q, k, v, out=o)) if B == 1 else (
        lambda: lightglue_amd.mha_hd64_batched(q, k, v, out=o))
    for _ in range(args.warmup + args.steps):
        fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--nkv", type=int, default=1024)
    ap.add_argument("--batched", type=int, default=8, help="calls stacked per launch for the batched figure")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--matcher-separate", action="store_true",
                    help="also time the 36 matcher calls as separate enqueues (adds other sizes of the headline "
                         "kernel to a profile of this command)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run every other measurement and check (2000-step graphs, "
                         "cross-rank digest, roofline, batched, variants, streams, matcher, CPU baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the O of the last timed step as DIR/out.npy (float32; ranks > 0: out_rank<r>.npy)")
    ap.add_argument("--quick", action="store_true",
                    help="with --full: skip the secondary measurements (keep the 2000-step graphs and the digest)")
    ap.add_argument("--sweep", action="store_true", help="time every workgroup shape x KV split (stderr table)")
    ap.add_argument("--only", choices=["call", "batched"], default=None,
                    help="profiling driver: launch just this workload --steps times (eager), print nothing else")
    ap.add_argument("--replays", type=int, default=0,
                    help="replays of the K steps in the timed region (median taken; 0: enough for ~20k calls)")
    ap.add_argument("--launch", choices=["enqueue", "graph"], default="enqueue",
                    help="how the K timed steps are issued: K plugin enqueues straight onto the stream, or one "
                         "replay of a graph captured from those K enqueues")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # one process per GPU, started before anything touches the GPU (no exec from this process)
        sys.exit(launch_replicas(args.gpus, sys.argv[1:]))

    import torch

    ws, rank, local = dist_env()
    if ws != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={ws}", file=sys.stderr, flush=True)
        sys.exit(2)
    # BENCH_SHARE_DEVICE=1 (rehearsal only): ranks share the visible GPUs round-robin, so the N>1
    # path (gloo group, gathers, per-rank lines) can run on a one-GPU box; a real run never sets it
    share = os.environ.get("BENCH_SHARE_DEVICE") == "1"
    if visible_devices() <= local and not share:
        print(f"bench.py: rank {rank} needs GPU {local}, {visible_devices()} visible", file=sys.stderr, flush=True)
        sys.exit(2)
    result_out = claim_stdout(ws)
    dist = None
    device = torch.device("cuda", local % max(1, visible_devices()) if share else local)
    torch.cuda.set_device(device)
    if ws > 1:
        import torch.distributed as dist

        import datetime

        # CPU barrier / timer reduce only; no RCCL on the data path. A bounded timeout: a rank that
        # is gone fails the others' collectives within minutes instead of gloo's default 30.
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=600))
    barrier, reduce_max = make_collectives(torch, dist)

    import lightglue_amd
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    nq, nkv = args.nq, args.nkv
    if args.only:
        profile_driver(torch, args, device)
        return
    qn, kn, vn = synth.qkv(100 + rank, nq, nkv)
    q, k, v = (torch.from_numpy(x).to(device).half().contiguous() for x in (qn, kn, vn))
    out = torch.empty_like(q)

    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        for _ in range(args.warmup):                 # W untimed warmup steps
            lightglue_amd.mha_hd64(q, k, v, out=out)
    stream.synchronize()

    with torch.cuda.stream(stream):                  # the plugin's enqueue with its bindings prepared once
        enqueue = lightglue_amd.plugin.bound_enqueue(q, k, v, out)

    def enqueue_steps():                             # the K timed steps: K independent plugin enqueues
        for _ in range(args.steps):
            enqueue()

    def graph_of(n):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(n):
                enqueue()
        g.replay()                                   # upload / first-replay cost outside the timer
        stream.synchronize()
        return g

    mine, chunks = {}, None
    if args.replays == 0 and args.steps > 5000:
        # more steps than one backlog holds: the K steps issued once, in chunks (timed_chunks)
        chunks, replays = split_steps(args.steps), 1
        if args.launch == "graph":
            graphs = {n: graph_of(n) for n in set(chunks)}
            run_chunk = lambda n: graphs[n].replay()
        else:
            def run_chunk(n):
                for _ in range(n):
                    enqueue()
        elapsed, wall = timed_chunks(torch, run_chunk, chunks, stream, barrier, reduce_max, local=mine)
    else:
        # ... K enqueues, or one replay of a graph captured from them
        run_steps = graph_of(args.steps).replay if args.launch == "graph" else enqueue_steps
        replays = args.replays if args.replays > 0 else max(10, min(250, -(-5000 // args.steps)))
        elapsed, wall = timed_replays(torch, run_steps, stream, barrier, reduce_max, replays, local=mine)
    if args.dump_outputs:
        # the timed path's result: O as its last timed step left it (before any --full measurement
        # writes to the same buffer)
        import numpy as np

        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "out.npy" if rank == 0 else f"out_rank{rank}.npy"),
                out.float().cpu().numpy())
    total_calls = args.steps * ws
    value = total_calls / elapsed
    ms_per_step = elapsed * 1e3 / args.steps
    rank_values = gather(dist, round(args.steps / mine["median_s"], 1))  # each rank's own rate
    # Each timed repetition pays ~4.8 us for its event pair on the GPU, and a K-step graph replay a
    # further ~6-9 us of graph launch (tools/timing_probe.py, profiles/r02/timing_probe.txt): at the
    # driver's K = 20 the enqueue form runs 5.0 us per call, the graph form 5.35
    # (profiles/r06/headline_launch_ab.txt). The same calls in 2000-step graphs, for comparison:
    long_rate = None
    if args.full and args.steps < 2000:
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=stream):
            for _ in range(2000):
                lightglue_amd.mha_hd64(q, k, v, out=out)
        g2.replay()
        stream.synchronize()
        t_long, _ = timed_replays(torch, g2.replay, stream, barrier, reduce_max, 5)
        long_rate = round(2000 * ws / t_long, 1)
        del g2

    # Bit-identity across devices: every rank runs the same seeded pair-call and hashes its output.
    digests = None
    if args.full:
        import hashlib

        cq, ck, cv = (torch.from_numpy(x).to(device).half().contiguous() for x in synth.qkv(4242, nq, nkv))
        co = torch.empty_like(cq)
        with torch.cuda.stream(stream):
            lightglue_amd.mha_hd64(cq, ck, cv, out=co)
        stream.synchronize()
        digests = gather(dist, hashlib.sha256(co.cpu().numpy().tobytes()).hexdigest()[:16])

    import ctypes

    plan_c = (ctypes.c_int32 * 4)()
    ws_need = lib.mha_hd64_plan(1, 4, nq, nkv, 5242880, plan_c)
    q_waves, kv_waves, splits, _ = list(plan_c)
    flops = call_flops(1, 4, nq, nkv)
    result = {
        "metric": METRIC,
        "value": round(value, 1),
        "unit": "calls/s",
        "n_gpus": ws,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 5),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp16",
        "data": "synthetic",
        # an image pair is 36 such calls (9 layers x 2 self + 2 cross), so the
        # attention-only pair rate of the whole job is value / 36 (matcher_e2e_fp16 times whole pairs)
        "attention_pairs_per_s": round(value / 36, 1),
        "timing": {"replays": replays, "launch": args.launch,
                   "per_replay": "HIP events on the launch stream around the K steps (K enqueues or one K-step "
                                 "graph replay); median over replays, max over ranks; replays "
                                 "queued behind a sleep kernel so host submission does not gap "
                                 "the GPU" if chunks is None else
                                 f"the K steps issued once as {len(chunks)} chunks of <= {max(chunks)} steps, HIP events "
                                 "on the launch stream around each chunk, chunk times summed, max over ranks; "
                                 "each round of chunks queued behind a sleep kernel so host submission does not "
                                 "gap the GPU",
                   "host_submit_ms_per_replay": round(wall * 1e3, 4),
                   "calls_per_s_in_2000_step_graphs": long_rate},
        "per_rank_calls_per_s": rank_values,
        "outputs_bitwise_identical_across_ranks": None if digests is None else len(set(digests)) == 1,
        "config": {"workload": "MHAHeadDim64 plugin enqueue, Q/K/V [1,4,1024,64] fp16 -> O fp16 "
                               "(BASELINE configs[1]); K independent plugin enqueues per timed repetition",
                   "batch": 1, "heads": 4, "nq": nq, "nkv": nkv, "head_dim": 64,
                   "parallelism": f"replicas{ws}", "pairs": "one pair stream per GPU, no collective",
                   "plan": {"q_waves": q_waves, "kv_waves": kv_waves, "kv_splits": splits}},
    }

    if args.full and not args.quick:
        ws_buf = torch.empty(max(ws_need, 16), dtype=torch.uint8, device=device)

        def forced(mask):
            lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, 4, nq, nkv, 0,
                                       0, q_waves, kv_waves, splits, ws_buf.data_ptr(), ws_buf.numel(),
                                       torch.cuda.current_stream(device).cuda_stream, mask)

        def full_call():
            with torch.cuda.stream(stream):
                lightglue_amd.mha_hd64(q, k, v, out=out)

        # Kernel durations as the headline runs them: K back-to-back launches replayed from a graph on
        # the launch stream, HIP events around the replay (per launch = total / K; this is the
        # dispatch-to-dispatch interval, an upper bound on the kernel's own duration). The production
        # form is ONE launch (split partials merged by each query group's last-arriving workgroup);
        # the two-kernel form (main + combine kernel) is timed beside it.
        # the single-pass kernels: 22 = 16-row blocks (csrc/mha_hd64_direct16.hip), 21 = 32-row
        # blocks (csrc/mha_hd64_direct.hip)
        direct = q_waves in (21, 22)
        t_main = graph_per_launch_ms(torch, lambda: forced(3), stream)

        def direct32(mask):
            lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, 4, nq, nkv, 0,
                                       0, 21, 0, 0, ws_buf.data_ptr(), ws_buf.numel(),
                                       torch.cuda.current_stream(device).cuda_stream, mask)

        t_direct32 = graph_per_launch_ms(torch, lambda: direct32(3), stream) if q_waves == 22 else None

        # The ring kernel's split plan for the same call, timed beside the production kernel: (1,8)
        # with the 2-way split merged in-launch, and its two-kernel form (main + combine kernel).
        def ring(mask):
            lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 1, 4, nq, nkv, 0,
                                       0, 1, 8, 0, ws_buf2.data_ptr(), ws_buf2.numel(),
                                       torch.cuda.current_stream(device).cuda_stream, mask)

        ws_buf2 = torch.empty(5242880, dtype=torch.uint8, device=device)
        t_ring = graph_per_launch_ms(torch, lambda: ring(3), stream)
        lib.mha_hd64_set_fused_combine(0)
        t_main2 = graph_per_launch_ms(torch, lambda: ring(1), stream)
        t_comb2 = graph_per_launch_ms(torch, lambda: ring(2), stream)
        t_two = graph_per_launch_ms(torch, lambda: ring(3), stream)
        lib.mha_hd64_set_fused_combine(1)
        t_call = statistics.median(event_durations_ms(torch, full_call, 200, stream)[20:])
        achieved = flops / (t_main * 1e-3) / 1e12
        mfma_busy = load_traffic("direct16_mfma_busy_cycles_per_simd")
        rocprof_ns = load_traffic("direct16_rocprof_median_ns")
        rocprof_avg_ns = load_traffic("direct16_rocprof_avg_ns")
        traffic = load_traffic({22: "direct16_kernel_bytes_per_launch", 21: "direct_kernel_bytes_per_launch"}.get(
            q_waves, "main_kernel_bytes_per_launch"))
        two = " in two passes of 4 tiles" if nkv > 1024 else ""
        kname = {22: f"mha_hd64_direct16_kernel<f16,4 waves,4 tiles> (single pass: 16 query rows x all {nkv} keys "
                     f"per workgroup{two}, no split)",
                 21: f"mha_hd64_direct_kernel<f16,4 waves,4 tiles> (single pass: 32 query rows x all {nkv} keys per "
                     f"workgroup{two}, no split)"}.get(
            q_waves, f"mha_hd64_fwd_kernel<f16,f16,{q_waves},{kv_waves}> ({splits}-way KV split, in-launch combine)")
        result["roofline"] = {
            "bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_F16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_F16_TFLOPS, 4), "traffic": traffic,
            # from the committed PMC passes (profiles/traffic.json): measured HBM bytes per launch over
            # this run's kernel time, and SQ_VALU_MFMA_BUSY_CYCLES per SIMD over the kernel's cycles
            # at the 2.4 GHz peak clock (a lower bound on the busy fraction at the clock held)
            "hbm_gbs_measured_bytes": None if traffic is None else round(traffic / (t_main * 1e-3) / 1e9, 1),
            "mfma_busy_frac_pmc": (None if mfma_busy is None or q_waves != 22
                                   else round(mfma_busy / (t_main * 1e-3 * 2.4e9), 4)),
            "kernel": kname,
            "kernel_us": round(t_main * 1e3, 3),
            # the same kernel's MEDIAN begin-to-end duration in the committed rocprofv3 --kernel-trace
            # --stats trace of this bench command (profiles/r04, tools/profile_round.sh): the median,
            # not the average, because the tracer's per-dispatch completion signal inflates a few
            # dispatches (the r03 average exceeded the step time); checked against this run's step
            # time below (rocprof_kernel_le_step)
            "frac_rocprof_median": (None if rocprof_ns is None or q_waves != 22
                                    else round(flops / (rocprof_ns * 1e-9) / 1e12 / PEAK_F16_TFLOPS, 4)),
            "rocprof_median_us": None if rocprof_ns is None or q_waves != 22 else round(rocprof_ns * 1e-3, 3),
            #  the trace's AVERAGE beside the median, with its own <= step check
            "rocprof_avg_us": None if rocprof_avg_ns is None or q_waves != 22 else round(rocprof_avg_ns * 1e-3, 3),
            "frac_rocprof_avg": (None if rocprof_avg_ns is None or q_waves != 22
                                 else round(flops / (rocprof_avg_ns * 1e-9) / 1e12 / PEAK_F16_TFLOPS, 4)),
            "direct32_kernel_us": None if t_direct32 is None else round(t_direct32 * 1e3, 3),
            "ring_split_plan_us": {"in_launch_combine": round(t_ring * 1e3, 3), "main": round(t_main2 * 1e3, 3),
                                   "combine": round(t_comb2 * 1e3, 3), "two_kernels": round(t_two * 1e3, 3)},
            "timing": "graph replay of 200 back-to-back launches per kernel on the launch stream",
            "flops_per_launch": flops, "algorithmic_bytes_per_call": call_bytes(1, 4, nq, nkv),
        }
        rp = result["roofline"].get("rocprof_median_us")
        # a kernel cannot take longer than the step that contains it
        result["roofline"]["rocprof_kernel_le_step"] = None if rp is None else bool(rp <= ms_per_step * 1e3)
        ra = result["roofline"].get("rocprof_avg_us")
        result["roofline"]["rocprof_avg_le_step"] = None if ra is None else bool(ra <= ms_per_step * 1e3)
        result["isolated_call_us"] = round(t_call * 1e3, 3)
        result["cold_inputs"] = cold_inputs(torch, lightglue_amd, stream, q, k, v, barrier, reduce_max, ws)
        result["mall_inputs"] = cold_inputs(torch, lightglue_amd, stream, q, k, v, barrier, reduce_max, ws,
                                            pool_mib=96)

        # Batched launch: `batched` independent calls stacked in the batch dimension of one launch.
        B = args.batched
        qb, kb, vb = synth.qkv(300 + rank, nq, nkv, batch=B)
        qb, kb, vb = (torch.from_numpy(x).to(device).half().contiguous() for x in (qb, kb, vb))
        ob = torch.empty_like(qb)

        def batched():
            with torch.cuda.stream(stream):
                lightglue_amd.mha_hd64_batched(qb, kb, vb, out=ob)

        for _ in range(20):
            batched()
        tb_ev = statistics.median(event_durations_ms(torch, batched, 100, stream)[10:])
        # back-to-back launches replayed from a graph, as the headline's steps (events around each
        # single launch, which include the event records' own gaps, beside it)
        tb = graph_per_launch_ms(torch, lambda: lightglue_amd.mha_hd64_batched(qb, kb, vb, out=ob), stream)
        result["batched"] = {
            "calls_per_launch": B, "launch_us": round(tb * 1e3, 3), "launch_us_events": round(tb_ev * 1e3, 3),
            "timing": "graph replay of 200 back-to-back launches",
            "calls_per_s_per_gpu": round(B / (tb * 1e-3), 1),
            "tflops": round(B * flops / (tb * 1e-3) / 1e12, 2),
            "frac": round(B * flops / (tb * 1e-3) / 1e12 / PEAK_F16_TFLOPS, 4),
        }
        # more calls per launch (a pair stream of 16 / 32 / 64 pairs' calls stacked): the planner's plan,
        # graph replay of 50 back-to-back launches
        sweep_b = {}
        for B2 in (16, 32, 64):
            qs, ks, vs = (torch.from_numpy(x).to(device).half().contiguous()
                          for x in synth.qkv(310 + B2 + rank, nq, nkv, batch=B2))
            os_ = torch.empty_like(qs)
            # the persistent streaming kernel forced (plan 23; the planner's own choice past one round
            # of 128-row blocks), timed interleaved with the planner's plan (A/B/A/B replays: no order
            # or clock-drift bias)
            def stream_launch(qs=qs, ks=ks, vs=vs, os_=os_, B2=B2):
                st = lib.mha_hd64_launch_forced(qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), os_.data_ptr(), B2, 4, nq,
                                                nkv, 0, 0, 23, 0, 0, ws_buf2.data_ptr(), ws_buf2.numel(),
                                                torch.cuda.current_stream(device).cuda_stream, 3)
                assert st == 0
            t2, t3 = graphs_interleaved_ms(
                torch, [lambda qs=qs, ks=ks, vs=vs, os_=os_: lightglue_amd.mha_hd64_batched(qs, ks, vs, out=os_),
                        stream_launch], stream, k=50)
            sweep_b[str(B2)] = {"launch_us": round(t2 * 1e3, 3), "calls_per_s_per_gpu": round(B2 / (t2 * 1e-3), 1),
                                "frac": round(B2 * flops / (t2 * 1e-3) / 1e12 / PEAK_F16_TFLOPS, 4)}
            sweep_b[str(B2)]["stream_kernel"] = {
                "launch_us": round(t3 * 1e3, 3),
                "frac": round(B2 * flops / (t3 * 1e-3) / 1e12 / PEAK_F16_TFLOPS, 4),
                "timing": "interleaved with the planner's plan, median of 7 replays each"}
            del qs, ks, vs, os_
        result["batched"]["more_calls_per_launch"] = sweep_b
        # two streams of 16-call launches (two pair streams): one launch's prologue and tail overlap
        # the other's steady state (tools/batched_streams.py sweeps B x streams)
        ov = overlapped_batched(torch, lightglue_amd, device, nq, nkv, rank, flops, B=16, S=2)
        result["batched"]["two_streams_16_calls"] = ov
        best_b, best = max(((B, result["batched"]["frac"]),) + tuple((int(b), v["frac"]) for b, v in sweep_b.items()),
                           key=lambda x: x[1])
        if ov["frac"] > best:
            best_b, best = "2 streams x 16", ov["frac"]

        # The 70 % bar read against the saturated form: one call alone is bounded by the dependent
        # launch boundary (MI355X_MICROARCH.md price list, row 'boundary': 1.45 us between trivial
        # 256-workgroup kernels) against an ideal 0.43 us of MFMA work.
        result["roofline"]["ideal_us_at_peak"] = round(flops / (PEAK_F16_TFLOPS * 1e12) * 1e6, 4)
        result["roofline"]["launch_boundary_floor_us"] = 1.45
        result["roofline"]["saturated"] = {"form": f"{best_b} calls per launch (batched), best of 8 / 16 / 32 / 64",
                                           "frac": best, "frac_8_calls": result["batched"]["frac"]}
        # What this instruction mix sustains on the part (measured, not the 2.5 PF spec): the
        # head_dim-64 step's MFMAs with its softmax density beside them, registers only
        # (tools/mb_mfma_shape.hip), and the whole step with LDS reads, LDS-DMA refill and barrier
        # (tools/mb_step.hip, rows e and h); `frac` read against both
        att = ATTAINABLE
        result["roofline"]["attainable"] = dict(att, frac_vs_mix_ceiling=round(result["roofline"]["frac"] / att["mix_frac"], 4),
                                                saturated_frac_vs_mix_ceiling=round(best / att["mix_frac"], 4),
                                                saturated_frac_vs_full_step=round(best / att["full_step_frac"], 4))

        result["variants"] = variants(torch, lightglue_amd, device, stream, q, k, v, (qn, kn, vn), flops)
        result["variants"]["float_boundary"]["inputs"] = "raw fp32 (synth.qkv), not fp16-representable"
        result["concurrent_streams"] = concurrent_streams(torch, lightglue_amd, device, nq, nkv, rank, flops)
        result["matcher_attention"] = matcher_attention(torch, device, stream, rank, separate=args.matcher_separate)
        result["matcher_e2e_fp16"] = matcher_e2e(torch, device, stream, rank)
        result["matcher_e2e_fp32"] = matcher_e2e(torch, device, stream, rank, dtype=torch.float32)
        result["matcher_batched_pairs_fp16"] = {"n": nq, "pairs": matcher_batched_pairs(torch, device, stream, rank, n=nq)}
        result["matcher_pair_streams_fp16"] = {"n": nq, "streams": matcher_pair_streams(torch, lightglue_amd, device,
                                                                                        rank, n=nq)}
        # whole-job pair rate (BASELINE configs[4]): each GPU streams its own pairs through the matcher
        pair_rates = gather(dist, result["matcher_e2e_fp16"][str(nq)]["pairs_per_s"]
                            if str(nq) in result["matcher_e2e_fp16"] else None)
        stream_rates = gather(dist, max(v["pairs_per_s"] for v in
                                        result["matcher_pair_streams_fp16"]["streams"].values()))
        batch_rates = gather(dist, max(max(v["pairs_per_s"], v.get("pairs_per_s_2_streams", 0.0)) for v in
                                       result["matcher_batched_pairs_fp16"]["pairs"].values()))
        if all(p is not None for p in pair_rates):
            result["pairs_per_s_all_gpus"] = {"matcher_e2e_fp16": round(sum(pair_rates), 1), "n": nq,
                                              "per_rank": pair_rates,
                                              "pair_streams_best": round(sum(stream_rates), 1),
                                              "pair_streams_per_rank": stream_rates,
                                              "batched_pairs_best": round(sum(batch_rates), 1),
                                              "batched_pairs_per_rank": batch_rates}

    if args.sweep and rank == 0:
        sweep(torch, lib, device, stream, nq, nkv)
    if rank == 0 and ws == 1 and args.full and not args.no_cpu_baseline and not args.quick:  # CPU baseline: N=1 only
        result["cpu_baseline"] = cpu_baseline(args.cpu_seconds, nq, nkv)
    if rank == 0:
        print(json.dumps(result), file=result_out, flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
