#!/usr/bin/env python3
"""Benchmark of the HippoMM hot path on MI355X (contract: see the round brief).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload cfg2|cfg5] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the headline line (value, ms_per_step, ...).  Everything else
the benchmark measures or checks -- the count read-back variant of the step, the roofline and per-kernel table, the
all-gather alone, the scan and the other N = 1 legs, the CPU baselines and every comparison with the oracle -- runs only
with --full.  --dump-outputs DIR writes what the last timed step computed (see dump_outputs) before anything else runs.

`--gpus N` with N > 1 and no torchrun environment launches the N ranks itself: the parent process never touches the
GPU, starts `python -m torch.distributed.run` as a child, exits non-zero when fewer than N GPUs are visible and
returns the child's exit code.  A rank whose WORLD_SIZE disagrees with --gpus refuses to run.

Workloads
  cfg2 (default; BASELINE.json configs[1]): ImageBind-huge ViT-H/14 vision tower, bf16 MFMA, 256 synthetic 224x224
        frames per GPU per step.  A step = one pass of the path over one batch: encode the local 256 frames ->
        (N > 1: one RCCL all-gather of the (256,1024) fp32 embeddings) -> cosine key-frame selection on the
        gathered matrix.  Weak scaling: per-GPU work is fixed, value = N*256*K / time.
  cfg5 (BASELINE.json configs[4]): a 1-hour video at 1 fps = 3600 frames in contiguous time shards of ceil(3600/N)
        frames per rank -> encode -> ONE all-gather -> global selection on every rank.  Strong scaling: total work
        is fixed, value = 3600*K / time; the line also carries the all-gather time and whether the kept indices
        equal the CPU oracle's on the same gathered matrix.
The frames are synthetic "scenes": a low-frequency random pattern per scene (6 consecutive frames) plus pixel noise,
so that the random-init tower yields distinct embeddings per scene and the timed selection really drops frames.

With --full, at N = 1 (cfg2) the same JSON line carries the second half of BASELINE's metric under "scan" (the feature_search scan
over a resident 1M x 1024 fp32 store, k = 32, GB/s of algorithmic bytes), BASELINE cfg 3 under "joint_vision_audio",
the encoder's latency at the reference's own call sizes (32-frame buffer, one frame, one segment, one question) under
"reference_call_sizes", the consolidation timings and the CPU baselines of BASELINE.md section 4.

roofline      : the dominant kernel of the step (the bf16 GEMM instance with the largest time share),
                algorithmic FLOPs per launch / mean launch time measured live with HIP events on the
                launch stream; peak = 2.5 PFLOP/s dense bf16 (MI355X_MICROARCH.md); traffic is read from the
                committed PMC summary under profiles/ (null when there is none for this kernel).
cpu_baseline  : the fp32 oracle of the same tower (oracle/imagebind_oracle.py, torch CPU) timed on this
                host's cores on a bounded sample, rank 0, N=1 only.  A reported baseline, not a target.
parity_vs_oracle : rows of the TIMED batch (both halves of the two-stream split) against the fp32 oracle.
"""
from __future__ import annotations

import argparse
import glob
import hashlib
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA, MI355X
PEAK_HBM_GBS = 8000.0          # HBM3E spec
FRAMES_PER_GPU = 256           # cfg2
CFG5_FRAMES = 3600             # cfg5: one hour at 1 fps
SCENE_LEN = 6                  # frames per synthetic scene
SCAN_ROWS, SCAN_K = 1_000_000, 32
LAUNCH_TIMEOUT_S = 840.0       # wall-clock limit of a self-launched multi-rank run, below the outer `timeout 900` of tools/runs/*.sh
                               # (HMM_BENCH_LAUNCH_TIMEOUT_S overrides)
SCAN_FIRST_WARM_MS = 800.0     # the first leg on a freshly written store: see scan_bench
SCAN_WARM_MS = 60.0            # every scan leg is timed in steady state: see event_time_ms
# Rehearsal of the N > 1 code path on a box with fewer GPUs (HMM_BENCH_REHEARSAL=1): every rank uses cuda:0 and the
# collectives run over gloo.  Exercises launch, sharding, gathers, merges and the JSON line -- NOT RCCL, and the
# numbers are meaningless (the ranks share one GPU); the line says so and is never a result.
REHEARSAL = os.environ.get("HMM_BENCH_REHEARSAL") == "1"


# ------------------------------------------------------------------------------------------------
# launching
# ------------------------------------------------------------------------------------------------
def visible_gpu_count(topology: str = "/sys/class/kfd/kfd/topology/nodes", dri: str = "/dev/dri") -> int:
    """GPUs this process would see, counted WITHOUT opening the HIP runtime (the self-launching parent must never touch the
    GPU).  The KFD topology in sysfs lists one node per agent of the HOST, GPUs are the nodes with SIMDs; inside a container
    only the GPUs whose render node (`drm_render_minor`) is mapped and accessible under /dev/dri are usable, so those are the
    ones counted; ROCR_VISIBLE_DEVICES / HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES narrow the set as the runtime would."""
    n = 0
    have_dri = os.path.isdir(dri)
    for path in glob.glob(os.path.join(topology, "*", "properties")):
        try:
            props = dict(line.split(None, 1) for line in open(path).read().splitlines() if " " in line)
        except OSError:
            continue
        if int(props.get("simd_count", "0")) <= 0:
            continue
        minor = props.get("drm_render_minor")
        if have_dri and minor is not None:
            node = os.path.join(dri, f"renderD{int(minor)}")
            if not (os.path.exists(node) and os.access(node, os.R_OK | os.W_OK)):
                continue
        n += 1
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        val = os.environ.get(var)
        if val is not None:
            n = min(n, len([v for v in val.split(",") if v.strip() != ""]))
    return n


def launch_ranks(n: int, argv) -> int:
    """Parent of a self-launched multi-GPU run.  Never initialises the GPU: the GPUs are counted from sysfs and the ranks are
    fresh child processes."""
    visible = visible_gpu_count()
    if visible < n and not REHEARSAL:
        print(f"bench.py: --gpus {n} but only {visible} GPU(s) visible", file=sys.stderr)
        return 3
    port = 29500 + os.getpid() % 2000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *argv]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.setdefault("NCCL_DEBUG", "VERSION")                  # one stderr line naming the RCCL build the ranks loaded
    # The ranks are a fresh process group of their own: if they are not done within the wall-clock limit (a rank stuck in a
    # collective, a rendezvous that never completes) the whole group is killed and the run fails loudly instead of hanging the
    # box.  Nothing here re-executes a process that has touched the GPU: the parent never has, the children are new.
    limit = float(os.environ.get("HMM_BENCH_LAUNCH_TIMEOUT_S", LAUNCH_TIMEOUT_S))
    import signal

    def kill_group(proc):
        for sig, grace in ((signal.SIGTERM, 10.0), (signal.SIGKILL, 10.0)):
            try:
                os.killpg(proc.pid, sig)
            except ProcessLookupError:
                return
            try:
                proc.wait(timeout=grace)
                return
            except subprocess.TimeoutExpired:
                continue

    def on_term(signum, _frame):                              # an outer `timeout` / the driver ends the parent: take the ranks along
        raise KeyboardInterrupt(f"signal {signum}")
    old_term = signal.signal(signal.SIGTERM, on_term)
    proc = subprocess.Popen(cmd, env=env, start_new_session=True)
    try:
        return proc.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"bench.py: the {n} ranks did not finish within {limit:.0f} s; killing their process group", file=sys.stderr)
        return 5
    except BaseException as exc:                              # Ctrl-C, SIGTERM, anything: the ranks live in their own session and
        print(f"bench.py: interrupted ({exc!r}); killing the ranks' process group", file=sys.stderr)      # would otherwise keep the GPUs
        return 130
    finally:
        if proc.poll() is None:
            kill_group(proc)
        signal.signal(signal.SIGTERM, old_term)


# ------------------------------------------------------------------------------------------------
# synthetic input and the step (also driven on CPU / gloo by tests/test_cpu_bench_step.py)
# ------------------------------------------------------------------------------------------------
def synthetic_frames(lo: int, hi: int, device, amp: float = 1.5, sigma: float = 0.3) -> torch.Tensor:
    """Frames lo..hi-1 of the synthetic video, BIT-identical whatever the sharding and whatever process makes them: scene
    s = frame // SCENE_LEN is a low-frequency pattern (4x4 random field seeded by s, bilinear to 224x224), each frame adds
    pixel noise seeded by its own index.  Everything is drawn and computed on `device` (Philox streams, element-wise
    kernels): the host-side version of this function gave fp32 pixels that differed in the last bit with the number of
    OpenMP threads (torch.distributed.run sets OMP_NUM_THREADS=1), enough to move 96 % of the bf16 embeddings of a
    multi-rank run away from the one-process run.  Stands for CLIP-normalised pixels, i.e. post-load_data."""
    dev = torch.device(device)
    out = torch.empty(hi - lo, 3, 224, 224, dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev)
    scene, scene_id = None, -1
    for i in range(lo, hi):
        s = i // SCENE_LEN
        if s != scene_id:
            g.manual_seed(1000 + s)
            base = torch.randn(1, 3, 4, 4, generator=g, device=dev) * amp
            scene = torch.nn.functional.interpolate(base, size=(224, 224), mode="bilinear", align_corners=False)[0]
            scene_id = s
        g.manual_seed(7_000_000 + i)
        noise = torch.randn(3, 224, 224, generator=g, device=dev)
        out[i - lo] = scene + sigma * noise
    return out


def make_step(frames_local, counts, encode_fn, gather_fn, select_fn):
    """One pass of the hot path over this rank's batch: encode -> all-gather -> global key-frame selection."""
    def step():
        emb = encode_fn(frames_local)
        feats = gather_fn(emb, counts)
        return feats, select_fn(feats)
    return step


def timed_steps(step, steps: int, warmup: int, sync, barrier, reduce_max):
    """The timing contract: W untimed steps, then exactly K steps bracketed by barrier + device sync, max over ranks."""
    last = None
    for _ in range(warmup):
        last = step()
    sync(); barrier(); sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step()
    sync(); barrier(); sync()
    return reduce_max(time.perf_counter() - t0), last


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(folder: str, feats: torch.Tensor, kept: torch.Tensor, limit_bytes: int = DUMP_LIMIT_BYTES) -> None:
    """--dump-outputs: what a caller of the timed path receives from its last step, as .npy files in `folder`:
    embeddings.npy (the gathered (n, 1024) fp32 matrix that the selection ran on) and kept_indices.npy (the kept frame
    indices, float64).  Should the matrix not fit in `limit_bytes` with the indices, a fixed, seeded sample of its rows is
    written instead, increasing, and embedding_rows.npy (float64) names them."""
    import numpy as np
    os.makedirs(folder, exist_ok=True)
    emb = feats.detach().float().cpu().numpy()
    out = {"kept_indices": kept.detach().cpu().numpy().astype(np.float64)}
    row_bytes = emb.shape[1] * 4 + 8
    budget = (limit_bytes - out["kept_indices"].nbytes - 4096) // row_bytes
    if emb.shape[0] > budget:
        rows = np.sort(np.random.default_rng(0).choice(emb.shape[0], size=budget, replace=False))
        emb = emb[rows]
        out["embedding_rows"] = rows.astype(np.float64)
    out["embeddings"] = np.ascontiguousarray(emb, dtype=np.float32)
    for name, arr in out.items():
        np.save(os.path.join(folder, f"{name}.npy"), arr)


def host_threads() -> int:
    """THE core count of every CPU baseline in the line: the threads the baseline actually runs on = torch's intra-op pool
    (physical cores on these hosts; os.cpu_count() counts SMT siblings).  numpy / BLAS legs are pinned to the same number with
    threadpoolctl, so `cores` means one thing everywhere."""
    return int(torch.get_num_threads())


class blas_threads:
    """with blas_threads(): numpy's BLAS / OpenMP pools limited to host_threads()."""

    def __enter__(self):
        try:
            from threadpoolctl import threadpool_limits
            self._ctx = threadpool_limits(limits=host_threads())
            self._ctx.__enter__()
        except Exception:                                   # noqa: BLE001 - threadpoolctl missing: default pools, still reported
            self._ctx = None
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
        return False


def mfma_roofline(flops: float, ms: float, scope: str) -> dict:
    """Roofline object of a whole forward (scope says what was timed): nominal FLOPs (SURVEY 8d accounting) / wall time against the
    dense bf16 MFMA peak.  traffic: null (no PMC pass for this workload)."""
    tf = flops / ms / 1e9
    return {"bound": "mfma", "scope": scope, "achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tf / PEAK_BF16_TFLOPS, 4), "traffic": None, "flops": flops, "ms": round(ms, 4),
            "flops_accounting": "nominal (reference's un-folded patch conv, every block on every token)"}


def event_time_ms(fn, iters, warmup=2, warm_ms=0.0, groups=1, detail=None):
    """ms per call over `iters` back-to-back calls (HIP events on the current stream) after `warmup` calls and, when
    `warm_ms` > 0, after at least that many milliseconds of the same calls: sub-millisecond kernels timed right after the
    device has idled -- a read-back, host work -- run their first 10-30 launches 10-25 % slow while the clocks come back up
    (tools/multi_thermal_probe.py, profiles/r5_multi_thermal.json: the 16-query scan 0.85 / 0.70 / 0.67 / 0.66 / 0.65 ms over its
    first five groups of ten launches).  That, not the kernel, was round 4's batched_16_queries 0.672 -> 0.765 ms: the leg had
    moved behind a read-back and was timed over launches 4-13.

    `groups` > 1: the same `iters` calls, still back to back with no synchronisation in between, with an event after every
    iters / groups of them; the MEDIAN group is returned and `detail` receives every group, the mean and what the host spent
    enqueueing a call (far below the device time: the queue stays ahead)."""
    for _ in range(warmup):
        fn()
    if warm_ms > 0:                      # never for a leg that contains a collective: the number of calls would differ per rank
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < warm_ms:
            for _ in range(8):
                fn()
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    per = max(1, iters // groups)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(groups + 1)]
    evs[0].record()
    t0 = time.perf_counter()
    for g in range(groups):
        for _ in range(per):
            fn()
        evs[g + 1].record()
    host_s = time.perf_counter() - t0
    torch.cuda.synchronize()
    by_group = [evs[g].elapsed_time(evs[g + 1]) / per for g in range(groups)]
    mean = evs[0].elapsed_time(evs[groups]) / (per * groups)
    if detail is not None:
        detail.update({"groups_ms": [round(x, 4) for x in by_group], "mean_ms": round(mean, 4),
                       "host_us_per_call": round(host_s / (per * groups) * 1e6, 1)})
    return _median(by_group) if groups > 1 else mean


def profile_summary(pattern: str, kernel: str):
    """Newest committed PMC summary under profiles/ that names `kernel` -> (traffic bytes per launch, file) or (None, None)."""
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), reverse=True):
        try:
            doc = json.load(open(path))
        except (OSError, ValueError):
            continue
        if doc.get("kernel") == kernel and "traffic_bytes_per_launch" in doc:
            return int(doc["traffic_bytes_per_launch"]), os.path.relpath(path, ROOT)
    return None, None


def rank_proof(world: int, rank: int, local_rank: int, n_frames: int):
    """Self-proving N (every rank calls this): a sum of ones over the data-path backend, every rank's device, and the shard each
    one encoded."""
    ones = torch.ones(1, dtype=torch.int32, device="cuda")
    dist.all_reduce(ones, op=dist.ReduceOp.SUM)
    props = torch.cuda.get_device_properties(torch.cuda.current_device())
    mine = {"rank": rank, "local_rank": local_rank, "device": torch.cuda.current_device(), "name": props.name,
            "gcn_arch": getattr(props, "gcnArchName", None), "pci_bus_id": getattr(props, "pci_bus_id", None),
            "frames": n_frames}
    everyone = [None] * world
    dist.all_gather_object(everyone, mine)
    return {"backend": dist.get_backend(), "all_reduced_rank_count": int(ones.item()), "ranks": everyone}


def committed_n1_value(workload: str):
    """The 1-GPU value of the same workload that is on disk: the driver's newest BENCH_r*.json (cfg2, the default run) or a
    committed profiles/*bench_line*.json of that workload -> {"value", "source"} or None."""
    cands = sorted(glob.glob(os.path.join(ROOT, "BENCH_r*.json")), reverse=True) + \
        sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_line*.json")), reverse=True)
    for path in cands:
        try:
            doc = json.load(open(path))
        except (OSError, ValueError):
            continue
        doc = doc.get("parsed", doc) if isinstance(doc, dict) else None
        if not isinstance(doc, dict) or doc.get("n_gpus") != 1 or "value" not in doc:
            continue
        wl = str(doc.get("config", {}).get("workload", ""))
        if ("cfg2" in wl) == (workload == "cfg2") and ("cfg5" in wl) == (workload == "cfg5"):
            return {"value": float(doc["value"]), "source": os.path.relpath(path, ROOT)}
    return None


# ------------------------------------------------------------------------------------------------
# N = 1 extras
# ------------------------------------------------------------------------------------------------
def gemm_roofline(batch=FRAMES_PER_GPU):
    """The kernels of one vision-tower block at the step's batch, launched IN SEQUENCE on the current stream exactly as the tower
    chains them (so that every GEMM finds its operands where the previous kernel left them), each bracketed by HIP events on
    that stream; 6 blocks after 2 warm-up blocks, median per kernel.  The roofline object is that of the dominant kernel;
    the table also carries each GEMM timed alone in a loop (`ms_isolated`), which is what round 1 reported."""
    from hippomm_amd import _lib as L
    lib = L.load()
    T, D, H, MLP = 257, 1280, 16, 5120
    R = batch * T
    dev = "cuda"
    x = torch.randn(R, D, device=dev)
    a = torch.empty(R, D, dtype=torch.bfloat16, device=dev)
    big = torch.empty(R, MLP, dtype=torch.bfloat16, device=dev)
    g1, b1 = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    wq = (torch.randn(3 * D, D, device=dev) * 0.02).to(torch.bfloat16); bq = torch.zeros(3 * D, device=dev)
    wo = (torch.randn(D, D, device=dev) * 0.02).to(torch.bfloat16); bo = torch.zeros(D, device=dev)
    w1 = (torch.randn(MLP, D, device=dev) * 0.02).to(torch.bfloat16); bb1 = torch.zeros(MLP, device=dev)
    w2 = (torch.randn(D, MLP, device=dev) * 0.02).to(torch.bfloat16); bb2 = torch.zeros(D, device=dev)
    cls_rows = torch.empty(batch, D, dtype=torch.bfloat16, device=dev)
    qkv_cls = torch.empty(batch, 3 * D, dtype=torch.bfloat16, device=dev)
    S = L.stream_ptr

    def cls_proj():
        cls_rows.copy_(a.view(batch, T, D)[:, 0])
        return lib.hmm_op_gemm_bf16(cls_rows.data_ptr(), wq.data_ptr(), bq.data_ptr(), qkv_cls.data_ptr(), batch, 3 * D, D, 0, S())

    gemm = lambda A, W, Bv, Cc, N, K, epi: lib.hmm_op_gemm_bf16(A.data_ptr(), W.data_ptr(), Bv.data_ptr(), Cc.data_ptr(), R, N, K, epi, S())
    chain = [
        ("layernorm[norm_1]", None, lambda: lib.hmm_op_layernorm_bf16(x.data_ptr(), g1.data_ptr(), b1.data_ptr(), a.data_ptr(), R, D, 1e-6, S())),
        ("gemm_bf16[cls rows in_proj]", 2.0 * batch * 3 * D * D, cls_proj),
        ("qkv_attention[in_proj+attention]", 2.0 * (R - batch) * 3 * D * D + 4.0 * batch * H * T * T * (D // H),
         lambda: lib.hmm_op_qkv_attention_bf16(a.data_ptr(), wq.data_ptr(), bq.data_ptr(), qkv_cls.data_ptr(), big.data_ptr(), batch, S())),
        ("gemm_bf16[out_proj+residual]", 2.0 * R * D * D, lambda: gemm(big, wo, bo, x, D, D, 2)),
        ("layernorm[norm_2]", None, lambda: lib.hmm_op_layernorm_bf16(x.data_ptr(), g1.data_ptr(), b1.data_ptr(), a.data_ptr(), R, D, 1e-6, S())),
        ("gemm_bf16[mlp_fc1+gelu]", 2.0 * R * MLP * D, lambda: gemm(a, w1, bb1, big, MLP, D, 1)),
        ("gemm_bf16[mlp_fc2+residual]", 2.0 * R * D * MLP, lambda: gemm(big, w2, bb2, x, D, MLP, 2)),
    ]
    times = {name: [] for name, _, _ in chain}
    for blk in range(8):
        evs = []
        for name, _, fn in chain:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); L.check(fn(), name); e1.record()
            evs.append((name, e0, e1))
        torch.cuda.synchronize()
        if blk >= 2:
            for name, e0, e1 in evs:
                times[name].append(e0.elapsed_time(e1))
        x.normal_()
    table = []
    for name, flops, _ in chain:
        ms = sorted(times[name])[len(times[name]) // 2]
        rec = {"kernel": name, "ms": round(ms, 4), "launches_per_step": 31 if "cls" in name or "qkv_attention" in name else 32}
        if flops:
            rec["tflops"] = round(flops / ms / 1e9, 1)
        table.append(rec)
    # the same GEMMs alone in a loop (cold operand placement: what round 1 reported)
    iso = {"gemm_bf16[out_proj+residual]": (big, wo, bo, x, D, D, 2), "gemm_bf16[mlp_fc1+gelu]": (a, w1, bb1, big, MLP, D, 1),
           "gemm_bf16[mlp_fc2+residual]": (big, w2, bb2, x, D, MLP, 2)}
    for rec in table:
        if rec["kernel"] in iso:
            args = iso[rec["kernel"]]
            rec["ms_isolated"] = round(event_time_ms(lambda: L.check(gemm(*args), "gemm"), 10), 4)
            rec.update({"M": R, "N": args[4], "K": args[5]})
    gemms = [r for r in table if r["kernel"].startswith("gemm_bf16[") and "cls" not in r["kernel"]]
    dom = max(gemms, key=lambda r: r["ms"])
    traffic, src = profile_summary("r*_gemm_pmc_summary.json", dom["kernel"]) if R == 65792 else (None, None)
    out_bytes = 8 if "residual" in dom["kernel"] else 2           # fp32 read-modify-write / bf16 store, per element
    roof = {"bound": "mfma", "kernel": dom["kernel"], "achieved": dom["tflops"], "peak": PEAK_BF16_TFLOPS,
            "unit": "TFLOP/s", "frac": round(dom["tflops"] / PEAK_BF16_TFLOPS, 4), "traffic": traffic,
            "traffic_source": src, "flops_per_launch": 2.0 * dom["M"] * dom["N"] * dom["K"],
            "ms_per_launch": dom["ms"], "timed": "in the tower's kernel sequence, HIP events on the launch stream",
            "algorithmic_bytes_per_launch": 2 * (dom["M"] * dom["K"] + dom["N"] * dom["K"]) + dom["M"] * dom["N"] * out_bytes}
    return roof, table


def scan_bench(do_cpu):
    from hippomm_amd.vector_ops import FeatureStore
    from hippomm_amd import _lib as L
    g = torch.Generator(device="cuda").manual_seed(42)
    rows = torch.empty(SCAN_ROWS, 1024, dtype=torch.float32, device="cuda")
    for s in range(0, SCAN_ROWS, 125_000):
        blk = torch.randn(125_000, 1024, generator=g, device="cuda")
        rows[s:s + 125_000] = blk / blk.norm(dim=1, keepdim=True)
    q = torch.randn(1024, generator=torch.Generator(device="cuda").manual_seed(43), device="cuda")
    store = FeatureStore(rows)
    d_query, d_kernel, d_pre, d_multi = {}, {}, {}, {}
    # The first leg streams a store that was allocated and written a moment ago.  In about half of the processes the streaming kernel
    # then runs 4-5 % slow for the first 0.1-0.5 s (595-615 us inside a query against 570-583, in the kernel trace too; no gaps, the
    # finishing kernel unchanged; the kernel alone is just as slow when it is timed inside that window) and settles afterwards:
    # rounds 4-6 read it as "38 us of whole-query overhead" because this leg came first and the kernel-only leg 0.1 s later
    # (profiles/r6_scan_first_leg_transient.txt).  So this leg warms for 0.8 s, not 60 ms.
    ms_query = event_time_ms(lambda: store.search_device(q, SCAN_K), 50, warmup=3, warm_ms=SCAN_FIRST_WARM_MS, groups=5, detail=d_query)
    # the streaming kernel alone (dominant kernel of the scan)
    lib = L.load()
    cand = torch.empty(2048 * SCAN_K, dtype=torch.int64, device="cuda")
    ms_kernel = event_time_ms(lambda: L.check(lib.hmm_op_scan_topk_only(rows.data_ptr(), SCAN_ROWS, q.data_ptr(), SCAN_K,
                                                                        cand.data_ptr(), L.stream_ptr()), "scan"), 50,
                             warm_ms=SCAN_WARM_MS, groups=5, detail=d_kernel)
    algo_bytes = SCAN_ROWS * 4096.0
    traffic, src = profile_summary("r*_scan_pmc_summary.json", "scan_topk_kernel")
    out = {
        "metric": "cosine-scan GB/s (feature_search, 1M x 1024 fp32 store, top-32, 1 query)",
        "value": round(algo_bytes / ms_query / 1e6, 1), "unit": "GB/s", "ms_per_query": round(ms_query, 4),
        "timing": "every scan leg: 50 back-to-back calls, one HIP event after every 10, no synchronisation in between; the MEDIAN "
                  "group is the figure, all five groups and the mean of the 50 are in *_timing (see event_time_ms)",
        "ms_per_query_timing": d_query, "dtype": "f32",
        "roofline": {"bound": "hbm", "kernel": "scan_topk_kernel", "achieved": round(algo_bytes / ms_kernel / 1e6, 1),
                     "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(algo_bytes / ms_kernel / 1e6 / PEAK_HBM_GBS, 4),
                     "traffic": traffic, "traffic_source": src,
                     "bytes_per_launch": algo_bytes, "ms_per_launch": round(ms_kernel, 4), "ms_per_launch_timing": d_kernel},
    }
    # the same query through the bf16 shadow store (reported SEPARATELY, against 2048 B per row; the headline above is
    # the fp32 store): candidates from one pass over the shadow, exact fp32 re-score -> the same indices and similarity bits
    store.build_shadow()
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    ms_pre = event_time_ms(lambda: store.search_prefiltered_device(q, SCAN_K, stats), 50, warmup=3, warm_ms=SCAN_WARM_MS, groups=5,
                           detail=d_pre)
    i_ex, s_ex = store.search_device(q, SCAN_K)
    i_pre, s_pre = store.search_prefiltered_device(q, SCAN_K, stats)
    shadow_bytes = SCAN_ROWS * 2048.0
    pre_traffic, pre_src = profile_summary("r*_prefilter_pmc_summary.json", "prefilter_topk_kernel")
    out["prefilter_bf16_shadow"] = {
        "what": "hmm_cosine_topk_prefilter: bf16 shadow (row / ||row||, 2048 B per row) streamed for candidates under a proven "
                "error bound, exact fp32 re-score of the candidates; same result as the fp32 scan",
        "ms_per_query": round(ms_pre, 4), "ms_per_query_timing": d_pre, "speedup_vs_fp32_scan": round(ms_query / ms_pre, 2),
        "identical_to_fp32_scan": bool(torch.equal(i_ex, i_pre) and torch.equal(s_ex.view(torch.int32), s_pre.view(torch.int32))),
        "candidates_rescored": int(stats[0].item()), "saturated_lists": int(stats[1].item()),
        "roofline": {"bound": "hbm", "kernel": "prefilter_topk_kernel (+ prefilter_final_kernel)", "scope": "whole query",
                     "achieved": round(shadow_bytes / ms_pre / 1e6, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                     "frac": round(shadow_bytes / ms_pre / 1e6 / PEAK_HBM_GBS, 4), "traffic": pre_traffic, "traffic_source": pre_src,
                     "bytes_per_launch": shadow_bytes, "ms_per_launch": round(ms_pre, 4)},
        "extra_hbm_bytes_held": shadow_bytes}
    # batched questions: 16 queries per pass over the same store
    q16 = torch.randn(16, 1024, generator=torch.Generator(device="cuda").manual_seed(44), device="cuda")
    ms_multi = event_time_ms(lambda: store.search_multi_device(q16, SCAN_K), 50, warmup=3, warm_ms=SCAN_WARM_MS, groups=5, detail=d_multi)
    out["batched_16_queries"] = {"ms_per_pass": round(ms_multi, 4), "ms_per_pass_timing": d_multi, "us_per_query": round(ms_multi / 16 * 1e3, 1),
                                 "store_read_GBps": round(algo_bytes / ms_multi / 1e6, 1),
                                 "hbm_frac": round(algo_bytes / ms_multi / 1e6 / PEAK_HBM_GBS, 4),
                                 "speedup_vs_16_single_scans": round(16 * ms_query / ms_multi, 2)}
    # reference point: the same query through stock PyTorch-ROCm operators on the resident store (vector_ops.py:151-188
    # moved to the GPU as is: norms, matrix-vector product, division, top-k)
    def torch_scan():
        sims = (rows @ q) / (rows.norm(dim=1) * q.norm())
        return torch.topk(sims, SCAN_K)
    ms_torch = event_time_ms(torch_scan, 10, warmup=3, warm_ms=SCAN_WARM_MS)
    out["torch_rocm_reference"] = {"ms_per_query": round(ms_torch, 4), "GBps": round(algo_bytes / ms_torch / 1e6, 1),
                                   "what": "rows @ q / (rows.norm(dim=1) * q.norm()) + torch.topk on the same GPU"}
    if do_cpu:
        from oracle.vector_ops_oracle import top_k_cosine_similarity_oracle
        idx_gpu, _ = store.search_device(q, SCAN_K)
        host = rows.cpu().numpy()
        qh = q.cpu().numpy()
        with blas_threads():
            o_idx, _ = top_k_cosine_similarity_oracle(qh, host, SCAN_K)     # warm run (also the parity check)
            best = 1e9
            for _ in range(3):
                t0 = time.perf_counter()
                top_k_cosine_similarity_oracle(qh, host, SCAN_K)
                best = min(best, time.perf_counter() - t0)
        out["cpu_baseline"] = {"value": round(algo_bytes / best / 1e9, 2), "unit": "GB/s", "s_per_query": round(best, 3),
                               "cores": host_threads(), "kind": "port",
                               "sample": "numpy oracle (vector_ops.py:151-188 restated) on the full 1M x 1024 store, k=32, "
                                         f"best of 3 after a warm run; BLAS threads = {host_threads()} (host_threads())"}
        out["parity_vs_oracle"] = {"top32_indices_equal": idx_gpu.cpu().tolist() == [int(i) for i in o_idx]}
        del host
    out["retrieval"] = retrieval_bench(rows, do_cpu)
    del rows, store
    torch.cuda.empty_cache()
    return out


def retrieval_bench(rows, do_cpu):
    """The retrieval path as one latency (SURVEY 8f-1 + 8f-4): question string -> BPE ids -> text tower -> per-event top-5
    over the resident store cut into 2000 events of 500 rows -> results on the host; hippocampal_memory.py:2173-2177 ->
    :3143-3153 -> :3275-3277.  Beside it the reference's route on this host's cores: the fp32 oracle text tower and the
    Python loop of one numpy scan per event."""
    from hippomm_amd.encoder import HipTower, synthetic_state_dict
    from hippomm_amd.tokenizer import SimpleTokenizer
    from hippomm_amd.vector_ops import EventStore
    n_events, per_event = 2000, SCAN_ROWS // 2000
    events = EventStore.from_device_rows(rows, [per_event] * n_events)
    tok = SimpleTokenizer("", merges=[])                     # byte-level ids (the upstream merge table is not in this image)
    sd = synthetic_state_dict(("text",), seed=99)
    tower = HipTower("text", sd)
    question = "who opens the door after the phone rang?"
    emb = torch.empty(1, 1024, device="cuda")

    def ask():
        ids = tok([question]).cuda()
        tower.forward_into(ids, emb)
        hits = events.top_k_per_event(emb[0], 5)             # reads the results back: this is the synchronisation
        flat = [(float(s), e, int(i)) for e, (idx, sims) in enumerate(hits) for i, s in zip(idx, sims)]
        flat.sort(key=lambda h: -h[0])
        return flat[:5]

    ask(); ask()
    t = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        top = ask()
        t.append(time.perf_counter() - t0)
    def ask_device_ranked():                                 # the same, the final ranking on the device (EventStore.top_hits)
        tower.forward_into(tok([question]).cuda(), emb)
        return events.top_hits(emb[0], 5, 5)

    ask_device_ranked()
    t2 = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        top2 = ask_device_ranked()
        t2.append(time.perf_counter() - t0)
    events.build_shadow()

    def ask_device_ranked_prefilter():                       # the same through the bf16 shadow of the store (identical hits)
        tower.forward_into(tok([question]).cuda(), emb)
        return events.top_hits(emb[0], 5, 5, prefilter=True)

    ask_device_ranked_prefilter()
    t3 = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        top3 = ask_device_ranked_prefilter()
        t3.append(time.perf_counter() - t0)
    t_tower = event_time_ms(lambda: tower.forward_into(tok([question]).cuda(), emb), 10, warmup=2, warm_ms=SCAN_WARM_MS)
    q = emb[0].clone()
    t_scan = event_time_ms(lambda: events.search_segments_device(q, events.offsets, 5), 30, warmup=2, warm_ms=SCAN_WARM_MS)
    events.build_shadow()
    t_scan_pre = event_time_ms(lambda: events.search_segments_device(q, events.offsets, 5, prefilter=True), 30, warmup=2,
                               warm_ms=SCAN_WARM_MS)
    ex, pre = events.search_segments_device(q, events.offsets, 5), events.search_segments_device(q, events.offsets, 5, prefilter=True)
    pre_same = bool(torch.equal(ex[0], pre[0]) and torch.equal(ex[1].view(torch.int32), pre[1].view(torch.int32)) and torch.equal(ex[2], pre[2]))
    # the reference's loop UNCHANGED (hippocampal_memory.py:3143-3153): one top_k_cosine_similarity call per event with the event's
    # host array, as a drop-in: uploaded per call, and with hippomm_amd.vector_ops.enable_store_cache() (resident from the 2nd call)
    from hippomm_amd import vector_ops as vo
    host_events = [rows[e * per_event:(e + 1) * per_event].cpu().numpy() for e in range(100)]
    qh0 = q.cpu().numpy()

    def loop():
        t0 = time.perf_counter()
        for ev in host_events:
            vo.top_k_cosine_similarity(qh0, ev, 5)
        return (time.perf_counter() - t0) / len(host_events) * 1e3
    loop()
    ms_upload = min(loop() for _ in range(3))
    vo.enable_store_cache()
    try:
        loop()
        ms_cached = min(loop() for _ in range(3))
    finally:
        vo.disable_store_cache()
    del host_events
    out = {"what": "question -> tokenizer -> text tower (24 blocks, batch 1) -> top-5 per event over 2000 events x 500 rows "
                   "(one pass) -> the best 5 hits of all events, ranked on the device, on the host (EventStore.top_hits: what "
                   "INTEGRATION.md's patch for hippocampal_memory.py:3143-3153 + :3275-3277 calls); ms_end_to_end_host_ranked = the same "
                   "with every event's hits read back and ranked in Python as the reference's loop does",
           "ms_end_to_end": round(sorted(t2)[len(t2) // 2] * 1e3, 3),
           "ms_end_to_end_host_ranked": round(sorted(t)[len(t) // 2] * 1e3, 3),
           "ms_end_to_end_bf16_prefilter": round(sorted(t3)[len(t3) // 2] * 1e3, 3),
           "prefilter_hits_equal": [(e, i) for e, i, _ in top3] == [(e, i) for e, i, _ in top2] and
           [v for _, _, v in top3] == [v for _, _, v in top2],
           "ms_text_tower": round(t_tower, 3),
           "ms_per_event_scan_all_events": round(t_scan, 3), "events": n_events, "rows": n_events * per_event,
           "ms_per_event_scan_bf16_prefilter": round(t_scan_pre, 3), "prefilter_identical_to_fp32_scan": pre_same,
           "unchanged_reference_loop_ms_per_event": {"numpy_store_uploaded_per_call": round(ms_upload, 4),
                                                     "with_enable_store_cache": round(ms_cached, 4), "events_timed": 100,
                                                     "rows_per_event": per_event,
                                                     "store_cache_semantics": "opt-in; every call hashes the WHOLE host array "
                                                     "(xxh3, arrays <= 64 MB) before it trusts the resident copy, so an in-place "
                                                     "edit is a miss; above 64 MB only a 64 x 16 sample is compared "
                                                     "(hippomm_amd.vector_ops.enable_store_cache)"},
           "device_ranking_equals_host_ranking": [(e, i) for e, i, _ in top2] == [(e, i) for _, e, i in top]}
    if do_cpu:
        from oracle import imagebind_oracle as ib
        from oracle.vector_ops_oracle import top_k_cosine_similarity_oracle
        st = {k: v.detach().float().cpu() for k, v in sd.items()}
        ids = tok([question])
        ib.text_forward(ids, st)
        t0 = time.perf_counter()
        ref_q = ib.text_forward(ids, st)
        t_tower_cpu = time.perf_counter() - t0
        cos = torch.nn.functional.cosine_similarity(emb.cpu(), ref_q, dim=1)
        qh = q.cpu().numpy()
        host = rows[: 200 * per_event].cpu().numpy()         # the reference's loop on a bounded sample: 200 of the 2000 events
        with blas_threads():
            t0 = time.perf_counter()
            hits = [top_k_cosine_similarity_oracle(qh, host[e * per_event:(e + 1) * per_event], 5) for e in range(200)]
            t_loop = (time.perf_counter() - t0) * (n_events / 200)
        flat = [(float(s), e, int(i)) for e, (idx, sims) in enumerate(hits) for i, s in zip(idx, sims)]
        flat.sort(key=lambda h: -h[0])
        mine = sorted([h for h in _all_hits(events, q) if h[1] < 200], key=lambda h: -h[0])[:5]
        out["cpu_reference"] = {"ms_text_tower_oracle": round(t_tower_cpu * 1e3, 1), "ms_python_loop_all_events": round(t_loop * 1e3, 1),
                                "cores": host_threads(), "sample": "fp32 oracle text tower, 1 query; numpy scan per event on 200 of the "
                                "2000 events, scaled x10"}
        out["parity_vs_oracle"] = {"text_embedding_cos": round(float(cos.min()), 7),
                                   "top5_of_first_200_events_equal": [(e, i) for _, e, i in mine] == [(e, i) for _, e, i in flat[:5]]}
        out["speedup_vs_cpu_reference"] = round((t_tower_cpu + t_loop) * 1e3 / out["ms_end_to_end"], 1)
    del tower, sd
    torch.cuda.empty_cache()
    return out


def _all_hits(events, q):
    return [(float(s), e, int(i)) for e, (idx, sims) in enumerate(events.top_k_per_event(q, 5)) for i, s in zip(idx, sims)]


def consolidation_bench(do_cpu):
    """key-frame selection at n = 32 (cfg 1) and n = 3600 (cfg 5, 600 kept), HIP and CPU."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import recipes
    from hippomm_amd.consolidation import select_key_frames_device
    out = {}
    for n, clusters in ((32, 6), (3600, 600)):
        feats = recipes.clustered(n, clusters, 0.2, seed=7)
        dev = torch.from_numpy(feats).cuda()
        kept = select_key_frames_device(dev)
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            kept = select_key_frames_device(dev)          # includes the read-back of the count
            t.append(time.perf_counter() - t0)
        rec = {"kept": int(kept.numel()), "hip_ms": round(sorted(t)[len(t) // 2] * 1e3, 3)}
        if do_cpu:
            from oracle.consolidation_oracle import select_key_frames_oracle
            want = select_key_frames_oracle(feats, None, 0.9)
            tc = []
            with blas_threads():
                for _ in range(3):
                    t0 = time.perf_counter()
                    select_key_frames_oracle(feats, None, 0.9)
                    tc.append(time.perf_counter() - t0)
            rec["cpu_ms"] = round(sorted(tc)[1] * 1e3, 3)
            rec["cpu_cores"] = host_threads()
            rec["kept_equal_oracle"] = kept.cpu().tolist() == want.tolist()
        out[f"n{n}"] = rec
    out["what"] = ("hmm_gram_select vs the numpy oracle (hippocampal_memory.py:944-967 restated) on clustered unit rows; "
                   "hip_ms is the whole call incl. the count read-back, cpu_ms the median of 3")
    return out


def joint_bench():
    """BASELINE configs[2]: vision + audio joint encode, 128 frame / 10 s-spectrogram pairs on one GPU."""
    from hippomm_amd.encoder import HipTower, synthetic_state_dict
    pairs = 128
    sd = synthetic_state_dict(("vision", "audio"), seed=1234)
    vis, aud = HipTower("vision", sd), HipTower("audio", sd)
    del sd
    frames = torch.randn(pairs, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    mels = torch.randn(pairs, 3, 1, 128, 204, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    ev, ea = torch.empty(pairs, 1024, device="cuda"), torch.empty(pairs, 1024, device="cuda")

    def run():
        vis.forward_into(frames, ev)
        aud.forward_into(mels, ea)
    ms = event_time_ms(run, 5, warmup=2)
    flops = vis.flops(pairs) + aud.flops(pairs)
    out = {"workload": "BASELINE cfg3: 128 frame + 10 s log-mel (3 clips) pairs, vision then audio tower",
           "pairs_per_s": round(pairs / ms * 1e3, 1), "ms": round(ms, 3), "tflops": round(flops / ms / 1e9, 1),
           "mfma_frac": round(flops / ms / 1e9 / PEAK_BF16_TFLOPS, 4),
           "tflops_executed": round((vis.flops_executed(pairs) + aud.flops_executed(pairs)) / ms / 1e9, 1),
           "roofline": mfma_roofline(flops, ms, "vision forward + audio forward of 128 pairs, HIP events on the launch stream")}
    del vis, aud
    torch.cuda.empty_cache()
    return out


def call_size_bench():
    """The encoder at the sizes the reference calls it with: the 32-frame buffer of `_process_frame_batch`
    (hippocampal_memory.py:1328; BASELINE configs[0]), one query frame (:2173), one 10-s audio segment (:1222-1225) and one
    question (:2173-2176).  Latency-bound launches: wall clock per forward call, outputs left on the device."""
    from hippomm_amd.encoder import HipTower, synthetic_state_dict
    out = {"what": "wall-clock ms per forward call at the reference's call sizes (median of 5 x 10 calls after 3 warm-up calls)"}
    gen = torch.Generator(device="cuda").manual_seed(5)
    for kind, cases in (("vision", (("frames_32", 32), ("frame_1", 1))), ("audio", (("segment_1", 1),)), ("text", (("question_1", 1),))):
        tower = HipTower(kind, synthetic_state_dict((kind,), seed=1234))
        for tag, b in cases:
            if kind == "vision":
                x = torch.randn(b, 3, 224, 224, device="cuda", generator=gen)
            elif kind == "audio":
                x = torch.randn(b, 3, 1, 128, 204, device="cuda", generator=gen)
            else:
                x = torch.randint(1, 49000, (b, 77), device="cuda", generator=gen)
                x[:, 0], x[:, 20] = 49406, 49407
            emb = torch.empty(b, 1024, device="cuda")
            for _ in range(3):
                tower.forward_into(x, emb)
            torch.cuda.synchronize()
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(10):
                    tower.forward_into(x, emb)
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) / 10 * 1e3)
            ms = sorted(t)[2]
            out[f"{kind}_{tag}_ms"] = round(ms, 3)
            if b > 1:
                out[f"{kind}_{tag}_per_s"] = round(b / ms * 1e3, 1)
                out[f"{kind}_{tag}_roofline"] = mfma_roofline(tower.flops(b), ms, f"one forward call of {b} frames, wall clock incl. launch")
            else:
                # one sample: the bound is the one read of the tower's bf16 weights from HBM, not the matrix cores
                wbytes = float(tower.weight_bytes())
                out[f"{kind}_{tag}_roofline"] = {"bound": "hbm", "scope": "one forward call of 1 sample, wall clock incl. launch",
                                                 "achieved": round(wbytes / ms / 1e6, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                                 "frac": round(wbytes / ms / 1e6 / PEAK_HBM_GBS, 4), "traffic": None,
                                                 "algorithmic_bytes": wbytes, "what": "bf16 matrices of every block + head, read once"}
        del tower
        torch.cuda.empty_cache()
    return out


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def write_synthetic_jpegs(folder: str, n: int, h: int = 720, w: int = 1280, quality: int = 90):
    """n frames of the synthetic video as JPEG files (scene-structured like synthetic_frames: a low-frequency pattern per scene
    of SCENE_LEN frames plus per-frame sensor noise of sigma 4 grey levels), generated on the GPU, encoded by Pillow on the
    host's threads.  Returns (paths in time order, mean file size in bytes)."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from hippomm_amd.preprocess import decode_workers
    g = torch.Generator(device="cuda")
    frames = []
    scene, scene_id = None, -1
    for i in range(n):
        sid = i // SCENE_LEN
        if sid != scene_id:
            g.manual_seed(1000 + sid)
            base = torch.randn(1, 3, 6, 8, generator=g, device="cuda")
            scene = torch.nn.functional.interpolate(base, size=(h, w), mode="bicubic", align_corners=False)[0] * 50.0 + 128.0
            scene_id = sid
        g.manual_seed(7_000_000 + i)
        frame = scene + 4.0 * torch.randn(3, h, w, generator=g, device="cuda")
        frames.append(frame.clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy())
    paths = [os.path.join(folder, f"video_00_{i:05d}.jpg") for i in range(n)]
    with ThreadPoolExecutor(max_workers=min(32, decode_workers())) as pool:
        list(pool.map(lambda a: Image.fromarray(a[0]).save(a[1], quality=quality), zip(frames, paths)))
    return paths, sum(os.path.getsize(p) for p in paths) / n


def formation_bench(do_cpu):
    """The reference's REAL formation call (hippocampal_memory.py:1180-1186, :1328-1335): JPEG paths in, embeddings out on the
    host -- `extract_features({'vision': paths}, ['vision'])['vision'].detach().cpu().numpy()` -- for the 32-frame buffer and for
    256 frames of 1280x720, whole call by wall clock, beside the stages timed alone and the tensor-in forward of the same size."""
    import shutil
    import tempfile
    from hippomm_amd import preprocess as pp
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    folder = tempfile.mkdtemp(prefix="hmm_frames_")
    out = {"what": "extract_features({'vision': [paths]}, ['vision'])['vision'].detach().cpu().numpy() on 1280x720 JPEG files "
                   "(quality 90, synthetic scenes + sensor noise), wall clock of the whole call, median of 7 after 2 warm calls; "
                   "stages: each timed ALONE (median of 3), in the pipeline they overlap",
           "host_threads_decode": pp.decode_workers(), "host_cpu_quota": pp.cpu_quota(),
           "bound": "a range of few frames is latency-bound on the tower (~2.7 ms + 0.29 ms per frame), so a call cut into k ranges costs "
                    "~2.7 (k - 1) ms over the tensor-in forward plus the decode of its first range; the host decodes ~6 frames/ms on its "
                    "threads (one interpreter lock), about 1.8x the tower's rate, which gives 3-4 ranges for 256 frames"}
    try:
        paths, mean_bytes = write_synthetic_jpegs(folder, 256)
        out["jpeg_mean_bytes"] = int(mean_bytes)
        model = ImageBind(state_dict=synthetic_state_dict(("vision",), seed=1234), towers=("vision",))
        tower = model.model.towers["vision"]
        call = lambda ps: model.extract_features({"vision": ps}, ["vision"])["vision"].detach().cpu().numpy()
        one = []
        for _ in range(3):                                        # one frame on one thread: the unit of the decode bound
            t0 = time.perf_counter()
            pp.decode_rgb(paths[:8], workers=1)
            one.append((time.perf_counter() - t0) / 8 * 1e3)
        out["decode_ms_per_frame_one_thread"] = round(_median(one), 3)
        for n in (32, 256):
            ps = paths[:n]
            call(ps); call(ps)
            t, stats = [], {}
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                emb_files = call(ps)
                t.append((time.perf_counter() - t0) * 1e3)
            emb = torch.empty(n, 1024, device="cuda")
            pp.vision_pipeline(ps, "cuda", lambda x, lo, hi: tower.forward_into(x[lo:hi], emb[lo:hi]), stats=stats)
            torch.cuda.synchronize()
            # the stages alone
            load = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x = pp.load_and_transform_vision_data_device(ps, "cuda")      # decode | upload | resize, no tower
                torch.cuda.synchronize()
                load.append((time.perf_counter() - t0) * 1e3)
            dec = []
            for _ in range(3):
                t0 = time.perf_counter()
                frames = pp.decode_rgb(ps)
                dec.append((time.perf_counter() - t0) * 1e3)
            wx, wy, ww, wh = pp.needed_window(720, 1280)
            pinned = torch.empty(n, wh, ww, 3, dtype=torch.uint8, pin_memory=True)
            np_view = pinned.numpy()
            for i, f in enumerate(frames):
                np_view[i] = f[wy:wy + wh, wx:wx + ww]
            del frames
            dev_u8 = torch.empty(n, wh, ww, 3, dtype=torch.uint8, device="cuda")
            h2d_ms = event_time_ms(lambda: dev_u8.copy_(pinned, non_blocking=True), 3, warmup=1)
            resize_ms = event_time_ms(lambda: pp._preprocess_into(dev_u8, x, (720, 1280)), 3, warmup=1)
            fwd_ms = event_time_ms(lambda: tower.forward_into(x, emb), 5, warmup=2)
            same = bool(torch.equal(emb.cpu(), torch.from_numpy(emb_files)))
            d2h = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                emb.detach().cpu().numpy()
                d2h.append((time.perf_counter() - t0) * 1e3)
            ms = _median(t)
            rec = {"ms_end_to_end": round(ms, 3), "frames_per_s": round(n / ms * 1e3, 1),
                   "ms_tensor_in_forward": round(fwd_ms, 3), "frames_per_s_tensor_in": round(n / fwd_ms * 1e3, 1),
                   "ratio_to_tensor_in": round(fwd_ms / ms, 3), "ms_over_tensor_in": round(ms - fwd_ms, 3),
                   "stages_alone_ms": {"files_to_preprocessed_tensors": round(_median(load), 3),
                                       "decode_to_arrays_all_threads": round(_median(dec), 3),
                                       "h2d_pinned_needed_window": round(h2d_ms, 3), "resize_crop_normalise": round(resize_ms, 3),
                                       "forward": round(fwd_ms, 3), "d2h_embeddings": round(_median(d2h), 3)},
                   "pipeline": {"ranges_issued": stats.get("chunks"), "decode_threads": stats.get("workers"),
                                "pinned_ring_frames": stats.get("ring_frames"), "uploaded_window_xywh": list(stats.get("window", ())),
                                "uploaded_bytes_per_frame": int(ww * wh * 3)},
                   "decode_cpu_ms_all_frames": round(n * out["decode_ms_per_frame_one_thread"], 1),
                   "embeddings_equal_tensor_in_forward_bitwise": same}
            out[f"paths_{n}"] = rec
            del pinned, dev_u8, x, emb
        if do_cpu:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from host_vision_pipeline import load_and_transform_vision_data
            load_and_transform_vision_data(paths[:2], "cpu")
            t0 = time.perf_counter()
            ref = load_and_transform_vision_data(paths[:32], "cpu")
            dt = time.perf_counter() - t0
            got = pp.load_and_transform_vision_data_device(paths[:32], "cuda").cpu()
            out["cpu_baseline"] = {"value": round(32 / dt, 1), "unit": "frames/s (files -> normalised (3,224,224) tensors; no encoder)",
                                   "ms_per_frame": round(dt / 32 * 1e3, 2), "cores": 1, "kind": "port",
                                   "sample": "the reference's host chain restated (tests/host_vision_pipeline.py: Pillow decode, BICUBIC "
                                             "resize, centre crop, ToTensor, Normalize) on the first 32 files, one thread as upstream runs it"}
            out["preprocessed_tensors_equal_host_chain_bitwise"] = bool(torch.equal(got, ref))
        del model, tower
    finally:
        shutil.rmtree(folder, ignore_errors=True)
        torch.cuda.empty_cache()
    return out


def audio_bench():
    """The reference's real audio call (hippocampal_memory.py:1219-1225): one 10-second 16 kHz wav path in, one embedding out on the
    host; and 16 files in one call.  Whole call by wall clock, the stages timed alone beside it."""
    import shutil
    import tempfile
    import numpy as np
    from scipy.io import wavfile
    from hippomm_amd import preprocess as pp
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    folder = tempfile.mkdtemp(prefix="hmm_wav_")
    out = {"what": "extract_features({'audio': [wav paths]}, ['audio'])['audio'].detach().cpu().numpy() on 10-second 16 kHz float32 "
                   "wav files (as hippocampal_memory.py:1219 writes them), wall clock of the whole call, median of 15 after 3 warm calls"}
    try:
        rng = np.random.default_rng(11)
        paths = []
        for i in range(16):
            p = os.path.join(folder, f"segment_{i:02d}.wav")
            wavfile.write(p, 16000, (rng.standard_normal(160000) * 0.1).astype(np.float32))
            paths.append(p)
        model = ImageBind(state_dict=synthetic_state_dict(("audio",), seed=1234), towers=("audio",))
        tower = model.model.towers["audio"]
        call = lambda ps: model.extract_features({"audio": ps}, ["audio"])["audio"].detach().cpu().numpy()
        for n in (1, 16):
            ps = paths[:n]
            for _ in range(3):
                call(ps)
            t = []
            for _ in range(15):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(ps)
                t.append((time.perf_counter() - t0) * 1e3)
            rd, sl = [], []
            for _ in range(15):
                t0 = time.perf_counter()
                raw = [pp._read_wav_raw(p) for p in ps]
                rd.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                clips = [d[s:e] for d, _ in raw for s, e in pp.audio_clip_bounds(d.shape[0])]
                buf = np.empty((len(clips), 32000), dtype=np.float32)
                for r, c in enumerate(clips):
                    pp._pcm_to_float(c, buf[r])
                sl.append((time.perf_counter() - t0) * 1e3)
            mel = pp.load_and_transform_audio_data_device(ps, "cuda")
            host_clips = torch.from_numpy(buf).pin_memory()
            dev_clips = torch.empty_like(host_clips, device="cuda")
            h2d_ms = event_time_ms(lambda: dev_clips.copy_(host_clips, non_blocking=True), 20, warmup=3, warm_ms=20.0)
            fbank_ms = event_time_ms(lambda: pp.melspec_clips_device(dev_clips), 20, warmup=3, warm_ms=20.0)
            emb = torch.empty(n, 1024, device="cuda")
            tower_ms = event_time_ms(lambda: tower.forward_into(mel, emb), 20, warmup=3, warm_ms=SCAN_WARM_MS)   # steady clocks, as every sub-ms leg
            load_ms = []
            for _ in range(15):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pp.load_and_transform_audio_data_device(ps, "cuda")
                torch.cuda.synchronize()
                load_ms.append((time.perf_counter() - t0) * 1e3)
            ms = _median(t)
            out[f"wav_{n}"] = {"ms_end_to_end": round(ms, 3), "ms_tower_tensor_in": round(tower_ms, 3),
                               "ms_over_tower": round(ms - tower_ms, 3), "ms_load_data_alone_synced": round(_median(load_ms), 3),
                               "stages_alone_ms": {"wav_read": round(_median(rd), 3), "clip_slicing_into_buffer": round(_median(sl), 3),
                                                   "h2d_pinned": round(h2d_ms, 4), "fbank": round(fbank_ms, 4),
                                                   "tower": round(tower_ms, 3)}}
        del model, tower
    finally:
        shutil.rmtree(folder, ignore_errors=True)
        torch.cuda.empty_cache()
    return out


def encoder_cpu_baseline(frames32: torch.Tensor):
    """the fp32 oracle tower on this host's cores, batch 32 (processing.frame_buffer_size),
    median of 3 passes."""
    from oracle import imagebind_oracle as ib
    threads = host_threads()
    st = ib.synthetic_state(ib.VISION_HUGE, seed=1234, init="fast")
    x = frames32.cpu()
    ib.vision_forward(x[:2], st)
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        ib.vision_forward(x, st)
        times.append(time.perf_counter() - t0)
    dt = sorted(times)[1]
    return {"value": round(x.shape[0] / dt, 2), "unit": "frame-embeddings/s", "cores": threads, "kind": "port",
            "sample": f"fp32 torch-CPU oracle of the same ViT-H/14 tower (32 blocks), batch {x.shape[0]} "
                      f"(processing.frame_buffer_size), median of 3 passes after a 2-frame warm-up, "
                      f"torch intra-op threads = {threads}"}


def encoder_parity(tower_sd, frames, emb, rows=(0, 1, 127, 128, 255)):
    """A few rows of the TIMED batch (both halves of the two-stream split) against the fp32 oracle on the same weights."""
    from oracle import imagebind_oracle as ib
    st = {k: v.detach().float().cpu() for k, v in tower_sd.items()}
    rows = [r for r in rows if r < frames.shape[0]]
    want = ib.vision_forward(frames[rows].cpu(), st)
    got = emb[rows].cpu()
    cos = torch.nn.functional.cosine_similarity(got, want, dim=1)
    return {"rows": rows, "min_cos": round(float(cos.min()), 7), "max_abs_diff": float((got - want).abs().max()),
            "tolerance": "cos >= 1 - 5e-5 and max |diff| <= 2e-3 on unit rows (bf16 operands, fp32 accumulate vs the fp32 oracle)",
            "ok": bool((1 - cos).max() <= 5e-5 and (got - want).abs().max() <= 2e-3)}


def torch_rocm_reference():
    """The same ViT-H/14 tower through stock PyTorch-ROCm operators on this GPU (tools/torch_vit_lib.py): fp32 is what the
    reference runs (ImageBind.forward under no_grad, no autocast, foundation_models.py:116-133), bf16 is the vendor-library
    route.  A reported reference point, never part of the product path."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("torch_vit_probe_lib", os.path.join(ROOT, "tools", "torch_vit_lib.py"))
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    out = {}
    for name, dtype, iters in (("fp32", torch.float32, 2), ("bf16", torch.bfloat16, 4)):
        ms = lib.time_forward(FRAMES_PER_GPU, dtype, iters)
        out[name] = {"ms_per_forward": round(ms, 2), "frames_per_s": round(FRAMES_PER_GPU / ms * 1e3, 1)}
    out["what"] = ("stock PyTorch-ROCm operators (vendor GEMM, scaled_dot_product_attention, layer_norm, gelu), same batch, "
                   "random weights; fp32 = the reference's own execution mode")
    return out


def sharded_scan_bench(rank, world, reduce_max, rows_per_gpu=None, strong=True):
    """The 1M x 1024 scan at N GPUs (north_star: both metrics at 1 / 2 / 4 / 8 GPUs).  The store is row-sharded
    (hippomm_amd.sharding.sharded_top_k): every rank scans its shard, ONE all-gather of k packed keys (8 k bytes)
    and of the row offsets per query, the same merge on every rank.  Two shapes: 1M rows per GPU (weak; the aggregate
    GB/s is the figure that scales) and 1M rows in all (strong; latency-bound from a few GPUs on).  Every rank calls this."""
    from hippomm_amd.sharding import sharded_top_k
    from hippomm_amd.vector_ops import FeatureStore
    q = torch.randn(1024, generator=torch.Generator(device="cuda").manual_seed(43), device="cuda")
    out = {"metric": "cosine-scan GB/s over a row-sharded store (feature_search, 1024-d fp32 rows, top-32, 1 query)",
           "unit": "GB/s", "exchange": "all-gather of 32 packed keys + 1 row offset per rank, merge on every rank"}

    def all_ranks_ok(ok: bool) -> bool:
        """Every rank takes the same path: a rank that failed locally (allocation, a kernel error) tells the others BEFORE
        anybody enters a collective, so nobody waits in an all-gather for a rank that has left."""
        t = torch.tensor([1 if ok else 0], dtype=torch.int32, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    base_rows = rows_per_gpu or SCAN_ROWS                        # tests pass a small store
    legs = (("weak_1M_rows_per_gpu", base_rows),) + ((("strong_1M_rows_total", base_rows // world),) if strong else ())
    for tag, n_local in legs:
        rows = store = None
        err = None
        try:
            g = torch.Generator(device="cuda").manual_seed(1000 + rank)
            rows = torch.empty(n_local, 1024, dtype=torch.float32, device="cuda")
            for s in range(0, n_local, 125_000):
                blk = torch.randn(min(125_000, n_local - s), 1024, generator=g, device="cuda")
                rows[s:s + blk.shape[0]] = blk / blk.norm(dim=1, keepdim=True)
            store = FeatureStore(rows)
            store.search_keys_device(q, SCAN_K)                # the local leg once, outside any collective
            torch.cuda.synchronize()
        except Exception as exc:                               # noqa: BLE001 - reported in the line, and fails the run
            err = f"rank {rank}: {type(exc).__name__}: {exc}"
        if not all_ranks_ok(err is None):
            out[tag] = {"error": err or "another rank failed before the exchange"}
            out["error"] = f"{tag}: {out[tag]['error']}"
            del rows, store
            torch.cuda.empty_cache()
            continue
        offset = rank * n_local
        query = lambda: sharded_top_k(q, SCAN_K, n_local, offset, store.search_keys_device)
        idx, sims = query()
        # parity: torch ranks every shard, the candidates are gathered, and the global order must agree wherever it is separated
        local = torch.topk((rows @ q) / (rows.norm(dim=1) * q.norm()), SCAN_K + 1)
        cand_v = [torch.empty_like(local.values) for _ in range(world)]
        cand_i = [torch.empty_like(local.indices) for _ in range(world)]
        dist.all_gather(cand_v, local.values.contiguous())
        dist.all_gather(cand_i, (local.indices + offset).contiguous())
        best = torch.topk(torch.cat(cand_v), SCAN_K + 1)
        want = torch.cat(cand_i)[best.indices]
        gap = best.values[:-1] - best.values[1:]                 # gap[i] = value i - value i+1, i = 0 .. SCAN_K-1
        below = gap[:SCAN_K] > 2e-6
        above = torch.cat([torch.ones(1, dtype=torch.bool, device=gap.device), gap[:SCAN_K - 1] > 2e-6])
        separated = below & above                                # a rank is pinned only when BOTH neighbours are clear of it
        ok = bool(idx.numel() == SCAN_K and torch.equal(idx[separated], want[:SCAN_K][separated]))
        dist.barrier()
        # steady state by COUNT, not by time: `query` holds a collective, and a time-based warm-up would let the ranks leave it
        # after different numbers of calls -- mismatched all-gathers, i.e. a hang
        ms = reduce_max(event_time_ms(query, 50, warmup=80))
        total = float(n_local) * world * 4096.0
        out[tag] = {"rows_per_gpu": n_local, "ms_per_query": round(ms, 4), "GBps_all_gpus": round(total / ms / 1e6, 1),
                    "frac_of_n_gpus_x_8TBps": round(total / ms / 1e6 / (PEAK_HBM_GBS * world), 4),
                    "indices_match_torch_where_separated": ok}
        del rows, store, local
        torch.cuda.empty_cache()
    out["value"] = out["weak_1M_rows_per_gpu"].get("GBps_all_gpus")
    return out


# ------------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--workload", choices=("cfg2", "cfg5"), default="cfg2")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-scan", action="store_true")
    ap.add_argument("--cfg5-frames", type=int, default=CFG5_FRAMES,
                    help="cfg5: frames of the synthetic video (default 3600 = BASELINE cfg 5; other values exercise ragged shards)")
    ap.add_argument("--scan-strong", action="store_true",
                    help="N > 1: also time the scan with 1M rows in ALL (strong scaling); default is the weak leg only")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the count read-back step, roofline and kernel table, all-gather alone, scan and "
                         "the other N = 1 legs, CPU baselines and the oracle checks (--no-scan / --no-cpu-baseline / "
                         "--scan-strong shape this part)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/*.npy (see dump_outputs)")
    args = ap.parse_args()
    t_start = time.perf_counter()
    if args.steps is None:
        args.steps = 10 if args.workload == "cfg2" else 2
    if args.warmup is None:
        args.warmup = 3 if args.workload == "cfg2" else 1
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "RANK" not in os.environ:          # self-launch; this process never initialises the GPU
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a line for the wrong N",
              file=sys.stderr)
        sys.exit(2)
    if world > 1 and REHEARSAL:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    elif world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world,
                                device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(0)
    n_gpus = world

    from hippomm_amd.consolidation import select_key_frames_async
    from hippomm_amd.encoder import HipTower, synthetic_state_dict
    from hippomm_amd.sharding import all_gather_embeddings, shard_bounds

    sd = synthetic_state_dict(("vision",), seed=1234)
    tower = HipTower("vision", sd)
    extras = args.full and rank == 0 and n_gpus == 1 and args.workload == "cfg2"
    if not (extras and not args.no_cpu_baseline):
        sd = None
    torch.cuda.empty_cache()

    if args.workload == "cfg2":
        n_total = FRAMES_PER_GPU * world
        bounds = [(r * FRAMES_PER_GPU, (r + 1) * FRAMES_PER_GPU) for r in range(world)]
    else:
        n_total = args.cfg5_frames
        bounds = shard_bounds(n_total, world)
    lo, hi = bounds[rank]
    counts = [b - a for a, b in bounds]
    frames = synthetic_frames(lo, hi, "cuda")
    emb = torch.empty(hi - lo, 1024, dtype=torch.float32, device="cuda")

    def encode(x):
        for s in range(0, x.shape[0], FRAMES_PER_GPU):
            tower.forward_into(x[s:s + FRAMES_PER_GPU], emb[s:s + FRAMES_PER_GPU])
        return emb

    # launch-only until the final sync of the timed region: the selection returns (kept buffer, count) on the device
    step = make_step(frames, counts, encode, all_gather_embeddings, select_key_frames_async)

    def reduce_max(x):
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    startup_s = time.perf_counter() - t_start                  # imports excluded; weights, frames, process group included
    elapsed, (feats, (kept_buf, n_kept)) = timed_steps(step, args.steps, args.warmup, torch.cuda.synchronize,
                                                       (dist.barrier if world > 1 else (lambda: None)), reduce_max)
    kept = kept_buf[: int(n_kept.item())].clone()
    if rank == 0 and args.dump_outputs:                        # before anything else reuses the step's buffers
        dump_outputs(args.dump_outputs, feats, kept)
    elapsed_rb = None
    if args.full:
        # The timed step is launch-only (selection result left on the device; the last step's list is read after the timer).
        # Rounds 1-2 read the kept count back inside every step: the same K steps with that read-back, for comparison.
        def step_with_readback():
            f, (kb, nk) = step()
            return f, kb[: int(nk.item())]
        elapsed_rb, _ = timed_steps(step_with_readback, args.steps, 1, torch.cuda.synchronize,
                                    (dist.barrier if world > 1 else (lambda: None)), reduce_max)

    proof = rank_proof(world, rank, local_rank, hi - lo) if world > 1 else None

    gather_ms = None
    sharded_scan = None
    if world > 1 and args.full:                                # the exchange step alone
        gather_ms = reduce_max(event_time_ms(lambda: all_gather_embeddings(emb, counts), 20, warmup=3))
        if not args.no_scan:
            # rank-local failures are agreed on inside (all_ranks_ok) before any collective; what still raises here raises on
            # every rank alike.  Either way the line carries scan.error and the run exits non-zero.
            try:
                sharded_scan = sharded_scan_bench(rank, world, reduce_max, strong=args.scan_strong)
            except Exception as exc:                           # noqa: BLE001
                sharded_scan = {"error": f"{type(exc).__name__}: {exc}"}

    if rank == 0:
        value = n_total * args.steps / elapsed
        ms_step = elapsed / args.steps * 1e3
        enc_flops = sum(tower.flops(c) for c in counts if c > 0)                   # whole job, nominal
        enc_flops_exec = sum(tower.flops_executed(c) for c in counts if c > 0)
        line = {
            "metric": "frame-embeddings/sec (ImageBind-huge ViT-H/14 vision tower; scan GB/s under 'scan')",
            "value": round(value, 1), "unit": "frame-embeddings/s", "n_gpus": n_gpus, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True,
            "scaling": "weak" if args.workload == "cfg2" else "strong", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic",
            "timed_step": "launch-only: encode -> (all-gather) -> selection, result left on the device, one sync after K steps",
            "startup_s": round(startup_s, 2),
        }
        if elapsed_rb is not None:
            line["ms_per_step_with_count_readback"] = round(elapsed_rb / args.steps * 1e3, 3)
            line["value_with_count_readback"] = round(n_total * args.steps / elapsed_rb, 1)
        if args.workload == "cfg2":
            line["config"] = {"workload": "BASELINE cfg2: ViT-H/14 vision encoder (32 blocks, 257 tokens, D=1280), 256 "
                                          "synthetic 224x224 frames per GPU per step (scenes of 6 frames), random-init "
                                          "weights; step = encode -> (N>1: RCCL all-gather of embeddings) -> cosine "
                                          "key-frame selection",
                              "frames_per_gpu": FRAMES_PER_GPU, "sharding": f"frames x{n_gpus}",
                              "kept_key_frames": int(kept.numel()), "of_frames": int(feats.shape[0])}
        else:
            line["config"] = {"workload": f"BASELINE cfg5: 1-hour video at 1 fps = {n_total} synthetic frames (scenes of 6), "
                                          "contiguous time shards of ceil(3600/N) frames per rank -> encode -> ONE RCCL "
                                          "all-gather of the (n_local,1024) fp32 embeddings -> global cosine key-frame "
                                          "selection on every rank",
                              "frames_total": n_total, "frames_per_rank": counts, "sharding": f"time shards x{n_gpus}",
                              "kept_key_frames": int(kept.numel()),
                              "all_gather_bytes_per_rank": max(counts) * 4096}
            if args.full:
                from oracle.consolidation_oracle import select_key_frames_oracle
                want = select_key_frames_oracle(feats.cpu().numpy(), None, 0.9)
                line["config"].update({
                    "kept_equal_cpu_oracle_on_gathered_matrix": kept.cpu().tolist() == want.tolist(),
                    # fingerprints: the same at every N (time shards + bitwise batch invariance of the tower)
                    "gathered_embeddings_sha256": hashlib.sha256(feats.cpu().numpy().tobytes()).hexdigest(),
                    "kept_indices_sha256": hashlib.sha256(kept.cpu().numpy().tobytes()).hexdigest()})
        if gather_ms is not None:
            line["config"]["all_gather_ms"] = round(gather_ms, 4)
        if proof is not None:
            line["rccl_ranks"] = proof["all_reduced_rank_count"] if proof["backend"] == "nccl" else None
            line["collective_backend"] = ("nccl (RCCL)" if proof["backend"] == "nccl" else proof["backend"])
            line["all_reduced_rank_count"] = proof["all_reduced_rank_count"]
            if proof["backend"] == "nccl":                      # the library behind backend "nccl" on ROCm is RCCL
                try:
                    line["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
                except Exception as exc:                        # noqa: BLE001
                    line["rccl_version"] = f"unavailable: {exc}"
                line["rccl_env"] = {k: v for k, v in os.environ.items() if k.startswith(("NCCL_", "RCCL_", "HSA_ENABLE_IPC"))}
            line["ranks"] = proof["ranks"]
            n1 = committed_n1_value(args.workload)
            if n1 is not None and not REHEARSAL:
                line["scaling_vs_n1"] = {"n1_value": n1["value"], "n1_source": n1["source"],
                                         "ratio": round(value / n1["value"], 3),
                                         "note": "this run's whole-job value / the committed 1-GPU value of the same workload"}
        line["step_tflops"] = round(enc_flops * args.steps / elapsed / 1e12, 1)
        line["step_mfma_frac"] = round(enc_flops * args.steps / elapsed / 1e12 / PEAK_BF16_TFLOPS, 4)
        line["flops_per_frame_nominal"] = tower.flops(1)
        line["flops_per_frame_executed"] = round(tower.flops_executed(FRAMES_PER_GPU) / FRAMES_PER_GPU, 1)
        line["step_tflops_executed"] = round(enc_flops_exec * args.steps / elapsed / 1e12, 1)
        line["step_mfma_frac_executed"] = round(enc_flops_exec * args.steps / elapsed / 1e12 / PEAK_BF16_TFLOPS, 4)
        line["step_mfma_frac_note"] = ("step_mfma_frac credits the reference's nominal FLOPs (SURVEY 8d: un-folded patch conv, full last "
                                       "block); step_mfma_frac_executed counts only what this build runs; roofline.frac is ONE kernel "
                                       "(the dominant GEMM) on its own 2MNK")
        if args.full:
            roof, table = gemm_roofline(FRAMES_PER_GPU)
            line["roofline"], line["kernels"] = roof, table
            line["kernels_note"] = ("NOT additive: each kernel of one block is timed between its own HIP events in ONE full-batch "
                                    "chain (event gaps included), while the timed step runs two half-batch chains that overlap on "
                                    "the chip; 32 x the column sums to more than ms_per_step")
        if sharded_scan is not None:
            line["scan"] = sharded_scan
        if REHEARSAL:
            line["rehearsal"] = "HMM_BENCH_REHEARSAL=1: all ranks on cuda:0 over gloo -- code-path check only, NOT a measurement"
        if extras:
            if sd is not None:
                line["parity_vs_oracle"] = encoder_parity(sd, frames, emb)
                sd = None
            frames32 = frames[:32].clone()
            del tower, frames, emb
            torch.cuda.empty_cache()
            if not args.no_scan:
                line["scan"] = scan_bench(do_cpu=not args.no_cpu_baseline)
                line["joint_vision_audio"] = joint_bench()
                line["reference_call_sizes"] = call_size_bench()
                line["consolidation"] = consolidation_bench(do_cpu=not args.no_cpu_baseline)
                line["formation_from_files"] = formation_bench(do_cpu=not args.no_cpu_baseline)
                line["audio_from_wav"] = audio_bench()
            if not args.no_cpu_baseline:
                line["torch_rocm_reference"] = torch_rocm_reference()
                line["cpu_baseline"] = encoder_cpu_baseline(frames32)
        print(json.dumps(line), flush=True)
        bad = [k for k in ("parity_vs_oracle",) if k in line and not line[k].get("ok", True)]
        if "scan" in line and "error" in line["scan"]:      # a missing second metric is a failed run, not a shorter line
            bad.append("scan.error")
        if args.workload == "cfg5" and not line["config"].get("kept_equal_cpu_oracle_on_gathered_matrix", True):
            bad.append("cfg5.kept_equal_cpu_oracle_on_gathered_matrix")
        if proof is not None and proof["all_reduced_rank_count"] != world:
            bad.append("all_reduced_rank_count")
        if "scan" in line and not line["scan"].get("parity_vs_oracle", {}).get("top32_indices_equal", True):
            bad.append("scan.parity_vs_oracle")
        if "scan" in line and not line["scan"].get("prefilter_bf16_shadow", {}).get("identical_to_fp32_scan", True):
            bad.append("scan.prefilter_bf16_shadow")
        rp = line.get("scan", {}).get("retrieval", {}).get("parity_vs_oracle")
        if rp and not (rp["top5_of_first_200_events_equal"] and 1 - rp["text_embedding_cos"] <= 5e-5):
            bad.append("scan.retrieval.parity_vs_oracle")
        if not line.get("scan", {}).get("retrieval", {}).get("prefilter_identical_to_fp32_scan", True) or \
                not line.get("scan", {}).get("retrieval", {}).get("prefilter_hits_equal", True):
            bad.append("scan.retrieval.prefilter")
        for tag in ("weak_1M_rows_per_gpu", "strong_1M_rows_total"):
            if "scan" in line and not line["scan"].get(tag, {}).get("indices_match_torch_where_separated", True):
                bad.append(f"scan.{tag}")
        if bad:                                            # a fast wrong answer is not a result
            print(f"bench.py: parity check failed: {bad}", file=sys.stderr)
            sys.exit(4)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
