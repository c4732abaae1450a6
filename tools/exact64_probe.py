"""The float64 route (exact64=True) against the fp32 exact routes on one MI355X, alternating in one process.

    python tools/exact64_probe.py                      # -> profiles/exact64.json
    python tools/exact64_probe.py --kernel-loop 20     # only 20 flat float64 calls: the workload of a kernel trace
                                                       # (rocprofv3 --kernel-trace --stats -- python tools/exact64_probe.py --kernel-loop 20)
    python tools/exact64_probe.py --kernel-stats FILE  # fold the trace's kernel_stats.csv into profiles/exact64.json

Workloads: the flat call at 1M x 1024, k = 32; the per-event call on bench.py's question store (2000 events x 500 rows, the same
4.1 GB buffer), k = 5; relevant_hits end to end (host query, read-back, rules).  The fp32 sides are the default routes, which
this route leaves untouched: the same kernels and bits as before it existed.  A call is timed on the wall clock between two device
synchronisations; five alternating rounds, per round and side 60 ms of the same calls and then 20 timed calls, the median round.
Register counts are the compiler's (-Rpass-analysis=kernel-resource-usage), read off the build.  Not part of bench.py; nothing
depends on these numbers."""
from __future__ import annotations

import csv
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
EVENTS, PER_EVENT, K_FLAT, K_EVENT, KEEP = 2000, 500, 32, 5, 5
WARM_MS, ROUNDS, ITERS = 60.0, 5, 20
OUT = ROOT / "profiles" / "exact64.json"
# hipcc -Rpass-analysis=kernel-resource-usage on hippomm_amd/csrc/cosine_topk_f64.hip (gfx950): VGPRs, scratch bytes per lane
REGISTERS = {"scan_sims_f64_kernel<fp32 query>": {"vgprs": 92, "scratch_bytes": 0, "occupancy_waves_per_simd": 5},
             "scan_sims_f64_kernel<fp64 query>": {"vgprs": 92, "scratch_bytes": 0, "occupancy_waves_per_simd": 5},
             "select_f64_kernel<argmax>": {"vgprs": 64, "scratch_bytes": 0, "lds_bytes": 256},
             "select_f64_kernel<lds chunks>": {"vgprs": 24, "scratch_bytes": 0, "lds_bytes": 24576},
             "rows_f64_are_f32_kernel": {"vgprs": 16, "scratch_bytes": 0}}


def _store():
    import torch
    from hippomm_amd.vector_ops import EventStore
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    rows = torch.randn(EVENTS * PER_EVENT, 1024, generator=g, device="cuda", dtype=torch.float32)
    rows /= rows.norm(dim=1, keepdim=True)
    query = torch.randn(1024, generator=g, device="cuda", dtype=torch.float32)
    return EventStore.from_device_rows(rows, [PER_EVENT] * EVENTS), query


def _alternate(sides):
    import torch
    got = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < WARM_MS:
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                fn()
            torch.cuda.synchronize()
            got[name].append((time.perf_counter() - t0) * 1e3 / ITERS)
    return {name: {"rounds_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4)} for name, v in got.items()}


def measure():
    import numpy as np
    es, q = _store()
    q_host = q.cpu().numpy()
    n = len(es)
    i32, v32 = es.search_device(q, K_FLAT)
    i64, v64 = es.search_device(q, K_FLAT, exact64=True)
    out = {"workload": {"rows": n, "events": EVENTS, "rows_per_event": PER_EVENT, "k_flat": K_FLAT, "k_per_event": K_EVENT,
                        "keep": KEEP, "store_bytes": n * 4096},
           "method": f"wall clock between device synchronisations; {ROUNDS} alternating rounds, per round and side {WARM_MS:.0f} ms "
                     f"of the same calls and then {ITERS} timed calls, median round; the fp32 sides are the default routes, "
                     f"unchanged by this route",
           "flat_same_rows_as_fp32": bool(i32.tolist() == i64.tolist()),
           "flat_max_abs_difference_to_fp32": float((v64 - v32.double()).abs().max()),
           "flat_1M_k32_device_query": _alternate({
               "fp32_search_device": lambda: es.search_device(q, K_FLAT),
               "f64_search_device": lambda: es.search_device(q, K_FLAT, exact64=True)}),
           "per_event_2000x500_k5_device_query": _alternate({
               "fp32_search_segments_device": lambda: es.search_segments_device(q, es.offsets, K_EVENT),
               "f64_search_segments_device": lambda: es.search_segments_device(q, es.offsets, K_EVENT, exact64=True)}),
           "relevant_hits_end_to_end_host_query": _alternate({
               "fp32_relevant_hits": lambda: es.relevant_hits(q_host, K_EVENT, KEEP),
               "f64_relevant_hits": lambda: es.relevant_hits(q_host, K_EVENT, KEEP, exact64=True)}),
           "registers": REGISTERS}
    flat = out["flat_1M_k32_device_query"]
    for side in flat:
        flat[side]["whole_call_GBps"] = round(n * 4096 / (flat[side]["median_ms"] * 1e-3) / 1e9, 1)
    OUT.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


def kernel_loop(calls: int):
    import torch
    es, q = _store()
    for _ in range(calls):
        es.search_device(q, K_FLAT, exact64=True)
        es.search_device(q, K_FLAT)
    torch.cuda.synchronize()


def fold_kernel_stats(path: str):
    """Average kernel times of the trace -> profiles/exact64.json["kernel_trace"], with the streaming kernels' GB/s."""
    out = json.loads(OUT.read_text())
    rows = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name") or r.get("KernelName") or ""
            if "scan_sims_f64" in name or "select_f64" in name or "scan_topk_kernel" in name or "topk_final" in name:
                rows[name.split("(")[0][:120]] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2)}
    bytes_read = out["workload"]["store_bytes"]
    for name, r in rows.items():
        if "scan_sims_f64" in name or "scan_topk_kernel" in name:
            r["GBps"] = round(bytes_read / (r["average_us"] * 1e-6) / 1e9, 1)
    out["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "kernels": rows}
    OUT.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["kernel_trace"], indent=1))


if __name__ == "__main__":
    if "--kernel-loop" in sys.argv:
        kernel_loop(int(sys.argv[sys.argv.index("--kernel-loop") + 1]))
    elif "--kernel-stats" in sys.argv:
        fold_kernel_stats(sys.argv[sys.argv.index("--kernel-stats") + 1])
    else:
        measure()
