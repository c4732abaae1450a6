"""The batched float64 route (exact64=True on the ``_multi`` calls) against Q single float64 calls and against the fp32 batched
default on one MI355X, alternating in one process.

    python tools/exact64_multi_probe.py                      # -> profiles/exact64_multi.json
    python tools/exact64_multi_probe.py --kernel-loop 20     # only 20 flat float64 calls of 16 questions: the workload of a kernel trace
                                                             # (rocprofv3 --kernel-trace --stats --output-format csv -d DIR --
                                                             #  python tools/exact64_multi_probe.py --kernel-loop 20), a run of its own
    python tools/exact64_multi_probe.py --kernel-stats FILE  # fold the trace's kernel_stats.csv into profiles/exact64_multi.json

Workloads, each for Q = 1, 4 and 16 questions that lie on the device: the per-event call on bench.py's question store (2000 events
x 500 rows, 4.1 GB), k = 5; the per-event call on a 3600-row store in 36 events, k = 5; the flat call at 1M x 1024, k = 32.  Sides:
the batched float64 call; Q calls of the single float64 route (tools/exact64_probe.py measures one of them); the fp32 batched
default, which this route leaves untouched.  A side is timed on the wall clock between two device synchronisations; five
alternating rounds, per round and side 60 ms of the same calls and then 20 timed calls, the median round.  Register counts are the
compiler's (-Rpass-analysis=kernel-resource-usage), read off the build.  Not part of bench.py; nothing depends on these numbers."""
from __future__ import annotations

import csv
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
EVENTS, PER_EVENT, K_FLAT, K_EVENT = 2000, 500, 32, 5
SMALL_EVENTS, SMALL_PER_EVENT = 36, 100
BATCHES = (1, 4, 16)
WARM_MS, ROUNDS, ITERS = 60.0, 5, 20
OUT = ROOT / "profiles" / "exact64_multi.json"
# hipcc -Rpass-analysis=kernel-resource-usage on hippomm_amd/csrc/cosine_topk_f64.hip (gfx950); LDS is dynamic: 128 B + 4 KiB (fp32)
# or 8 KiB (fp64) per question of the pass
REGISTERS = {"scan_sims_f64_multi_kernel<fp32 queries>": {"vgprs": 186, "agprs": 0, "scratch_bytes": 0, "occupancy_waves_per_simd": 2,
                                                          "lds_bytes_at_16_questions": 65664},
             "scan_sims_f64_multi_kernel<fp64 queries>": {"vgprs": 218, "agprs": 0, "scratch_bytes": 0, "occupancy_waves_per_simd": 2,
                                                          "lds_bytes_at_16_questions": 131200}}


def _stores():
    import torch
    from hippomm_amd.vector_ops import EventStore
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    rows = torch.randn(EVENTS * PER_EVENT, 1024, generator=g, device="cuda", dtype=torch.float32)
    rows /= rows.norm(dim=1, keepdim=True)
    queries = torch.randn(max(BATCHES), 1024, generator=g, device="cuda", dtype=torch.float32)
    big = EventStore.from_device_rows(rows, [PER_EVENT] * EVENTS)
    small = EventStore.from_device_rows(rows[: SMALL_EVENTS * SMALL_PER_EVENT].clone(), [SMALL_PER_EVENT] * SMALL_EVENTS)
    return big, small, queries


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


def _per_event_sides(es, q):
    def singles():
        for i in range(q.shape[0]):
            es.search_segments_device(q[i], es.offsets, K_EVENT, exact64=True)
    return {"f64_batched": lambda: es.search_segments_multi_device(q, es.offsets, K_EVENT, exact64=True),
            "f64_single_calls": singles,
            "fp32_batched": lambda: es.search_segments_multi_device(q, es.offsets, K_EVENT)}


def _flat_sides(es, q):
    def singles():
        for i in range(q.shape[0]):
            es.search_device(q[i], K_FLAT, exact64=True)
    return {"f64_batched": lambda: es.search_multi_device(q, K_FLAT, exact64=True),
            "f64_single_calls": singles,
            "fp32_batched": lambda: es.search_multi_device(q, K_FLAT)}


def _same_bits(es, q):
    import torch
    idx, sims, _ = es.search_segments_multi_device(q, es.offsets, K_EVENT, exact64=True)
    ok = True
    for i in range(q.shape[0]):
        i1, s1, _ = es.search_segments_device(q[i], es.offsets, K_EVENT, exact64=True)
        ok = ok and bool(torch.equal(idx[i], i1)) and bool(torch.equal(sims[i].view(torch.int64), s1.view(torch.int64)))
    return ok


def measure():
    big, small, queries = _stores()
    out = {"workload": {"rows": len(big), "events": EVENTS, "rows_per_event": PER_EVENT, "small_rows": len(small),
                        "small_events": SMALL_EVENTS, "k_flat": K_FLAT, "k_per_event": K_EVENT, "store_bytes": len(big) * 4096,
                        "questions": list(BATCHES), "queries": "fp32, on the device (the kernel forms the norms)"},
           "method": f"wall clock between device synchronisations; {ROUNDS} alternating rounds, per round and side {WARM_MS:.0f} ms "
                     f"of the same calls and then {ITERS} timed calls, median round; a side answers all Q questions once per call "
                     f"(f64_single_calls: Q calls of the single float64 route); the fp32 side is the default batched route, unchanged",
           "batched_bits_equal_single_calls_per_event_16": _same_bits(big, queries),
           "registers": REGISTERS}
    for name, es, sides in (("per_event_2000x500_k5", big, _per_event_sides), ("per_event_36x100_k5", small, _per_event_sides),
                            ("flat_1M_k32", big, _flat_sides)):
        out[name] = {}
        for Q in BATCHES:
            got = _alternate(sides(es, queries[:Q]))
            got["single_calls_over_batched"] = round(got["f64_single_calls"]["median_ms"] / got["f64_batched"]["median_ms"], 2)
            got["batched_over_fp32_batched"] = round(got["f64_batched"]["median_ms"] / got["fp32_batched"]["median_ms"], 2)
            out[name][f"Q={Q}"] = got
    OUT.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


def kernel_loop(calls: int):
    import torch
    big, _, queries = _stores()
    for _ in range(calls):
        big.search_multi_device(queries, K_FLAT, exact64=True)
    torch.cuda.synchronize()


def fold_kernel_stats(path: str):
    """Average kernel times of the trace -> profiles/exact64_multi.json["kernel_trace"], with the scan kernel's row rate."""
    out = json.loads(OUT.read_text())
    rows = {}
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r.get("Name") or r.get("KernelName") or ""
            if "scan_sims_f64" in name or "select_f64" in name:
                rows[name.split("(")[0][:120]] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2)}
    for name, r in rows.items():
        if "scan_sims_f64_multi" in name:                        # one pass over the store for 16 questions
            r["row_rate_GBps"] = round(out["workload"]["store_bytes"] / (r["average_us"] * 1e-6) / 1e9, 1)
    out["kernel_trace"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own: 20 flat calls of 16 questions", "kernels": rows}
    OUT.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["kernel_trace"], indent=1))


if __name__ == "__main__":
    if "--kernel-loop" in sys.argv:
        kernel_loop(int(sys.argv[sys.argv.index("--kernel-loop") + 1]))
    elif "--kernel-stats" in sys.argv:
        fold_kernel_stats(sys.argv[sys.argv.index("--kernel-stats") + 1])
    else:
        measure()
