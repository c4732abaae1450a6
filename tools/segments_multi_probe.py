"""Batched per-event retrieval on one MI355X: 16 questions through one pass (hmm_cosine_topk_segmented_multi,
hmm_rank_segment_hits_multi) against the same work as 16 single-question calls, in one process.

    python tools/segments_multi_probe.py time        # -> profiles/segments_multi.json
    python tools/segments_multi_probe.py kernels     # workload for `rocprofv3 --kernel-trace --stats` (a run of its own)

Workload: bench.py's question store, 2000 events x 500 rows x 1024 fp32 (4.1 GB), k = 5, keep = 5, 16 questions, fp32 path.
time: HIP events on the launch stream, steady state (60 ms of the same calls first), the two sides alternating: five rounds of
(20 x loop of 16 search_segments_device | 20 x one search_segments_multi_device), the median round of each side; the same for the
batched whole-store scan (search_multi_device, no per-event selection: the difference is what the selection costs) and, end to end
with the read-back, 16 top_hits calls against one top_hits_multi call (wall clock, synchronised).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
EVENTS, PER_EVENT, K, KEEP, NQ = 2000, 500, 5, 5, 16
WARM_MS, ROUNDS, ITERS = 60.0, 5, 20


def _store():
    import torch
    from hippomm_amd.vector_ops import EventStore
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    rows = torch.randn(EVENTS * PER_EVENT, 1024, generator=g, device="cuda", dtype=torch.float32)
    rows /= rows.norm(dim=1, keepdim=True)
    queries = torch.randn(NQ, 1024, generator=g, device="cuda", dtype=torch.float32)
    return EventStore.from_device_rows(rows, [PER_EVENT] * EVENTS), queries


def _warm(fn, ms):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()


def _alternate(sides, iters=ITERS, rounds=ROUNDS):
    """sides: name -> fn.  Every round times `iters` back-to-back calls of each side in turn; per side the rounds and their median (ms per call)."""
    import torch
    for fn in sides.values():
        _warm(fn, WARM_MS)
    got = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            got[name].append(e0.elapsed_time(e1) / iters)
    return {name: {"rounds_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4)} for name, v in got.items()}


def _wall(sides, calls=9):
    import torch
    got = {name: [] for name in sides}
    for fn in sides.values():
        fn()
    for _ in range(calls):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            got[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"calls_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4)} for name, v in got.items()}


def measure():
    import torch
    es, queries = _store()
    qs = [queries[i].clone() for i in range(NQ)]

    def loop():
        for q in qs:
            es.search_segments_device(q, es.offsets, K)

    def batched():
        es.search_segments_multi_device(queries, es.offsets, K)

    def whole_store():
        es.search_multi_device(queries, K)

    # the two ways must name the same rows before anything is timed
    idx, sims, counts = es.search_segments_multi_device(queries, es.offsets, K)
    same_rows = all(torch.equal(idx[i], es.search_segments_device(qs[i], es.offsets, K)[0]) for i in range(NQ))
    out = {"workload": {"events": EVENTS, "rows_per_event": PER_EVENT, "k": K, "keep": KEEP, "queries": NQ,
                        "store_bytes": EVENTS * PER_EVENT * 4096},
           "method": f"HIP events, {WARM_MS:.0f} ms of the same calls first, {ROUNDS} alternating rounds of {ITERS} calls, median round",
           "same_rows_as_16_single_calls": bool(same_rows)}
    out["scan"] = _alternate({"loop_of_16_search_segments_device": loop, "search_segments_multi_device": batched,
                              "search_multi_device_whole_store": whole_store})
    a, b, c = (out["scan"][n]["median_ms"] for n in ("loop_of_16_search_segments_device", "search_segments_multi_device",
                                                     "search_multi_device_whole_store"))
    out["scan"]["loop_over_batched"] = round(a / b, 2)
    out["scan"]["batched_within_a_quarter_of_the_loop"] = bool(b <= a / 4)
    out["scan"]["per_event_selection_price_ms"] = round(b - c, 4)
    out["end_to_end"] = _wall({"16_top_hits": lambda: [es.top_hits(q, K, KEEP) for q in qs],
                               "top_hits_multi": lambda: es.top_hits_multi(queries, K, KEEP)})
    out["end_to_end"]["loop_over_batched"] = round(out["end_to_end"]["16_top_hits"]["median_ms"] /
                                                   out["end_to_end"]["top_hits_multi"]["median_ms"], 2)
    (ROOT / "profiles" / "segments_multi.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


def kernels():
    import torch
    es, queries = _store()
    for _ in range(23):
        es.search_segments_multi_device(queries, es.offsets, K)
        es.search_multi_device(queries, K)
        es.search_segments_device(queries[0], es.offsets, K)
    torch.cuda.synchronize()
    print("kernels: 23 x (search_segments_multi_device, search_multi_device, search_segments_device)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "kernels"])
    a = ap.parse_args()
    measure() if a.mode == "time" else kernels()
