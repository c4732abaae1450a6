"""The batched scans through the bf16 shadow against the exact batched scans on one MI355X, 16 questions, in one process.

    python tools/multi_prefilter_probe.py [--out profiles/multi_prefilter.json]

(a) flat, 1M x 1024 rows, k = 32: search_multi_device without and with the shadow (hmm_cosine_topk_multi against
    hmm_cosine_topk_multi_prefilter);
(b) per event, bench.py's question store, 2000 events x 500 rows, k = 5, keep = 5: top_hits_multi without and with `prefilter`
    (wall clock with the read-back) and the device side alone (search_segments_multi_device);
(c) both at a small store, 20 000 rows (per event: 40 events x 500), where the dispatch limits sit;
(d) the `stats` of each shadow run.
Method: steady state (60 ms of the same calls first), the two sides alternating in one session: five rounds per side, a HIP event
recorded every 10 calls, the median group of 10 per side over all rounds.  The exact side is the baseline of the same session."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
NQ, WARM_MS, ROUNDS, GROUPS, GROUP = 16, 60.0, 5, 4, 10


def _warm(fn, ms):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()


def _alternate(sides):
    """sides: name -> fn.  Per round and side GROUPS groups of GROUP calls, an event between groups; ms per call of the median group."""
    import torch
    for fn in sides.values():
        _warm(fn, WARM_MS)
    got = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(GROUPS + 1)]
            ev[0].record()
            for g in range(GROUPS):
                for _ in range(GROUP):
                    fn()
                ev[g + 1].record()
            torch.cuda.synchronize()
            got[name] += [ev[g].elapsed_time(ev[g + 1]) / GROUP for g in range(GROUPS)]
    return {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for name, v in got.items()}


def _wall(sides, calls=9):
    import torch
    got = {name: [] for name in sides}
    for fn in sides.values():
        _warm(fn, WARM_MS)
    for _ in range(calls):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            got[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": round(statistics.median(v), 4)} for name, v in got.items()}


def _ratio(r, exact, shadow):
    r["shadow_over_exact"] = round(r[shadow]["median_ms"] / r[exact]["median_ms"], 3)
    r["shadow_at_least_5_percent_faster"] = bool(r[shadow]["median_ms"] <= 0.95 * r[exact]["median_ms"])
    return r


def flat(n, k):
    import torch
    from hippomm_amd.vector_ops import FeatureStore
    g = torch.Generator(device="cuda").manual_seed(11)
    rows = torch.empty(n, 1024, device="cuda")
    for s in range(0, n, 100_000):
        rows[s:s + 100_000] = torch.randn(min(100_000, n - s), 1024, generator=g, device="cuda")
    queries = torch.randn(NQ, 1024, generator=g, device="cuda")
    fs = FeatureStore(rows).build_shadow()
    stats = torch.full((NQ, 2), -7, dtype=torch.int32, device="cuda")
    i0, s0 = (t.clone() for t in fs.search_multi_device(queries, k, prefilter=False))
    i1, s1 = fs.search_multi_device(queries, k, prefilter=True, stats=stats)
    same = bool(torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32)))
    r = _alternate({"exact": lambda: fs.search_multi_device(queries, k, prefilter=False),
                    "shadow": lambda: fs.search_multi_device(queries, k, prefilter=True)})
    r.update(rows=n, k=k, identical=same, stats_candidates=stats[:, 0].tolist(), stats_saturated=stats[:, 1].tolist())
    return _ratio(r, "exact", "shadow")


def per_event(events, per_event_rows, k, keep):
    import torch
    from hippomm_amd.vector_ops import EventStore
    g = torch.Generator(device="cuda").manual_seed(11)
    rows = torch.randn(events * per_event_rows, 1024, generator=g, device="cuda", dtype=torch.float32)
    rows /= rows.norm(dim=1, keepdim=True)
    queries = torch.randn(NQ, 1024, generator=g, device="cuda", dtype=torch.float32)
    es = EventStore.from_device_rows(rows, [per_event_rows] * events)
    es.build_shadow()
    stats = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    a = [t.clone() for t in es.search_segments_multi_device(queries, es.offsets, k)]
    b = es.search_segments_multi_device(queries, es.offsets, k, prefilter=True, stats=stats)
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2]))
    r = _alternate({"exact": lambda: es.search_segments_multi_device(queries, es.offsets, k),
                    "shadow": lambda: es.search_segments_multi_device(queries, es.offsets, k, prefilter=True)})
    r.update(events=events, rows_per_event=per_event_rows, k=k, keep=keep, identical=same, stats_whole_events=int(stats[0]),
             stats_rows_rescored=int(stats[1]))
    r["top_hits_multi_wall"] = _ratio(_wall({"exact": lambda: es.top_hits_multi(queries, k, keep),
                                             "shadow": lambda: es.top_hits_multi(queries, k, keep, prefilter=True)}), "exact", "shadow")
    return _ratio(r, "exact", "shadow")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "multi_prefilter.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"queries": NQ,
           "method": f"HIP events every {GROUP} calls, {WARM_MS:.0f} ms of the same calls first, {ROUNDS} alternating rounds of {GROUPS} groups, "
                     "median group; the exact side is the same session's baseline"}
    out["flat_1m_k32"] = flat(1_000_000, 32)
    torch.cuda.empty_cache()
    out["per_event_2000x500_k5"] = per_event(2000, 500, 5, 5)
    torch.cuda.empty_cache()
    out["flat_20000_k32"] = flat(20_000, 32)
    out["per_event_40x500_k5"] = per_event(40, 500, 5, 5)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
