"""Retrieval with the reference's row and fallback rules on one MI355X: what a question costs by each of the three routes, in
one process.

    python tools/relevant_hits_probe.py        # -> profiles/relevant_hits.json

Workload: bench.py's question store, 2000 events x 500 rows x 1024 fp32 (4.1 GB), k = 5, keep = 5, row_limits = one sixth of each
event's rows (the reference's consolidation ratio), no deferral.  The sides, alternating in one session:
  (a) top_k_per_event + the row rule and the ranking in Python  -- the only route to the reference's answer before
      EventStore.relevant_hits;
  (b) relevant_hits                                             -- the rules and the ranking on the device;
  (c) top_hits                                                  -- ranks every hit: fast, but not the reference's set.
and the same for 16 questions through the _multi forms.  Every call ends with its read-back, so a call is timed on the wall
clock between two device synchronisations; steady state as bench.py's event_time_ms asks for it: five alternating rounds,
in each round and for each side 60 ms of the same calls and then 20 timed calls (side (a) is mostly Python: without the warm-up
the device would have idled before the next side), the median round of each side.  Not part of bench.py; no threshold depends on it.
"""
from __future__ import annotations

import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

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


def _rule_in_python(per_event, limits, keep):
    """The row rule and the global stable sort, as a caller of top_k_per_event has to write them."""
    entries = [(float(s), e, int(i)) for e, (idx, sims) in enumerate(per_event) for i, s in zip(idx, sims) if i < limits[e]]
    entries.sort(key=lambda x: x[0], reverse=True)
    return [(e, i, s) for s, e, i in entries[:keep]]


def _warm(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < WARM_MS:
        fn()


def _alternate(sides):
    import torch
    got = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            _warm(fn)                                            # before EVERY timed group: the side before may have been host-bound
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                fn()
            torch.cuda.synchronize()
            got[name].append((time.perf_counter() - t0) * 1e3 / ITERS)
    return {name: {"rounds_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4)} for name, v in got.items()}


def measure():
    es, queries = _store()
    q = queries[0].clone()
    limits = [PER_EVENT // 6] * EVENTS
    limits_np = np.asarray(limits, np.int64)                     # kept beside the store by a caller, as the Python side keeps its list
    want = _rule_in_python(es.top_k_per_event(q, K), limits, KEEP)
    got = es.relevant_hits(q, K, KEEP, row_limits=limits_np)[0]
    want_multi = [_rule_in_python(p, limits, KEEP) for p in es.top_k_per_event_multi(queries, K)]
    got_multi = [h for h, _ in es.relevant_hits_multi(queries, K, KEEP, row_limits=limits_np)]
    top = es.top_hits(q, K, KEEP)
    out = {"workload": {"events": EVENTS, "rows_per_event": PER_EVENT, "k": K, "keep": KEEP, "row_limit": PER_EVENT // 6,
                        "queries_multi": NQ, "store_bytes": EVENTS * PER_EVENT * 4096},
           "method": f"wall clock between device synchronisations, read-back included; {ROUNDS} alternating rounds, per round and side "
                     f"{WARM_MS:.0f} ms of the same calls and then {ITERS} timed calls, median round",
           "relevant_hits_equals_the_rule_in_python": bool(got == want and got_multi == want_multi),
           "top_hits_returns_the_same_five": bool([(e, r) for e, r, _ in top] == [(e, r) for e, r, _ in want]),
           "one_question": _alternate({
               "a_top_k_per_event_plus_python_rule": lambda: _rule_in_python(es.top_k_per_event(q, K), limits, KEEP),
               "b_relevant_hits": lambda: es.relevant_hits(q, K, KEEP, row_limits=limits_np),
               "c_top_hits": lambda: es.top_hits(q, K, KEEP)}),
           "sixteen_questions": _alternate({
               "a_top_k_per_event_multi_plus_python_rule": lambda: [_rule_in_python(p, limits, KEEP)
                                                                    for p in es.top_k_per_event_multi(queries, K)],
               "b_relevant_hits_multi": lambda: es.relevant_hits_multi(queries, K, KEEP, row_limits=limits_np),
               "c_top_hits_multi": lambda: es.top_hits_multi(queries, K, KEEP)})}
    (ROOT / "profiles" / "relevant_hits.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    measure()
