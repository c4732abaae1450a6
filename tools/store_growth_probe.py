"""What keeping a resident EventStore current costs on one MI355X, against rebuilding it, in one process.

    python tools/store_growth_probe.py [--out profiles/store_growth.json]

(a) a store of 1M x 1024 rows (2000 events x 500 rows) with a bf16 shadow gains one event of 500 rows:
      append   EventStore.append_event of a device tensor (hmm_store_ingest_rows: the new rows and their shadow rows, one launch,
               one small offsets upload), wall clock per call with the device drained, and the device side alone;
      rebuild  what had to be done before: EventStore(host list of all events) + build_shadow(), wall clock with the device drained.
    The two sides alternate in one session; the rebuild is the same session's baseline.
(b) the two kernels as copies: bytes read plus bytes written per second of hmm_store_ingest_rows (fp32 and fp64 sources, with and
    without the shadow) and of hmm_store_gather_segments (with and without the shadow) on 262 144 rows, set beside the measured
    float4-copy rate of this part, 6.29 TB/s.
Method: every figure is the median of its repetitions; device times are HIP events around groups of calls after a warm-up of the
same calls."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
EVENTS, PER_EVENT, ROUNDS, APPENDS = 2000, 500, 3, 20
COPY_ROWS, COPY_REPS, FLOAT4_COPY_TBPS = 262_144, 7, 6.29


def _event_ms(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def growth():
    import torch
    from hippomm_amd.vector_ops import EventStore
    g = torch.Generator(device="cuda").manual_seed(5)
    n = EVENTS * PER_EVENT
    rows = torch.empty(n, 1024, device="cuda")
    for s in range(0, n, 100_000):
        rows[s:s + 100_000] = torch.randn(min(100_000, n - s), 1024, generator=g, device="cuda")
    host = rows.cpu().numpy()
    events = [host[e * PER_EVENT: (e + 1) * PER_EVENT] for e in range(EVENTS)]          # the host list a rebuild starts from
    new = [torch.randn(PER_EVENT, 1024, generator=g, device="cuda") for _ in range(4)]
    store = EventStore.from_device_rows(rows, [PER_EVENT] * EVENTS)
    store.reserve(n + (ROUNDS + 1) * (APPENDS + 1) * PER_EVENT)
    del rows
    store.build_shadow()
    torch.cuda.synchronize()
    wall, dev, rebuild = [], [], []
    for i in range(APPENDS):                                                             # warm-up: pinned staging, code objects
        store.append_event(new[i % 4])
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for i in range(APPENDS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store.append_event(new[i % 4])
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        lib_rows = len(store)
        dev.append(_event_ms(lambda: _ingest_only(store, new[0], lib_rows), APPENDS))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fresh = EventStore(events).build_shadow()
        torch.cuda.synchronize()
        rebuild.append((time.perf_counter() - t0) * 1e3)
        del fresh
        torch.cuda.empty_cache()
    out = {"rows": n, "events": EVENTS, "new_event_rows": PER_EVENT,
           "append_event_wall_ms": {"median": round(statistics.median(wall), 4), "min": round(min(wall), 4), "max": round(max(wall), 4)},
           "append_ingest_device_ms": {"median": round(statistics.median(dev), 5)},
           "rebuild_wall_ms": {"median": round(statistics.median(rebuild), 1), "min": round(min(rebuild), 1), "max": round(max(rebuild), 1)}}
    out["rebuild_over_append"] = round(out["rebuild_wall_ms"]["median"] / out["append_event_wall_ms"]["median"], 1)
    # the grown store answers as a rebuilt one does (bits), checked once outside the timing
    q = torch.randn(1024, generator=g, device="cuda")
    extra = [t.cpu().numpy() for t in new]
    fresh = EventStore(events + [extra[i % 4] for i in range((ROUNDS + 1) * APPENDS)])
    a, b = store.search_segments_device(q, store.offsets, 5, prefilter=True), fresh.search_segments_device(q, fresh.offsets, 5)
    out["identical_to_rebuilt"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and
                                       torch.equal(store.rows.view(torch.int32), fresh.rows.view(torch.int32)))
    return out


def _ingest_only(store, src, at):
    """The launch of an append alone, into the spare capacity (the same rows every time: the store does not grow)."""
    from hippomm_amd import _lib as L
    L.check(L.load().hmm_store_ingest_rows(src.data_ptr(), 0, src.shape[0], 1024, store._buf.data_ptr(), store._shadow_buf.data_ptr(),
                                           store._buf.shape[0], at, L.stream_ptr()), "hmm_store_ingest_rows")


def copies():
    import numpy as np
    import torch
    from hippomm_amd import _lib as L
    lib = L.load()
    n = COPY_ROWS
    g = torch.Generator(device="cuda").manual_seed(6)
    src32 = torch.randn(n, 1024, generator=g, device="cuda")
    src64 = src32.double()
    dst = torch.empty(n, 1024, device="cuda")
    shadow = torch.empty(n * 2048, dtype=torch.uint8, device="cuda")
    src_shadow = torch.empty(n * 2048, dtype=torch.uint8, device="cuda")
    L.check(lib.hmm_shadow_store_build(src32.data_ptr(), n, 1024, src_shadow.data_ptr(), src_shadow.numel(), L.stream_ptr()), "shadow")
    seg_rows = 512
    offsets = torch.arange(0, n + 1, seg_rows, dtype=torch.int64, device="cuda")
    n_seg = n // seg_rows
    order = torch.from_numpy(np.random.default_rng(7).permutation(n_seg).astype(np.int32)).to("cuda")

    def ingest(src, dtype, sh):
        return lambda: L.check(lib.hmm_store_ingest_rows(src.data_ptr(), dtype, n, 1024, dst.data_ptr(), sh.data_ptr() if sh is not None else None,
                                                         n, 0, L.stream_ptr()), "hmm_store_ingest_rows")

    def gather(sh):
        return lambda: L.check(lib.hmm_store_gather_segments(src32.data_ptr(), src_shadow.data_ptr() if sh else None, n, offsets.data_ptr(), n_seg,
                                                             order.data_ptr(), offsets.data_ptr(), n_seg, 1024, dst.data_ptr(),
                                                             shadow.data_ptr() if sh else None, n, n, L.stream_ptr()), "hmm_store_gather_segments")

    cases = {"ingest_fp32_with_shadow": (ingest(src32, 0, shadow), 4096 + 4096 + 2048),
             "ingest_fp32": (ingest(src32, 0, None), 4096 + 4096),
             "ingest_fp64_with_shadow": (ingest(src64, 1, shadow), 8192 + 4096 + 2048),
             "ingest_fp64": (ingest(src64, 1, None), 8192 + 4096),
             "gather_with_shadow": (gather(True), 2 * (4096 + 2048)),
             "gather": (gather(False), 2 * 4096)}
    out = {"rows": n, "float4_copy_tb_per_s": FLOAT4_COPY_TBPS}
    for name, (fn, bytes_per_row) in cases.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = statistics.median(_event_ms(fn, 5) for _ in range(COPY_REPS))
        tbps = n * bytes_per_row / (ms * 1e-3) / 1e12
        out[name] = {"median_ms": round(ms, 4), "bytes_per_row": bytes_per_row, "tb_per_s": round(tbps, 3),
                     "of_float4_copy": round(tbps / FLOAT4_COPY_TBPS, 3)}
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "store_growth.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"method": f"append: wall clock per call with the device drained, {ROUNDS} rounds of {APPENDS} calls alternating with one rebuild each, "
                     f"medians; copies: HIP events around 5 calls, median of {COPY_REPS}; bytes = read + written"}
    out["copies_262144_rows"] = copies()
    torch.cuda.empty_cache()
    out["append_vs_rebuild_1m_rows"] = growth()
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
