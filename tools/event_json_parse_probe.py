"""parse_event_features with the feature matrices converted on the host against converted on the device, in one session on one GPU.

    python tools/event_json_parse_probe.py [--out profiles/event_json_parse.json] [--find-out profiles/event_json_find.json] [--reps 5]
                                           [--find-only]

For an event file with one (600, 1024) and one with a (3600, 1024) fp32-origin vision matrix (ten minutes and an hour of video at
1 fps), written by save_event without sidecars:
  * parse_event_features(path)                       -- the call as it was before the device route existed (native=True), and
  * parse_event_features(path, matrices="device"),
alternating, one warm round first, median and minimum of --reps; the results are compared as bits.  Then the device route taken
apart: the file read, hmm_json_find_matrices, the upload of the text through pinned staging, the three kernels alone (device events
around hmm_json_parse_matrix_device) and the read-back of the report; the kernels' text bytes per second stand beside the float4
copy rate DESIGN.md quotes.  Times are wall-clock milliseconds ending in a device synchronise.

The span finder is a stage of its own, written to --find-out: parse_event_features(matrices="device") with find="host" against
find="device", alternating in the same session, one warm round first, medians of --reps, the results compared as bits; then
hmm_json_find_matrices on the host beside the eight kernels of hmm_json_find_matrices_device alone (device events) and
find_matrices_device on the uploaded text (launches, one read-back).  --find-only skips everything else and leaves --out alone."""
import argparse
import ctypes as C
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

import probe_common
import torch

from hippomm_amd import _lib, event_store as es

FLOAT4_COPY_TBS = 6.29               # the measured float4 copy of this part


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3)}


def timed(fn, reps):
    fn()
    return summary([wall(fn)[0] for _ in range(reps)])


def stages(path, dev, reps):
    lib = _lib.load()
    raw = path.read_bytes()
    spans = (C.c_size_t * 4 * 16)()
    n = C.c_int(0)

    def find():
        _lib.check(lib.hmm_json_find_matrices(raw, len(raw), es.NATIVE_MIN_VALUES, C.cast(spans, C.c_void_p), 16, C.byref(n)), "hmm_json_find_matrices")
    find()
    begin, end, rows, cols = (int(v) for v in spans[0])
    text = es._EventText(raw, dev)

    def upload():
        text.tensor = None
        with es._device_lock:
            text.on_device()
    out = torch.empty((rows, cols), dtype=torch.float32, device=dev)
    ws_bytes = lib.hmm_json_parse_matrix_device_workspace_bytes(end - begin)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    report = torch.empty(4 + 4 * es.FLAGGED_CAP, dtype=torch.int64, device=dev)
    upload()
    t = text.tensor

    def call():
        _lib.check(lib.hmm_json_parse_matrix_device(t.data_ptr(), begin, end, rows, cols, 0, out.data_ptr(), report.data_ptr(), report.data_ptr() + 32,
                                                    es.FLAGGED_CAP, ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "hmm_json_parse_matrix_device")
    kernels = sorted(probe_common.event_ms(call, 10) for _ in range(reps))
    pinned = torch.empty(report.numel(), dtype=torch.int64, pin_memory=True)
    median_ms = statistics.median(kernels)
    return {"file_bytes": len(raw), "span_bytes": end - begin, "rows": rows, "cols": cols,
            "file_read": timed(lambda: path.read_bytes(), reps), "find_matrices": timed(find, reps), "upload": timed(upload, reps),
            "kernels_ms": {"min_ms": round(kernels[0], 4), "median_ms": round(median_ms, 4)},
            "kernels_text_TBs": round((end - begin) / (median_ms * 1e-3) / 1e12, 4), "float4_copy_TBs_quoted": FLOAT4_COPY_TBS,
            "report_read_back": timed(lambda: pinned.copy_(report, non_blocking=True), reps)}


def find_stage(path, dev, reps):
    lib = _lib.load()
    raw = path.read_bytes()
    host_find = lambda: es.parse_event_features(path, matrices="device", device=dev, find="host")       # noqa: E731
    device_find = lambda: es.parse_event_features(path, matrices="device", device=dev, find="device")   # noqa: E731
    want, got = host_find()[0]["vision"], device_find()[0]["vision"]                                      # the warm round
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    host_ms, device_ms = [], []
    for _ in range(reps):                                                                                 # alternating
        host_ms.append(wall(host_find)[0])
        device_ms.append(wall(device_find)[0])
    spans = (C.c_size_t * 4 * 16)()
    n = C.c_int(0)

    def find():
        _lib.check(lib.hmm_json_find_matrices(raw, len(raw), es.NATIVE_MIN_VALUES, C.cast(spans, C.c_void_p), 16, C.byref(n)), "hmm_json_find_matrices")
    t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    out = torch.empty(4 + 4 * 16, dtype=torch.int64, device=dev)
    ws_bytes = lib.hmm_json_find_matrices_device_workspace_bytes(len(raw))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)

    def call():
        _lib.check(lib.hmm_json_find_matrices_device(t.data_ptr(), len(raw), es.NATIVE_MIN_VALUES, out.data_ptr() + 32, 16, out.data_ptr(), ws.data_ptr(),
                                                     ws_bytes, _lib.stream_ptr()), "hmm_json_find_matrices_device")
    kernels = sorted(probe_common.event_ms(call, 10) for _ in range(reps))
    find()
    assert out[:4].tolist()[0] == n.value and out[4:8].tolist() == [int(v) for v in spans[0]]
    median_ms = statistics.median(kernels)
    entry = {"file_bytes": len(raw), "workspace_bytes": ws_bytes,
             "parse_event_features_find_host": summary(host_ms), "parse_event_features_find_device": summary(device_ms),
             "host_find_matrices": timed(find, reps), "device_find_kernels_ms": {"min_ms": round(kernels[0], 4), "median_ms": round(median_ms, 4)},
             "device_find_kernels_text_TBs": round(len(raw) / (median_ms * 1e-3) / 1e12, 4),
             "find_matrices_device_on_uploaded_text": timed(lambda: es.find_matrices_device(t), reps)}
    entry["speedup_median"] = round(entry["parse_event_features_find_host"]["median_ms"] / entry["parse_event_features_find_device"]["median_ms"], 2)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(probe_common.ROOT) / "profiles" / "event_json_parse.json"))
    ap.add_argument("--find-out", default=str(Path(probe_common.ROOT) / "profiles" / "event_json_find.json"))
    ap.add_argument("--find-only", action="store_true", help="measure the span finder alone; --out is not written")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    rng = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "unit": "ms, wall clock ending in a device synchronise", "shapes": {}}
    found = {"device": result["device"], "reps": a.reps, "unit": result["unit"], "shapes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for rows in (600, 3600):
            v = rng.standard_normal((rows, 1024)).astype(np.float32)
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            path = es.save_event({"features": {"vision": v, "vision_times": np.arange(rows, dtype=np.float64)}, "summary": "A summary."},
                                 Path(tmp) / f"e{rows}.json", write_sidecars=False)
            found["shapes"][f"{rows}x1024_fp32"] = find_stage(path, dev, a.reps)
            if a.find_only:
                continue
            host = lambda: es.parse_event_features(path)                                      # noqa: E731
            device = lambda: es.parse_event_features(path, matrices="device", device=dev)     # noqa: E731
            want, got = host()[0]["vision"], device()[0]["vision"]                            # the warm round
            assert got.cpu().numpy().tobytes() == want.tobytes() == v.tobytes()
            host_ms, device_ms = [], []
            for _ in range(a.reps):                                                           # alternating
                host_ms.append(wall(host)[0])
                device_ms.append(wall(device)[0])
            entry = {"parse_event_features_host": summary(host_ms), "parse_event_features_device": summary(device_ms)}
            entry["speedup_median"] = round(entry["parse_event_features_host"]["median_ms"] / entry["parse_event_features_device"]["median_ms"], 2)
            entry["device_route_stages"] = stages(path, dev, a.reps)
            entry["find_matrices_share_of_device_route"] = round(entry["device_route_stages"]["find_matrices"]["median_ms"]
                                                                 / entry["parse_event_features_device"]["median_ms"], 3)
            result["shapes"][f"{rows}x1024_fp32"] = entry
    found["matrix_find_stats"] = es.matrix_find_stats()
    Path(a.find_out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.find_out).write_text(json.dumps(found, indent=1) + "\n")
    print(json.dumps(found, indent=1))
    if a.find_only:
        return 0
    result["matrix_parse_stats"] = es.matrix_parse_stats()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    sys.exit(main())
