"""save_event with the feature matrices written on the host against written on the device, in one session on one GPU.

    python tools/event_json_probe.py [--out profiles/event_json_device.json] [--reps 5]

For an event with one (600, 1024) and one (3600, 1024) fp32 vision matrix (ten minutes and an hour of video at 1 fps), each held
as a numpy array and as a device tensor:
  * save_event(..., matrices="host")   -- the call as it was before the device route existed (a device tensor is read back to
                                          numpy first, which is what a caller had to do), and
  * save_event(..., matrices="device"),
both without sidecars (they are the same work on both routes) and, once, with them; then the device route taken apart: upload
(numpy only), the three kernels alone (device events around hmm_json_write_matrix_device), the two read-backs, the splice
(event_json_bytes minus matrix_json_bytes) and the file write.  Times are wall-clock milliseconds ending in a device
synchronise, minimum and median of --reps runs after one warm-up; the files of both routes are compared byte for byte."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

import probe_common  # noqa: F401  (puts the repository on sys.path)
import torch

from hippomm_amd import _lib, event_store as es


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(out), 3), "median_ms": round(statistics.median(out), 3)}


def event_of(vision):
    rows = vision.shape[0]
    return dict(features={"vision": vision, "vision_times": np.arange(rows, dtype=np.float64)}, frames=[f"frames/v/{i:06d}.jpg" for i in range(0, rows, 30)],
                frame_times=[float(i) for i in range(0, rows, 30)], frame_captions=["a caption"] * len(range(0, rows, 30)), audio_times=[0.0, float(rows)],
                audio_transcription=[{"text": "hello there", "start": 0.2, "end": 1.1}], holistic_audio_transcription=[], summary="A summary.",
                start_time=0.0, end_time=float(rows))


def kernels_alone(m, reps):
    lib = _lib.load()
    rows, cols = m.shape
    cap = lib.hmm_json_matrix_text_bound(rows, cols, 4)
    ws_bytes = lib.hmm_json_write_matrix_device_workspace_bytes(rows, cols)
    out = torch.empty(cap, dtype=torch.uint8, device=m.device)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=m.device)
    written = torch.empty(1, dtype=torch.int64, device=m.device)

    def call():
        _lib.check(lib.hmm_json_write_matrix_device(m.data_ptr(), 0, rows, cols, 4, out.data_ptr(), cap, written.data_ptr(), ws.data_ptr(), ws_bytes,
                                                    _lib.stream_ptr()), "hmm_json_write_matrix_device")
    ms = sorted(probe_common.event_ms(call, 10) for _ in range(reps))
    n = int(written.item())
    pinned = torch.empty(n, dtype=torch.uint8, pin_memory=True)

    def read_back():
        int(written.item())
        pinned.copy_(out[:n], non_blocking=True)
    return {"kernels_ms": {"min_ms": round(ms[0], 4), "median_ms": round(statistics.median(ms), 4)}, "text_bytes": n,
            "read_back": timed(read_back, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(probe_common.ROOT) / "profiles" / "event_json_device.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    rng = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(dev), "reps": a.reps, "unit": "ms, wall clock ending in a device synchronise", "shapes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for rows in (600, 3600):
            v = rng.standard_normal((rows, 1024)).astype(np.float32)
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            on_device = torch.from_numpy(v).to(dev)
            entry = {}
            for source, vision in (("numpy", v), ("device_tensor", on_device)):
                event = event_of(vision)
                host_event = lambda: event_of(vision.cpu().numpy()) if source == "device_tensor" else event      # noqa: E731
                r = {"save_event_host": timed(lambda: es.save_event(host_event(), tmp / "h.json", write_sidecars=False), a.reps),
                     "save_event_device": timed(lambda: es.save_event(event, tmp / "d.json", write_sidecars=False, matrices="device"), a.reps)}
                assert (tmp / "h.json").read_bytes() == (tmp / "d.json").read_bytes()
                r["save_event_host_with_sidecars"] = timed(lambda: es.save_event(host_event(), tmp / "h.json"), 2)
                r["save_event_device_with_sidecars"] = timed(lambda: es.save_event(event, tmp / "d.json", matrices="device"), 2)
                stats = {}
                r["matrix_json_bytes"] = timed(lambda: es.matrix_json_bytes(vision, 4, stats=stats), a.reps)
                r["event_json_bytes"] = timed(lambda: es.event_json_bytes(event), a.reps)
                r["route"] = stats["route"]
                r["splice_ms"] = round(r["event_json_bytes"]["median_ms"] - r["matrix_json_bytes"]["median_ms"], 3)
                data = es.event_json_bytes(event)
                r["file_write"] = timed(lambda: (tmp / "w.json").write_bytes(data), a.reps)
                r["file_bytes"] = len(data)
                if source == "numpy":
                    r["upload"] = timed(lambda: torch.from_numpy(v).to(dev), a.reps)
                r["speedup_median"] = round(r["save_event_host"]["median_ms"] / r["save_event_device"]["median_ms"], 2)
                entry[source] = r
            entry["device_call_alone"] = kernels_alone(on_device, a.reps)
            result["shapes"][f"{rows}x1024_fp32"] = entry
    result["matrix_json_stats"] = es.matrix_json_stats()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    sys.exit(main())
