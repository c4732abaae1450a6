"""Where does the time of recall_window_frames go?

    python tools/recall_windows_probe.py [--out profiles/recall_windows.json] [--windows 15] [--frames 3] [--reps 5]

Frames: the synthetic video of bench.py's write_synthetic_jpegs (tools/jpeg_encode_probe.frames) at 1920x1080, as BGR host arrays
-- what cap.read() hands to the loop at hippocampal_memory.py:2226-2249 --, 15 windows of 3 consecutive frames by default (five
segments of three frame_times).  The stages of the call are run one by one, each ending with a device synchronisation, then the
whole call; host wall-clock milliseconds, median of `reps` after one warm round.

Absolute times only.  There is no fair host baseline on a machine without OpenCV (the numpy oracle of the tests is not what
anyone runs), and in a question the caller's video seeks and the captioner dominate: nothing in the package or its tests depends
on these numbers."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

W, H = 1920, 1080


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def _summary(values):
    return {"median_ms": round(float(np.median(values)), 3), "min_ms": round(float(min(values)), 3),
            "max_ms": round(float(max(values)), 3), "all_ms": [round(float(v), 3) for v in values]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recall_windows.json"))
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from PIL import Image
    from jpeg_encode_probe import frames as synthetic
    from hippomm_amd import _lib, jpeg, recall_window_frames, segmentation as seg, ssim
    dev = _lib.require_gpu()
    n = a.windows * a.frames
    host = list(synthetic(W, H, n).flip(-1).contiguous().cpu().numpy())      # BGR, on the host
    windows = [[(float(k), host[w * a.frames + k]) for k in range(a.frames)] for w in range(a.windows)]
    pairs = np.array([(w * a.frames + i, w * a.frames + j) for w in range(a.windows) for i in range(a.frames)
                      for j in range(i + 1, a.frames)], dtype=np.int32)
    legs = {k: [] for k in ("upload", "resize", "encode_with_decoded", "gray_minmax", "ssim_pairs", "read_back", "walk", "whole_call")}
    kept = None
    for rep in range(a.reps + 1):
        row = {}
        row["upload"], up = _timed(lambda: ssim.upload_frames(host, dev))
        row["resize"], small = _timed(lambda: seg.resize_frames(up, seg.RECALL_SIZE))
        row["encode_with_decoded"], (files, decoded) = _timed(
            lambda: jpeg.encode_jpeg(small, quality=seg.SAVE_QUALITY, subsampling=seg.SAVE_SUBSAMPLING, channel_order="BGR",
                                     return_decoded=True))
        row["gray_minmax"], (gray, minmax) = _timed(lambda: seg.gray_frames(decoded, "RGB", return_minmax=True))
        row["ssim_pairs"], scores = _timed(lambda: ssim.ssim_launch(gray, pairs, -1.0, minmax))
        row["read_back"], scores = _timed(lambda: scores.cpu().numpy())
        per = a.frames * (a.frames - 1) // 2

        def walk():
            out = []
            for w in range(a.windows):
                table = np.full((a.frames, a.frames), np.nan)
                table[np.triu_indices(a.frames, 1)] = scores[w * per:(w + 1) * per]
                out.append(seg.walk_recall_window(table))
            return out

        row["walk"], by_stage = _timed(walk)
        row["whole_call"], got = _timed(lambda: recall_window_frames(windows))
        assert got.kept == by_stage and got.all_segment_files == [files[w * a.frames + i] for w, ks in enumerate(by_stage) for i in ks]
        kept = got.kept
        if rep:                                                              # the first round warms allocator, tables and checks
            for k in legs:
                legs[k].append(row[k])
    result = {"pillow": Image.__version__, "device": torch.cuda.get_device_name(0), "source": f"{W}x{H}", "target": "320x180",
              "windows": a.windows, "frames_per_window": a.frames, "pairs": int(len(pairs)), "reps": a.reps,
              "frames_kept": int(sum(len(k) for k in kept)), "encode_stats": jpeg.encode_stats(),
              "note": "host wall clock per stage, each ending with a device synchronisation; one warm round dropped; absolute "
                      "times only, no host baseline exists here",
              "stages": {k: _summary(v) for k, v in legs.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({k: v["median_ms"] for k, v in result["stages"].items()}), flush=True)


if __name__ == "__main__":
    main()
