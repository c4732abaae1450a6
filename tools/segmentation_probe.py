"""SSIM / segmentation measurements on one MI355X (hippomm_amd/segmentation.py).

    python tools/segmentation_probe.py kernels --pairs N       # workload for `rocprofv3 --kernel-trace --stats` (a run of its own)
    python tools/segmentation_probe.py summarize --stats A --pairs N [--stats B --pairs M]   # A: kernel_stats.csv or results.db
    python tools/segmentation_probe.py calls                   # the drop-ins end to end, no profiler

kernels: N consecutive 1080p pairs through hmm_ssim_pairs (range of frame a), 20 times after a warm-up.  summarize: per-pair
kernel time from the stats CSVs against both floors -- bytes (2 H W per pair at 6.3 TB/s) and the fp64 operations of the formula
(78.6 TFLOP/s, the spec FP64 vector rate) -- written to profiles/segmentation_kernels.json.  calls: compute_frame_difference on two
1080p BGR arrays (upload included), _compute_frame_similarity on a 1080p JPEG pair (cold cache and warm), segment_sequence over
600 synthetic 1080p JPEG frames at 1 fps in a "cuts" and a "static" regime, and the numpy oracle's CPU time per 1080p pair (a
stand-in for skimage, which this environment cannot run on the GPU host) -> profiles/segmentation_calls.json.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
H, W = 1080, 1920
HBM = 6.3e12
FP64 = 78.6e12
# fp64 operations per window position as written (int -> double conversions not counted, a division counted as one): five
# divisions by 49, three variances (mul, sub, mul), A1 (mul, mul, add), A2 (mul, add), B1 (mul, mul, add, add), B2 (add, add),
# A1 A2, B1 B2, the division, the running sum
FLOP_PER_POSITION = 5 + 9 + 3 + 2 + 4 + 2 + 1 + 1 + 1 + 1


def kernels(n_pairs: int):
    import torch
    from hippomm_amd.ssim import gray_into, ssim_launch
    torch.cuda.set_device(0)
    g = torch.randint(0, 256, (n_pairs + 1, H, W), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    mm = torch.empty((n_pairs + 1, 2), dtype=torch.int32, device="cuda")
    gray_into(g, 2, None, mm)
    pairs = np.array([[i + 1, i] for i in range(n_pairs)], np.int32)
    for _ in range(3):
        ssim_launch(g, pairs, -1.0, mm)
    torch.cuda.synchronize()
    for _ in range(20):
        ssim_launch(g, pairs, -1.0, mm)
    torch.cuda.synchronize()
    print(f"kernels: {n_pairs} pairs x 23 calls")


def _kernel_stats(path, kernel):
    """Calls / TotalDurationNs / AverageNs of the kernels whose name contains `kernel`: from a `--stats` CSV, or from the rocpd
    database (results.db) that rocprofv3 writes when no output format is given."""
    if str(path).endswith(".db"):
        import sqlite3
        calls, total = sqlite3.connect(path).execute(
            "select count(*), sum(end - start) from kernels where name like ?", (f"%{kernel}%",)).fetchone()
        return {"Calls": calls, "TotalDurationNs": total, "AverageNs": total / calls}
    rows = [r for r in csv.DictReader(open(path)) if kernel in r["Name"]]
    calls, total = sum(int(r["Calls"]) for r in rows), sum(float(r["TotalDurationNs"]) for r in rows)
    return {"Calls": calls, "TotalDurationNs": total, "AverageNs": total / calls}


def summarize(stats, pairs):
    out = {"frame": [H, W], "calls_per_run": 23, "hbm_bytes_per_s": HBM, "fp64_flop_per_s": FP64,
           "fp64_flop_per_position": FLOP_PER_POSITION, "runs": {}}
    positions = (H - 6) * (W - 6)
    for path, n in zip(stats, pairs):
        tile, fin = _kernel_stats(path, "ssim_tile_kernel"), _kernel_stats(path, "ssim_finish_kernel")
        ns = float(tile["TotalDurationNs"]) + float(fin["TotalDurationNs"])
        per_call_us = ns / 23 / 1e3
        per_pair_us = per_call_us / n
        bytes_floor = 2 * H * W / HBM * 1e6
        flop_floor = positions * FLOP_PER_POSITION / FP64 * 1e6
        out["runs"][f"{n}_pairs"] = {
            "pairs": n, "tile_kernel_calls": int(tile["Calls"]), "finish_kernel_calls": int(fin["Calls"]),
            "tile_kernel_avg_us": float(tile["AverageNs"]) / 1e3, "finish_kernel_avg_us": float(fin["AverageNs"]) / 1e3,
            "kernel_us_per_call": per_call_us, "kernel_us_per_pair": per_pair_us,
            "floor_bytes_us_per_pair": bytes_floor, "floor_fp64_us_per_pair": flop_floor,
            "binding_floor": "fp64" if flop_floor > bytes_floor else "bytes",
            "fraction_of_binding_floor": max(bytes_floor, flop_floor) / per_pair_us}
    dst = ROOT / "profiles" / "segmentation_kernels.json"
    dst.write_text(json.dumps(out, indent=1))
    print(json.dumps(out, indent=1))


def _scene(seed):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (34, 62, 3), dtype=np.uint8)
    from PIL import Image
    return np.asarray(Image.fromarray(small).resize((W + 128, H), Image.BICUBIC))


def _write_video(folder, regime, n=600):
    from PIL import Image
    rng = np.random.default_rng(7)
    paths, scene, left, base = [], 0, 0, None
    noise = rng.integers(-3, 4, (H, W, 3), dtype=np.int16)
    for i in range(n):
        if base is None or (regime == "cuts" and left == 0):
            scene += 1
            base, left = _scene(scene), int(rng.integers(4, 13))
        off = i % 64 if regime == "cuts" else 0
        img = np.clip(base[:, off:off + W].astype(np.int16) + np.roll(noise, i, axis=1), 0, 255).astype(np.uint8)
        p = os.path.join(folder, f"{regime}_{i:04d}.jpg")
        Image.fromarray(img).save(p, quality=90)
        paths.append(p)
        left -= 1
    return paths


def calls():
    import torch
    import ssim_oracle
    from hippomm_amd import frame_cache, segmentation as seg
    torch.cuda.set_device(0)
    rng = np.random.default_rng(3)
    out = {"frame": [H, W]}
    f1 = _scene(1)[:, :W, ::-1].copy()
    f2 = np.clip(f1.astype(np.int16) + rng.integers(-8, 9, f1.shape), 0, 255).astype(np.uint8)
    for _ in range(5):
        seg.compute_frame_difference(f1, f2)
    t = []
    for _ in range(30):
        t0 = time.perf_counter()
        seg.compute_frame_difference(f1, f2)
        t.append(time.perf_counter() - t0)
    out["compute_frame_difference_ms"] = {"median": 1e3 * float(np.median(t)), "min": 1e3 * min(t), "calls": len(t)}

    g1, g2 = ssim_oracle.gray_from_bgr(f1), ssim_oracle.gray_from_bgr(f2)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        ssim_oracle.ssim(g1, g2)
        t.append(time.perf_counter() - t0)
    out["oracle_cpu_ms_per_1080p_pair"] = {"median": 1e3 * float(np.median(t)),
                                          "note": "numpy restatement on the GPU host's CPU, a stand-in for skimage"}

    with tempfile.TemporaryDirectory(prefix="hmm_seg_probe_") as folder:
        from PIL import Image
        pa, pb = os.path.join(folder, "a.jpg"), os.path.join(folder, "b.jpg")
        Image.fromarray(f1[..., ::-1]).save(pa, quality=90)
        Image.fromarray(f2[..., ::-1]).save(pb, quality=90)
        seg._compute_frame_similarity(None, pa, pb)
        cold, warm = [], []
        for _ in range(10):
            frame_cache._default_cache = None
            t0 = time.perf_counter()
            seg._compute_frame_similarity(None, pa, pb)
            cold.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            seg._compute_frame_similarity(None, pa, pb)
            warm.append(time.perf_counter() - t0)
        out["compute_frame_similarity_jpeg_ms"] = {"cold_cache_median": 1e3 * float(np.median(cold)),
                                                   "warm_cache_median": 1e3 * float(np.median(warm)), "calls": len(cold)}
        out["segment_sequence_600_frames_1fps"] = {}
        for regime in ("cuts", "static"):
            t0 = time.perf_counter()
            paths = _write_video(folder, regime)
            write_s = time.perf_counter() - t0
            times = [float(i) for i in range(len(paths))]
            seg.segment_sequence(paths[:12], times[:12])                 # warm-up on another cache
            scorer = seg.PathScorer(seg.FrameCache())
            t0 = time.perf_counter()
            segs = seg.segment_sequence(paths, times, scorer=scorer)
            ms = 1e3 * (time.perf_counter() - t0)
            out["segment_sequence_600_frames_1fps"][regime] = {
                "total_ms": ms, "decodes": scorer.cache.decodes, "pairs_scored": scorer.pairs_scored, "segments": len(segs),
                "ms_per_video_second": ms / (times[-1] - times[0]), "jpeg_write_s_not_timed": write_s}
            for p in paths:
                os.remove(p)
    dst = ROOT / "profiles" / "segmentation_calls.json"
    dst.write_text(json.dumps(out, indent=1))
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "summarize", "calls"])
    ap.add_argument("--pairs", type=int, action="append")
    ap.add_argument("--stats", action="append")
    a = ap.parse_args()
    if a.mode == "kernels":
        kernels(a.pairs[0] if a.pairs else 1)
    elif a.mode == "summarize":
        summarize(a.stats, a.pairs)
    else:
        calls()
