"""What does the resident extraction walk buy per checked and per kept frame?

    python tools/frame_extraction_probe.py [--out profiles/frame_extraction.json] [--candidates 64] [--reps 5]

Frames: the synthetic video of bench.py's write_synthetic_jpegs (tools/jpeg_encode_probe.frames), 1280x720 and 1920x1080, as BGR
host arrays -- what cap.read() hands to the loop of extract_frames_from_video.  Every frame is a check frame one second after the
one before it, so all `candidates` frames are compared.  In one process and one session, the routes alternating within every
round, one warm round dropped, median of `reps`:

  A            what the parent commit offers: per candidate compute_frame_difference(frame, anchor), the reference's rules on the
               host, save_frame(frame, path) where kept
  B batch=1,4,16   FrameExtractor.push for every candidate, then flush
  B batch=16 resident   the same with cache= and tower_inputs=

Both routes must keep the same frames and write the same bytes.  Files go to a tmpfs folder (/dev/shm) and, in one more leg per
route, to the temporary folder on disk.  The steps of B on their own, per candidate: the upload of the staged candidates, gray +
walk + read-back of the records, and save_frames of the kept frames from the resident BGR (encode + write).  Every leg ends with a
device synchronisation; times are host wall-clock milliseconds."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = ((1280, 720), (1920, 1080))
FPS, INTERVAL = 30.0, 30


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def _summary(values, per):
    return {"median_ms": round(float(np.median(values)), 3), "min_ms": round(float(min(values)), 3),
            "max_ms": round(float(max(values)), 3), "per_candidate_ms": round(float(np.median(values)) / per, 4)}


def route_a(frames, folder):
    """The loop of extract_frames_from_video with the two single-shot drop-ins."""
    from hippomm_amd import segmentation as seg
    kept, anchor, cumulative, last = [], None, 0.0, 0.0
    for k, frame in enumerate(frames):
        count = k * INTERVAL
        t = count / FPS
        save = anchor is None
        if not save and t - last >= 1.0:
            diff = seg.compute_frame_difference(frame, anchor)
            cumulative += diff
            save = diff > seg.MAX_DIFF_THRESHOLD or cumulative > seg.MAX_DIFF_THRESHOLD
        if save and seg.save_frame(frame, os.path.join(folder, f"t_{int(t):04d}", f"frame_{count:06d}.jpg")):
            kept.append(count)
            anchor, cumulative, last = frame, 0.0, t
    return kept


def route_b(frames, folder, batch, resident=False):
    from hippomm_amd import preprocess as pp, segmentation as seg
    caches = dict(cache=seg.FrameCache(), tower_inputs=pp.TowerInputCache()) if resident else {}
    ex = seg.FrameExtractor(FPS, folder, check_interval=INTERVAL, batch=batch, **caches)
    for k, frame in enumerate(frames):
        ex.push(k * INTERVAL, frame)
    ex.flush()
    return [int(os.path.basename(p)[6:12]) for p in ex.frame_paths]


def steps_of_b(frames, kept, folder, batch=16):
    """One batch of B, its steps timed apart: upload, gray + walk + read-back, encode + write of the kept ones."""
    import torch
    from hippomm_amd import frame_extraction as seg
    from hippomm_amd._pinned import PinnedStage
    n = min(batch, len(frames))
    stage = PinnedStage((n, *frames[0].shape))
    for k in range(n):
        stage.host[k] = frames[k]
    dev = torch.device("cuda", torch.cuda.current_device())
    walker = seg._Walker(frames[0].shape[0], frames[0].shape[1], n, dev)
    up_ms, up = _timed(lambda: stage.pinned.to(dev, non_blocking=True))

    def walk():
        walker.fill(up)
        walker.walk(0, [k * INTERVAL for k in range(n)], FPS, INTERVAL, [0] * n, seg.MAX_DIFF_THRESHOLD, seg.MIN_SAVE_GAP)
        return walker.read(n)
    walk_ms, (records, _) = _timed(walk)
    mine = [k for k in range(n) if records["saved"][k]]
    paths = [os.path.join(folder, f"frame_{k:06d}.jpg") for k in mine]
    save_ms, ok = _timed(lambda: seg.save_frames([up[k] for k in mine], paths))
    assert all(ok) and [k * INTERVAL for k in mine] == [c for c in kept if c < n * INTERVAL]
    return {"batch": n, "kept_in_batch": len(mine), "upload_ms": up_ms, "gray_walk_readback_ms": walk_ms, "encode_write_ms": save_ms}


def probe(w, h, n, reps, tmpfs, disk):
    from jpeg_encode_probe import frames as synthetic
    frames = list(synthetic(w, h, n).flip(-1).contiguous().cpu().numpy())     # BGR, on the host
    routes = {"A": lambda f: route_a(frames, f), "B_batch1": lambda f: route_b(frames, f, 1),
              "B_batch4": lambda f: route_b(frames, f, 4), "B_batch16": lambda f: route_b(frames, f, 16),
              "B_batch16_resident": lambda f: route_b(frames, f, 16, resident=True)}
    legs = {f"{name}@{where}": [] for name in routes for where in ("tmpfs", "disk")}
    steps = {k: [] for k in ("upload_ms", "gray_walk_readback_ms", "encode_write_ms")}
    kept, files, facts = None, None, {}
    for rep in range(reps + 1):
        for where, base in (("tmpfs", tmpfs), ("disk", disk)):
            if where == "disk" and rep > 1:
                continue                                                      # one warm and one timed round on disk
            for name, run in routes.items():
                folder = os.path.join(base, f"{w}x{h}_{rep}_{name}")
                ms, got = _timed(lambda: run(folder))
                written = {os.path.relpath(os.path.join(d, f), folder): open(os.path.join(d, f), "rb").read()
                           for d, _, fs in os.walk(folder) for f in fs}
                if kept is None:
                    kept, files = got, written
                assert got == kept and written == files, f"{name}: the routes disagree"
                shutil.rmtree(folder)
                if rep:
                    legs[f"{name}@{where}"].append(ms)
        folder = os.path.join(tmpfs, f"{w}x{h}_{rep}_steps")
        row = steps_of_b(frames, kept, folder)
        shutil.rmtree(folder, ignore_errors=True)
        if rep:
            for k in steps:
                steps[k].append(row[k])
            facts = {k: row[k] for k in ("batch", "kept_in_batch")}
    out = {"candidates": n, "kept": len(kept), "same_frames_and_bytes": True,
           "routes": {k: _summary(v, n) for k, v in legs.items() if v},
           "steps_of_one_B_batch": {**facts, **{k: round(float(np.median(v)), 3) for k, v in steps.items()}}}
    a = out["routes"]["A@tmpfs"]["median_ms"]
    out["B_over_A_tmpfs"] = {k.split("@")[0]: round(v["median_ms"] / a, 3) for k, v in out["routes"].items()
                             if k.startswith("B") and k.endswith("tmpfs")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_extraction.json"))
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from PIL import Image
    if not torch.cuda.is_available():
        raise SystemExit("frame_extraction_probe needs the GPU: nothing is measured without one")
    tmpfs = tempfile.mkdtemp(prefix="frame_extraction_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    disk = tempfile.mkdtemp(prefix="frame_extraction_")
    result = {"pillow": Image.__version__, "device": torch.cuda.get_device_name(0), "reps": a.reps,
              "tmpfs": tmpfs.startswith("/dev/shm"), "order": "routes alternating within every round; one warm round dropped",
              "sizes": {}}
    try:
        for w, h in SIZES:
            row = probe(w, h, a.candidates, a.reps, tmpfs, disk)
            result["sizes"][f"{w}x{h}"] = row
            print(json.dumps({f"{w}x{h}": row}), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(result, fh, indent=1)
    finally:
        shutil.rmtree(tmpfs, ignore_errors=True)
        shutil.rmtree(disk, ignore_errors=True)


if __name__ == "__main__":
    main()
