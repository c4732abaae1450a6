"""What does keeping the decoded pixels of saved frames on the device cost in save_frames, and what do the two reads after it save?

    python tools/jpeg_resident_probe.py [--out profiles/jpeg_resident.json] [--frames 32 256] [--reps 5]

Frames: the synthetic video of bench.py's write_synthetic_jpegs (tools/jpeg_encode_probe.frames), 1280x720 and 1920x1080, as BGR
host arrays -- what extract_frames_from_video hands to save_frame.  Per size and frame count, in one session, the two routes of
every call alternating (without, with, without, with ...), median of `reps` after one warm round:

  save_frames           into an empty folder, without caches and with cache= and tower_inputs= (the added cost; file writes included)
  segment_sequence      over the saved paths, with a fresh FrameCache (every consulted frame is decoded from its file) and with the
                        cache save_frames filled (no decode)
  extract_features      {'vision': paths} on the full-depth ViT-H tower with random weights, without a cache (the files are read
                        and decoded) and with the TowerInputCache save_frames filled (all hits)

The comparison route is the one without caches: the code of the parent commit, untouched.  Every leg ends with a device
synchronisation; times are host wall-clock milliseconds per call."""
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


def probe(w, h, n, reps, model, folder):
    import torch
    from jpeg_encode_probe import frames as synthetic
    from hippomm_amd import preprocess as pp, segmentation as seg
    host = synthetic(w, h, n).flip(-1).contiguous().cpu().numpy()             # BGR, on the host
    frames = list(host)
    times = [k * 0.5 for k in range(n)]
    legs = {k: [] for k in ("save_plain", "save_resident", "segment_files", "segment_resident", "extract_files", "extract_resident")}
    facts = {}
    for rep in range(reps + 1):
        rows = {}
        for route in ("plain", "resident"):
            sub = os.path.join(folder, f"{w}x{h}_{n}_{rep}_{route}")
            paths = [os.path.join(sub, f"frame_{k:06d}.jpg") for k in range(n)]
            os.makedirs(sub)
            cache, tower = (seg.FrameCache(), pp.TowerInputCache()) if route == "resident" else (None, None)
            ms, ok = _timed(lambda: seg.save_frames(frames, paths, cache=cache, tower_inputs=tower))
            assert all(ok)
            rows[f"save_{route}"] = ms
            scorer = seg.PathScorer(cache if cache is not None else seg.FrameCache())
            ms, segments = _timed(lambda: seg.segment_sequence(paths, times, scorer=scorer))
            rows["segment_" + ("resident" if cache is not None else "files")] = ms
            facts["segment_" + route] = {"segments": len(segments), "pairs_scored": scorer.pairs_scored, "decodes": scorer.cache.decodes}
            model.tower_inputs = tower
            ms, emb = _timed(lambda: model.extract_features({"vision": paths}, ["vision"])["vision"])
            rows["extract_" + ("resident" if tower is not None else "files")] = ms
            facts["extract_" + route] = {"hits": tower.hits if tower is not None else 0}
            rows["emb_" + route] = emb
            rows["segs_" + route] = [(s.start_time, s.end_time) for s in segments]
            shutil.rmtree(sub)
        assert torch.equal(rows["emb_plain"], rows["emb_resident"]) and rows["segs_plain"] == rows["segs_resident"]
        if rep:                                                                # the first round warms allocator, plans and checks
            for k in legs:
                legs[k].append(rows[k])
    model.tower_inputs = None
    out = {k: _summary(v) for k, v in legs.items()}
    med = {k: v["median_ms"] for k, v in out.items()}
    out["added_in_save_frames_ms"] = round(med["save_resident"] - med["save_plain"], 3)
    out["saved_in_segment_sequence_ms"] = round(med["segment_files"] - med["segment_resident"], 3)
    out["saved_in_extract_features_ms"] = round(med["extract_files"] - med["extract_resident"], 3)
    out["net_saved_ms"] = round(out["saved_in_segment_sequence_ms"] + out["saved_in_extract_features_ms"] - out["added_in_save_frames_ms"], 3)
    out["same_bits"] = True
    out["facts"] = facts
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_resident.json"))
    ap.add_argument("--frames", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from PIL import Image
    from hippomm_amd import preprocess as pp
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    model = ImageBind(state_dict=synthetic_state_dict(("vision",)), towers=("vision",))
    result = {"pillow": Image.__version__, "device": torch.cuda.get_device_name(0), "decode_workers": pp.decode_workers(),
              "reps": a.reps, "order": "plain, resident alternating within every round; one warm round dropped", "sizes": {}}
    folder = tempfile.mkdtemp(prefix="jpeg_resident_")
    try:
        for w, h in SIZES:
            for n in a.frames:
                row = probe(w, h, n, a.reps, model, folder)
                result["sizes"].setdefault(f"{w}x{h}", {})[f"n{n}"] = row
                print(json.dumps({f"{w}x{h} n{n}": {k: v for k, v in row.items() if k != "facts"}}), flush=True)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as fh:
                    json.dump(result, fh, indent=1)
    finally:
        shutil.rmtree(folder, ignore_errors=True)


if __name__ == "__main__":
    main()
