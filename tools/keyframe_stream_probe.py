"""What an up-to-date key-frame list costs on one MI355X while a video is still being encoded: growing the selection
(KeyFrameSelector / hmm_keyframe_extend) against re-selecting everything (select_key_frames_device), in one process.

    python tools/keyframe_stream_probe.py [--out profiles/keyframe_stream.json]

Input: tests/golden/recipes.py n3600_clusters600 (3600 rows seen, 600 kept) and 32 further rows of 6 new scenes.
(a) extend   one hmm_keyframe_extend of the 32 rows onto that state.  The state must not grow between repetitions, so each timed
             call is preceded by a one-word fill that puts the device count back (it is part of the figure).
(b) reselect the alternative before this class: select_key_frames_device on all 3632 rows (its own buffers, one count read-back),
             and hmm_gram_select alone on preallocated buffers (select_key_frames_async) for the device side.
(c) video    the whole 3600-row video fed in 32-row batches (113 extends, one kept() at the end) against one one-shot call.
             The stream of small launches is launch-bound and expected to be SLOWER than the one-shot: what the class buys is (a).
(d) bytes    device bytes held between calls: kept rows + indices + the 32-row workspace, against the one-shot's workspace.
Method: the sides alternate in one session; wall clock per call with the device drained before and after, and HIP events around
groups of calls after a warm-up of the same calls; every figure is the median of its repetitions."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "golden"))
ROUNDS, CALLS, BATCH = 5, 20, 32


def _event_ms(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def _wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def main():
    import numpy as np
    import torch
    import recipes
    from hippomm_amd import _lib as L
    from hippomm_amd.consolidation import KeyFrameSelector, select_key_frames_async, select_key_frames_device
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "keyframe_stream.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lib = L.load()
    video, _ = recipes.select_case("n3600_clusters600")
    more = recipes.clustered(BATCH, 6, 0.2, 99)
    seen = torch.from_numpy(video).cuda()
    new = torch.from_numpy(more).cuda()
    both = torch.cat([seen, new])
    n = seen.shape[0]

    sel = KeyFrameSelector()
    sel.extend(seen)
    kept_before = sel.kept()
    count = len(kept_before)
    thr, ws = sel.similarity_threshold, torch.empty(lib.hmm_keyframe_extend_workspace_bytes(BATCH), dtype=torch.uint8, device="cuda")

    def extend():
        sel._meta[:1].fill_(count)
        L.check(lib.hmm_keyframe_extend(new.data_ptr(), BATCH, 1024, thr, sel._rows.data_ptr(), sel._meta.data_ptr() + 8, sel.capacity,
                                        sel._meta.data_ptr(), n, count, ws.data_ptr(), ws.numel(), L.stream_ptr()), "hmm_keyframe_extend")

    def reselect():
        return select_key_frames_device(both)

    def reselect_async():
        return select_key_frames_async(both)

    def video_stream():
        s = KeyFrameSelector()
        for at in range(0, n, BATCH):
            s.extend(seen[at: at + BATCH])
        return s.kept()

    def video_one_shot():
        return select_key_frames_device(seen).cpu().numpy()

    # the answers agree, checked once outside the timing
    extend()
    torch.cuda.synchronize()
    grown = sel._meta[1: 1 + int(sel._meta[0].item())].cpu().tolist()
    one_shot = reselect().cpu().tolist()
    identical = grown == one_shot and video_stream().tolist() == video_one_shot().tolist() == kept_before.tolist()

    for fn in (extend, reselect, reselect_async, video_stream, video_one_shot):              # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ("extend_wall", "extend_dev", "reselect_wall", "reselect_dev", "video_stream_wall", "video_one_shot_wall")}
    for _ in range(ROUNDS):
        for _ in range(CALLS):
            t["extend_wall"].append(_wall_ms(extend))
            t["reselect_wall"].append(_wall_ms(reselect))
        t["extend_dev"].append(_event_ms(extend, CALLS))
        t["reselect_dev"].append(_event_ms(reselect_async, CALLS))
        t["video_stream_wall"].append(_wall_ms(video_stream))
        t["video_one_shot_wall"].append(_wall_ms(video_one_shot))
    out = {"method": f"{ROUNDS} rounds, the sides alternating; wall clock per call with the device drained ({CALLS} calls per round) and HIP "
                     f"events around {CALLS} calls; medians",
           "rows_seen": n, "rows_kept": count, "new_rows": BATCH, "new_rows_kept": len(one_shot) - count,
           "identical_to_one_shot": bool(identical),
           "a_extend_32_rows_ms": {"wall": _stats(t["extend_wall"]), "device": _stats(t["extend_dev"], 5)},
           "b_reselect_3632_rows_ms": {"wall": _stats(t["reselect_wall"]), "device_gram_select_alone": _stats(t["reselect_dev"], 5)},
           "c_whole_video_ms": {"stream_of_32_row_batches_wall": _stats(t["video_stream_wall"], 3),
                                "one_shot_wall": _stats(t["video_one_shot_wall"], 3), "extends": (n + BATCH - 1) // BATCH},
           "d_device_bytes": {"kept_rows": count * 4096, "kept_idx_and_count": 8 * (count + 1), "extend_workspace_32_rows": ws.numel(),
                              "one_shot_workspace_3632_rows": int(lib.hmm_gram_select_workspace_bytes(n + BATCH))}}
    out["b_over_a_wall"] = round(out["b_reselect_3632_rows_ms"]["wall"]["median"] / out["a_extend_32_rows_ms"]["wall"]["median"], 1)
    out["b_over_a_device"] = round(out["b_reselect_3632_rows_ms"]["device_gram_select_alone"]["median"] /
                                   out["a_extend_32_rows_ms"]["device"]["median"], 1)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
