"""Consolidating a video's segment memories: the device route against what a caller had to do before it existed, in one session on
one GPU.

    python tools/consolidate_timing.py [--out profiles/consolidate_device.json] [--groups 9] [--segments 360] [--rows 10]

Workload: 360 segment memories with a (10, 1024) fp32 vision block each, resident on the device (an hour of video at 1 fps:
n = 3600 rows in 40 planted clusters), handed over out of time order.
  * caller   every block read back to the host (once per block; the reference's _extract_frame_feature reads it once per FRAME),
             one row per frame, Python's stable sort by time, np.stack, select_key_frames on the stack (an upload), and the stack
             uploaded once more by event_json_bytes(event, matrices="device");
  * device   consolidate_short_term_memory(memories, features="device"): one gather launch over the blocks where they lie, the
             selection on the gathered matrix, the kept list read back, and the same event_json_bytes on the resident matrix.
Each is timed with and without the event text.  Times are wall-clock milliseconds ending in a device synchronise; the two routes
alternate inside every group and the median over the groups is reported, after two warm-up rounds.  The kept frames and the event
text of both routes are compared once.  hmm_rows_gather alone is timed with device events."""
import argparse
import json
import statistics
import sys
import time
import types
from pathlib import Path

import numpy as np

import probe_common  # noqa: F401  (puts the repository on sys.path)
import torch

from hippomm_amd import _lib, consolidate_short_term_memory, event_store as es
from hippomm_amd.consolidation import select_key_frames


def make_memories(segments, rows, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn(40, 1024, generator=g)
    order = torch.randperm(segments, generator=g).tolist()
    memories = []
    for s in order:
        cluster = torch.tensor([((s * rows + j) // 7) % 40 for j in range(rows)])
        block = (centres[cluster] + 0.05 * torch.randn(rows, 1024, generator=g)).to(dev)
        t0 = float(s * rows)
        memories.append(types.SimpleNamespace(
            features={"vision": block}, content={"frames": [f"frames/v/{s:04d}_{j:02d}.jpg" for j in range(rows)],
                                                 "frame_times": [t0 + j for j in range(rows)]},
            timestamp=1700000000.0 + s, source_time=t0, modalities=["vision"],
            segment_info=types.SimpleNamespace(start_time=t0, end_time=t0 + rows), transcription=[]))
    return memories


def event_of(features, times, frames, frame_times):
    return dict(features={"vision": features, "vision_times": times}, frames=frames, frame_times=frame_times,
                frame_captions=["a caption"] * len(frames), audio_times=None, audio_transcription=None, holistic_audio_transcription=None,
                summary="A summary.", start_time=0.0, end_time=float(len(times)))


def caller_route(memories, with_text):
    """What a caller does without the device route: the reference's loop (hippocampal_memory.py:818-865) around the drop-in selection."""
    memories = sorted(memories, key=lambda m: m.segment_info.start_time)
    data = []
    for m in memories:
        block = m.features["vision"].detach().cpu().numpy()
        for idx, frame in enumerate(m.content["frames"]):
            data.append((frame, block[idx], m.content["frame_times"][idx]))
    data.sort(key=lambda x: x[2])
    features = np.stack([d[1] for d in data])
    times = np.array([d[2] for d in data])
    kept = select_key_frames(features, times)
    frames, frame_times = [data[i][0] for i in kept], times[kept].tolist()
    text = es.event_json_bytes(event_of(features, times, frames, frame_times), matrices="device") if with_text else None
    return frames, text


def device_route(memories, with_text):
    c = consolidate_short_term_memory(list(memories), features="device")
    frames = c.content["frames"]
    text = (es.event_json_bytes(event_of(c.features["vision"], c.features["vision_times"], frames, c.content["frame_times"]), matrices="device")
            if with_text else None)
    return frames, text


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def gather_alone(memories, reps):
    lib = _lib.load()
    blocks = [m.features["vision"] for m in memories]
    rows = blocks[0].shape[0]
    table = torch.tensor([b.data_ptr() + 4096 * j for b in blocks for j in range(rows)], dtype=torch.int64, device=blocks[0].device)
    out = torch.empty(table.numel(), 1024, dtype=torch.float32, device=blocks[0].device)

    def call():
        _lib.check(lib.hmm_rows_gather(table.data_ptr(), table.numel(), 1024, out.data_ptr(), _lib.stream_ptr()), "hmm_rows_gather")
    ms = sorted(probe_common.event_ms(call, 20) for _ in range(reps))
    assert torch.equal(out, torch.cat(blocks))
    return {"min_us": round(ms[0] * 1e3, 2), "median_us": round(statistics.median(ms) * 1e3, 2), "rows": table.numel(),
            "bytes_moved": 2 * 4096 * table.numel()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(probe_common.ROOT) / "profiles" / "consolidate_device.json"))
    ap.add_argument("--groups", type=int, default=9)
    ap.add_argument("--segments", type=int, default=360)
    ap.add_argument("--rows", type=int, default=10)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    memories = make_memories(a.segments, a.rows, dev)
    routes = {"caller": caller_route, "device": device_route}
    answers = {name: fn(memories, True) for name, fn in routes.items()}          # warm-up 1, and the comparison
    assert answers["caller"][0] == answers["device"][0], "the two routes keep different frames"
    assert answers["caller"][1] == answers["device"][1], "the two routes write different event text"
    for name, fn in routes.items():                                              # warm-up 2
        fn(memories, True), fn(memories, False)
    times = {(name, with_text): [] for name in routes for with_text in (False, True)}
    for _ in range(a.groups):
        for with_text in (False, True):
            for name, fn in routes.items():                                      # the routes alternate inside every group
                times[(name, with_text)].append(wall_ms(lambda: fn(memories, with_text)))
    summary = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}   # noqa: E731
    result = {"device": torch.cuda.get_device_name(dev), "groups": a.groups, "segments": a.segments, "rows_per_segment": a.rows,
              "n": a.segments * a.rows, "kept_frames": len(answers["device"][0]), "event_text_bytes": len(answers["device"][1]),
              "unit": "ms, wall clock ending in a device synchronise; median of interleaved groups after two warm-up rounds",
              "consolidate": {name: summary(times[(name, False)]) for name in routes},
              "consolidate_and_event_text": {name: summary(times[(name, True)]) for name in routes},
              "rows_gather_alone": gather_alone(memories, 5)}
    for key in ("consolidate", "consolidate_and_event_text"):
        result[key]["caller_over_device"] = round(result[key]["caller"]["median_ms"] / result[key]["device"]["median_ms"], 2)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    sys.exit(main())
