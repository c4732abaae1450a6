"""save_checkpoint on the host route (the reference's expression) against the device route, in one session on one GPU.

    python tools/checkpoint_probe.py [--out profiles/checkpoint.json] [--reps 5] [--segments 360] [--hour-host-reps 1]

Two cases, each segment 10 s of 16 kHz float64 (160000, 1) audio with 10 frames of (10, 1024) fp32 vision and (1, 1024) audio
features:
  * one segment (the memory's own array is uploaded);
  * an hour-shaped video: --segments such segments cut from one track that is resident on the device (AudioTrack).
Per case: save_checkpoint(matrices="host") and save_checkpoint(matrices="device"), wall-clock milliseconds ending in a device
synchronise, medians of --reps runs after one warm-up, the two files compared byte for byte (by SHA-256; each file is deleted before
the next is written).  The hour case's host route runs --hour-host-reps times without a warm-up: one run of it takes minutes and
builds every sample as a Python list first, as the reference does.  The device route is then taken apart, each part on its own:
the kernels alone (device events around the encode and matrix-writer launches of all segments), the read-back of that many bytes
into pinned memory, and the write of that many bytes to a file.  The JSON is rewritten after every case."""
import argparse
import hashlib
import json
import statistics
import sys
import tempfile
import threading
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import probe_common  # noqa: F401  (puts the repository on sys.path)
import torch

from hippomm_amd import _lib, checkpoint as ck
from hippomm_amd.audio_track import AudioTrack

RATE, SECONDS, FRAMES = 16000, 10, 10


def heartbeat(stop):
    while not stop.wait(60):
        print("... still running", flush=True)


def wall(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(out), 3), "median_ms": round(statistics.median(out), 3), "runs": reps}


def digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 24), b""):
            h.update(block)
    return h.hexdigest()


def memories_of(track, n_segments, rng):
    out = []
    for i in range(n_segments):
        t0 = float(i * SECONDS)
        frames = [f"frames/v/{i:04d}_{j:02d}.jpg" for j in range(FRAMES)]
        out.append(SimpleNamespace(
            features={"vision": rng.standard_normal((FRAMES, 1024)).astype(np.float32), "audio": rng.standard_normal((1, 1024)).astype(np.float32)},
            content={"frames": frames}, timestamp=1.7e9 + i, source_time=t0, modalities=["vision", "audio"],
            segment_info=SimpleNamespace(start_time=t0, end_time=t0 + SECONDS, frames=frames, frame_times=[t0 + j for j in range(FRAMES)],
                                         audio_data=track[i * RATE * SECONDS:(i + 1) * RATE * SECONDS]),
            transcription=[{"start": t0, "end": t0 + SECONDS, "text": "what was said in these ten seconds"}]))
    return out


def parts(memories, dev, reps):
    """The device route's kernels, read-back and file write, each alone, for all segments."""
    lib = _lib.load()
    n = RATE * SECONDS
    wave = torch.from_numpy(np.ascontiguousarray(memories[0].segment_info.audio_data)).to(dev)
    vision = torch.from_numpy(memories[0].features["vision"]).to(dev)
    audio = torch.from_numpy(memories[0].features["audio"]).to(dev)
    cap = lib.hmm_json_matrix_text_bound(n, 1, ck.WAVEFORM_CLOSE_INDENT)
    ws_bytes = lib.hmm_json_write_matrix_device_workspace_bytes(n, 1)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.int64, device=dev)
    written = torch.empty(1, dtype=torch.int64, device=dev)
    b64 = torch.empty(lib.hmm_base64_encoded_length(8 * vision.numel()), dtype=torch.uint8, device=dev)

    def kernels():
        for _ in memories:
            _lib.check(lib.hmm_json_write_matrix_device(wave.data_ptr(), 1, n, 1, ck.WAVEFORM_CLOSE_INDENT, out.data_ptr(), cap, written.data_ptr(),
                                                        ws.data_ptr(), ws_bytes, _lib.stream_ptr()), "hmm_json_write_matrix_device")
            for f in (vision, audio):
                _lib.check(lib.hmm_base64_encode_device(f.data_ptr(), 0, f.numel(), b64.data_ptr(), b64.numel(), _lib.stream_ptr()),
                           "hmm_base64_encode_device")
    ms = sorted(probe_common.event_ms(kernels, 1, warmup=1) for _ in range(reps))
    text_bytes = int(written.item())
    per_segment = text_bytes + lib.hmm_base64_encoded_length(8 * vision.numel()) + lib.hmm_base64_encoded_length(8 * audio.numel())
    pinned = torch.empty(text_bytes, dtype=torch.uint8, pin_memory=True)

    def read_back():
        for _ in memories:
            pinned.copy_(out[:text_bytes], non_blocking=True)
            torch.cuda.current_stream().synchronize()
    host_text = pinned.numpy()
    with tempfile.TemporaryDirectory() as tmp:
        def file_write():
            with open(Path(tmp) / "w.json", "wb") as f:
                for _ in memories:
                    f.write(host_text)
        result = {"kernels_ms": {"min_ms": round(ms[0], 3), "median_ms": round(statistics.median(ms), 3), "runs": reps},
                  "read_back": wall(read_back, reps), "file_write": wall(file_write, reps),
                  "waveform_text_bytes_per_segment": text_bytes, "device_bytes_per_segment": per_segment}
    return result


def case(name, track, n_segments, resident, dev, reps, host_reps, host_warmup, tmp, publish):
    rng = np.random.default_rng(n_segments)
    memories = memories_of(track, n_segments, rng)
    audio_track = AudioTrack(track, RATE) if resident else None
    spans = [(i * RATE * SECONDS, (i + 1) * RATE * SECONDS) for i in range(n_segments)] if resident else None
    clock = lambda: 1.0                                            # noqa: E731  (one file name: each run overwrites the last)
    stats = {}
    entry = {"segments": n_segments, "track": "resident" if resident else "uploaded per segment"}
    entry["device"] = wall(lambda: ck.save_checkpoint(tmp, name, memories, matrices="device", audio_track=audio_track, audio_spans=spans,
                                                     now=clock, stats=stats), reps)
    path = Path(tmp) / "checkpoints" / f"checkpoint_{name}_1.json"
    entry["file_bytes"], entry["stats_last_run"] = path.stat().st_size, dict(stats)
    device_digest = digest(path)
    path.unlink()
    entry["device_parts"] = parts(memories, dev, reps)
    publish(entry)                                                 # the device route's figures survive a host route that does not finish
    entry["host"] = wall(lambda: ck.save_checkpoint(tmp, name, memories, matrices="host", now=clock), host_reps, warmup=host_warmup)
    entry["files_equal"] = digest(path) == device_digest
    path.unlink()
    entry["speedup_median"] = round(entry["host"]["median_ms"] / entry["device"]["median_ms"], 2)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(Path(probe_common.ROOT) / "profiles" / "checkpoint.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--segments", type=int, default=360)
    ap.add_argument("--hour-host-reps", type=int, default=1)
    a = ap.parse_args()
    dev = _lib.require_gpu()
    stop = threading.Event()
    threading.Thread(target=heartbeat, args=(stop,), daemon=True).start()
    rng = np.random.default_rng(0)
    track = rng.uniform(-1.0, 1.0, size=(a.segments * RATE * SECONDS, 1))
    result = {"device": torch.cuda.get_device_name(dev), "unit": "ms, wall clock ending in a device synchronise; kernels_ms from device events",
              "segment": f"{SECONDS} s of {RATE} Hz float64 (n, 1) audio, {FRAMES} frames", "cases": {}}

    def flush():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    with tempfile.TemporaryDirectory() as tmp:
        for key, args in (("one_segment", ("one", track[:RATE * SECONDS], 1, False, dev, a.reps, a.reps, 1)),
                          ("hour_shaped", ("hour", track, a.segments, True, dev, a.reps, a.hour_host_reps, 0))):
            def publish(entry, key=key):
                result["cases"][key] = entry
                flush()
                print(json.dumps({key: entry}), flush=True)
            publish(case(*args, tmp, publish))
    result["checkpoint_stats"] = ck.checkpoint_stats()
    flush()
    stop.set()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    sys.exit(main())
