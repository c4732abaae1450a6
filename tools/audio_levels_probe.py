"""The audio-level scan of sequence segmentation: the host route (numpy per 500 ms window) against the resident track, in one process.

    python tools/audio_levels_probe.py [--out profiles/audio_levels.json] [--minutes 20] [--rounds 5]

Input: a seeded float64 (n, 1) track of `minutes` minutes (noise at about -26 dB with a silent gap of 0.3 .. 1.2 s every 4 .. 13 s, so
that walk steps break at their end, in their middle and not at all), at 16 kHz and again at 44.1 kHz.
  host      segment_sequence(None, None, audio, rate): audio-only, one audio_level call per window
  resident  segment_sequence(None, None, None, rate, audio_track=track) on an AudioTrack that is already on the device: per walk step
            one hmm_audio_window_sums launch, one read-back, the dB on the host
  upload    AudioTrack(audio, rate) alone, which the caller pays once per video (and needs anyway to embed the segments)
  kernel    hmm_audio_window_sums alone over the 59 windows of one full 30-s step, between device events, averaged over a burst of
            launches after a warm-up
Method: the routes alternate in one process after a warm-up of each; each timed region is a host clock around a call that ends in
its own read-back (the resident route) or never leaves the host; medians over the rounds are reported with every round's figure
beside them.  The two routes' segment lists are compared on the way.  No threshold depends on any of this: the route is chosen by
the caller's argument."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
STEP_WINDOWS = 59                                                  # a 30-s walk step: range(30 s - 0.5 s, 0, -0.5 s)


def make_track(rate: int, minutes: float):
    import numpy as np
    rng = np.random.default_rng(rate)
    n = int(minutes * 60 * rate)
    x = 0.05 * rng.standard_normal(n)
    t = 0.0
    while True:
        t += float(rng.uniform(4.0, 13.0))
        gap = float(rng.uniform(0.3, 1.2))
        if (t + gap) * rate >= n:
            break
        x[int(t * rate):int((t + gap) * rate)] = 0.0
        t += gap
    return x[:, None]


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def kernel_alone(track, rate: int, launches: int = 200):
    """hmm_audio_window_sums over the 59 windows of a 30-s step, device events around a burst of launches -> microseconds each."""
    import numpy as np
    import torch
    from hippomm_amd import _lib
    from hippomm_amd.audio_track import window_table
    lib = _lib.load()
    window = int(0.5 * rate)
    table = window_table([off for off in range(30 * rate - window, 0, -window)], window, track.n_samples)
    assert table.shape[0] == STEP_WINDOWS
    table_dev = torch.from_numpy(table).to(track.device)
    sums = torch.empty(table.shape[0], dtype=track.samples.dtype, device=track.device)

    def launch():
        _lib.check(lib.hmm_audio_window_sums(track.samples.data_ptr(), track.dtype_code, track.n_samples, table.ctypes.data,
                                             table_dev.data_ptr(), table.shape[0], sums.data_ptr(), _lib.stream_ptr()),
                   "hmm_audio_window_sums")
    for _ in range(10):
        launch()
    bursts = []
    for _ in range(5):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            launch()
        end.record()
        end.synchronize()
        bursts.append(start.elapsed_time(end) * 1e3 / launches)
    samples = int(table[:, 1].sum())
    us = statistics.median(bursts)
    return {"windows": STEP_WINDOWS, "window_samples": window, "launches_per_burst": launches,
            "us_per_launch": {"median": round(us, 2), "all": [round(b, 2) for b in bursts]},
            "bytes_read": samples * np.dtype(np.float64 if track.dtype_code else np.float32).itemsize,
            "gb_per_s": round(samples * (8 if track.dtype_code else 4) / us / 1e3, 1)}


def one_rate(rate: int, minutes: float, rounds: int, max_segment_duration: float):
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.segmentation import segment_sequence
    audio = make_track(rate, minutes)
    track = AudioTrack(audio, rate)
    routes = {
        "host_ms": lambda: segment_sequence(None, None, audio, rate, max_segment_duration=max_segment_duration),
        "resident_ms": lambda: segment_sequence(None, None, None, rate, max_segment_duration=max_segment_duration,
                                                audio_track=track),
        "upload_ms": lambda: AudioTrack(audio, rate),
    }
    results = {k: fn() for k, fn in routes.items()}                # warm-up: code objects, pinned staging
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():                               # alternating
            ms, _ = timed(fn)
            times[k].append(ms)
    host, resident = results["host_ms"], results["resident_ms"]
    row = {"sample_rate": rate, "track_samples": int(audio.shape[0]), "track_bytes": int(audio.nbytes), "rounds": rounds,
           "max_segment_duration": max_segment_duration, "segments": len(host),
           "segments_equal": [(s.start_time, s.end_time) for s in host] == [(s.start_time, s.end_time) for s in resident]}
    for k, v in times.items():
        row[k] = {"median": round(statistics.median(v), 3), "all": [round(x, 3) for x in v]}
    row["host_over_resident"] = round(row["host_ms"]["median"] / row["resident_ms"]["median"], 3)
    row["host_over_resident_plus_upload"] = round(row["host_ms"]["median"] / (row["resident_ms"]["median"] + row["upload_ms"]["median"]), 3)
    row["kernel_alone"] = kernel_alone(track, rate)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "audio_levels.json"))
    ap.add_argument("--minutes", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rates", type=int, nargs="+", default=[16000, 44100])
    ap.add_argument("--max-segment-durations", type=float, nargs="+", default=[10.0, 30.0],
                    help="the reference's default (19 windows per step) and a 30-s step (59)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("audio_levels_probe needs a GPU: nothing is measured without one")
    rows = [one_rate(rate, a.minutes, a.rounds, d) for rate in a.rates for d in a.max_segment_durations]
    report = {"probe": "tools/audio_levels_probe.py", "device": torch.cuda.get_device_name(0), "minutes": a.minutes,
              "method": "host clock around each segment_sequence call, routes alternating after one warm-up each; the kernel alone "
                        "between device events over bursts of launches",
              "runs": rows}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
