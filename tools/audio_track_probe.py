"""The audio of one video: one call on the device track against the per-segment wav files it replaces, in one process.

    python tools/audio_track_probe.py [--out profiles/audio_track.json] [--minutes 20] [--rounds 5]

Input: a seeded float64 (n, 1) track (tones plus noise, peaks above 1 so that spans are scaled) of `minutes` minutes, cut into
consecutive 10-s spans (120 for 20 minutes); the full 12-block audio tower with synthetic weights.
  files   the parent route, per span: the reference's numpy recipe (hippocampal_memory.py:1205-1216), scipy.io.wavfile.write,
          extract_features({'audio': [path]}, ['audio']), .cpu()
  track   extract_audio_segments(audio_data, rate, spans).cpu() -- the upload of the track included -- and the same call on an
          AudioTrack that is already resident
Method: the routes alternate in one process after a warm-up round of each; every timed region is a host clock around work that
ends in a device synchronise (.cpu(), then torch.cuda.synchronize()); medians over the rounds are reported, with every round's
figure beside them.  Run at 16 kHz and again at 44.1 kHz (the files route then resamples with resample_waveform, the track route
in hmm_audio_gather_clips).  The embeddings of the two routes are compared on the way (worst 1 - cosine, worst |diff| on unit
rows): at 16 kHz single-file calls and the batched call run the tower in different batch regimes, so the bits differ."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
SPAN_SECONDS = 10


def make_track(rate: int, minutes: float):
    import numpy as np
    rng = np.random.default_rng(rate)
    n = int(minutes * 60 * rate)
    t = np.arange(n) / rate
    x = 0.1 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * np.sin(2 * np.pi * 1250.0 * t) + 0.4 * rng.standard_normal(n)
    return x[:, None]


def files_route(model, audio, rate, spans, folder):
    import numpy as np
    from scipy.io import wavfile
    out = []
    for i, (a, b) in enumerate(spans):
        seg = audio[a:b]
        mono = seg.mean(axis=1) if len(seg.shape) > 1 else seg
        if mono.dtype != np.float32:
            mono = mono.astype(np.float32)
        if np.abs(mono).max() > 1.0:
            mono = mono / np.abs(mono).max()
        path = os.path.join(folder, f"audio_segment_{i}.wav")
        wavfile.write(path, rate, mono)
        try:
            out.append(model.extract_features({"audio": [path]}, ["audio"])["audio"].detach().cpu())
        finally:
            os.remove(path)
    return out


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def one_rate(model, rate, minutes, rounds, folder):
    import torch
    from hippomm_amd.audio_track import AudioTrack
    audio = make_track(rate, minutes)
    n = audio.shape[0]
    spans = [(a, min(a + SPAN_SECONDS * rate, n)) for a in range(0, n, SPAN_SECONDS * rate)]
    routes = {
        "files_ms": lambda: torch.cat(files_route(model, audio, rate, spans, folder)),
        "track_from_array_ms": lambda: model.extract_audio_segments(audio, rate, spans).cpu(),
    }
    resident = AudioTrack(audio, rate, model.device)
    routes["track_resident_ms"] = lambda: model.extract_audio_segments(resident, rate, spans).cpu()
    results = {k: fn() for k, fn in routes.items()}              # warm-up: code objects, pinned staging, workspaces, tap tables
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():                             # alternating
            ms, _ = timed(fn)
            times[k].append(ms)
    unit = {k: torch.nn.functional.normalize(v.double(), dim=1) for k, v in results.items()}
    cos = (unit["files_ms"] * unit["track_from_array_ms"]).sum(dim=1)
    row = {"sample_rate": rate, "spans": len(spans), "track_samples": n, "track_bytes": int(audio.nbytes), "rounds": rounds}
    for k, v in times.items():
        row[k] = {"median": round(statistics.median(v), 3), "all": [round(x, 3) for x in v]}
    row["files_over_track_from_array"] = round(row["files_ms"]["median"] / row["track_from_array_ms"]["median"], 3)
    row["files_over_track_resident"] = round(row["files_ms"]["median"] / row["track_resident_ms"]["median"], 3)
    row["routes_agree"] = {"worst_one_minus_cos": float((1 - cos).max()),
                           "worst_abs_diff_unit_rows": float((unit["files_ms"] - unit["track_from_array_ms"]).abs().max()),
                           "resident_equals_from_array": bool(torch.equal(results["track_resident_ms"],
                                                                          results["track_from_array_ms"]))}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "audio_track.json"))
    ap.add_argument("--minutes", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rates", type=int, nargs="+", default=[16000, 44100])
    a = ap.parse_args()
    import torch
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("audio_track_probe needs a GPU: nothing is measured without one")
    model = ImageBind(state_dict=synthetic_state_dict(("audio",)), towers=("audio",))
    with tempfile.TemporaryDirectory(prefix="hmm_audio_probe_") as folder:
        rows = [one_rate(model, rate, a.minutes, a.rounds, folder) for rate in a.rates]
    report = {"probe": "tools/audio_track_probe.py", "device": torch.cuda.get_device_name(0), "minutes": a.minutes,
              "span_seconds": SPAN_SECONDS, "tower": "audio, 12 blocks, synthetic weights",
              "method": "host clock around work ending in a device synchronise; routes alternate after one warm-up round each",
              "rates": rows}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
