"""The audio track from the extracted 16-bit WAV against the float64 track from audio.npy, in one process.

    python tools/audio_pcm_probe.py [--out profiles/audio_pcm.json] [--minutes 20] [--rounds 5]

Input: the seeded 16 kHz track of tools/audio_track_probe.py (tones plus noise) of `minutes` minutes, quantised to int16 once and
written twice into a temporary folder: as the WAV ffmpeg would have written (scipy.io.wavfile.write) and as the audio.npy the
reference keeps beside it (np.save of the float64 (n, 1) array x / 32768, what sf.read returns for that WAV).  Both files are in the
page cache when they are read: the figures hold the host copy, the staging and the upload, not a disk.
  (a) file to resident track   np.load(audio.npy) + AudioTrack(array, rate)   against   AudioTrack.from_wav(path)
  (b) embeddings               extract_audio_segments over consecutive 10-s spans (120 for 20 minutes) on each resident track; the
                               full 12-block audio tower with synthetic weights
  (c) levels                   window_levels of the 59 windows of one 30-s walk step on each resident track
Method: the two routes of a figure alternate after one warm round of each; every timed region is a host clock around work that ends
in a device synchronise; the median of the rounds is reported with every round's figure beside it.  The two routes' results are
compared on the way: they must be equal bit for bit."""
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
RATE, SPAN_SECONDS, STEP_SECONDS = 16000, 10, 30


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def alternate(routes, rounds):
    """{name: fn} -> ({name: {"median", "all"}}, {name: the warm round's result})"""
    results = {k: fn() for k, fn in routes.items()}              # warm: code objects, pinned staging, workspaces
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(timed(fn)[0])
    return {k: {"median": round(statistics.median(v), 3), "all": [round(x, 3) for x in v]} for k, v in times.items()}, results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "audio_pcm.json"))
    ap.add_argument("--minutes", type=float, default=20.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from scipy.io import wavfile
    from audio_track_probe import make_track
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("audio_pcm_probe needs a GPU: nothing is measured without one")
    x = np.clip(np.rint(make_track(RATE, a.minutes)[:, 0] * 8192.0), -32768, 32767).astype(np.int16)
    n = x.shape[0]
    spans = [(s, min(s + SPAN_SECONDS * RATE, n)) for s in range(0, n, SPAN_SECONDS * RATE)]
    window = RATE // 2
    starts = list(range(STEP_SECONDS * RATE - window, 0, -window))
    model = ImageBind(state_dict=synthetic_state_dict(("audio",)), towers=("audio",))
    with tempfile.TemporaryDirectory(prefix="hmm_audio_pcm_probe_") as folder:
        npy, wav = os.path.join(folder, "audio.npy"), os.path.join(folder, "temp_audio.wav")
        np.save(npy, x.astype(np.float64).reshape(-1, 1) / 32768.0)
        wavfile.write(wav, RATE, x)
        sizes = {"audio_npy_bytes": os.path.getsize(npy), "wav_bytes": os.path.getsize(wav)}
        load, tracks = alternate({"npy_float64_ms": lambda: AudioTrack(np.load(npy), RATE, model.device),
                                  "wav_pcm16_ms": lambda: AudioTrack.from_wav(wav, model.device)}, a.rounds)
    f64, pcm = tracks["npy_float64_ms"], tracks["wav_pcm16_ms"]
    assert pcm.pcm and not f64.pcm and pcm.n_samples == f64.n_samples == n
    embed, emb = alternate({"float64_track_ms": lambda: model.extract_audio_segments(f64, RATE, spans).cpu(),
                            "pcm16_track_ms": lambda: model.extract_audio_segments(pcm, RATE, spans).cpu()}, a.rounds)
    levels, lev = alternate({"float64_track_ms": lambda: f64.window_levels(starts, window),
                             "pcm16_track_ms": lambda: pcm.window_levels(starts, window)}, a.rounds)
    report = {"probe": "tools/audio_pcm_probe.py", "device": torch.cuda.get_device_name(0), "minutes": a.minutes, "sample_rate": RATE,
              "track_samples": n, "rounds": a.rounds, "tower": "audio, 12 blocks, synthetic weights",
              "method": "host clock around work ending in a device synchronise; the two routes alternate after one warm round each; "
                        "both files come from the page cache",
              "bytes": dict(sizes, resident_float64=int(f64.samples.numel() * 8), resident_pcm16=int(pcm.samples.numel() * 2)),
              "file_to_resident_track": load,
              "extract_audio_segments": dict(embed, spans=len(spans)),
              "window_levels": dict(levels, windows=len(starts)),
              "routes_agree": {"embeddings_bit_equal": bool(torch.equal(emb["float64_track_ms"], emb["pcm16_track_ms"])),
                               "levels_bit_equal": bool(np.array_equal(lev["float64_track_ms"].view(np.uint64),
                                                                       lev["pcm16_track_ms"].view(np.uint64)))}}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
