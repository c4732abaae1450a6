"""The window walk of sequence segmentation: driven from the host (walk="host") against walked on the device (walk="device"), with
every input resident, in one process.

    python tools/segment_walk_probe.py [--out profiles/segment_walk.json] [--frames 600] [--rounds 7]

Input: `frames` gray-replicated 1920 x 1080 frames at 1 fps, a new scene every 6 .. 14 frames, put into a FrameCache under the paths of
placeholder files (what save_frames(cache=) leaves behind: nothing is decoded on either side), and a float64 track of the same
length at 16 kHz on the device as an AudioTrack (noise at about -26 dB with a silent gap of 0.3 .. 1.2 s every 4 .. 13 s).
  host    segment_sequence(paths, times, None, 16000, scorer=, audio_track=): per walk step one or two hmm_ssim_pairs calls and one
          hmm_audio_window_sums call, each followed by a read-back -- the parent route, untouched
  device  the same call with walk="device": every adjacent pair scored in chunks of 64 frames, one hmm_segment_walk call, one read-back
Method: one warm-up of each side, then the sides alternate; each timed region is a host clock around one call, with a device
synchronisation before and after; medians over the rounds are reported with every round's figure beside them.  Library calls and
read-backs of the host side are counted in a pass of their own with the two functions that make them wrapped; the device side
reports its own.  The two segment lists are compared on the way.  No threshold depends on any of this: the route is the caller's
argument."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
H, W, RATE = 1080, 1920, 16000


def make_track(seconds: int):
    import numpy as np
    rng = np.random.default_rng(RATE)
    n = seconds * RATE
    x = 0.05 * rng.standard_normal(n)
    t = 0.0
    while True:
        t += float(rng.uniform(4.0, 13.0))
        gap = float(rng.uniform(0.3, 1.2))
        if (t + gap) * RATE >= n:
            break
        x[int(t * RATE):int((t + gap) * RATE)] = 0.0
        t += gap
    return x


def fill_cache(cache, folder: Path, n: int, dev):
    """n frames into the cache, made on the device: a smooth random scene per run of 6 .. 14 frames, +-1 of noise per frame."""
    import numpy as np
    import torch
    rng = np.random.default_rng(5)
    gen = torch.Generator(device=dev).manual_seed(5)
    paths, scene, left = [], None, 0
    for c0 in range(0, n, 30):
        batch = []
        for i in range(c0, min(c0 + 30, n)):
            if left == 0:
                coarse = torch.rand((1, 1, H // 40, W // 40), generator=gen, device=dev) * 200 + 20
                scene = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear")[0, 0]
                left = int(rng.integers(6, 15))
            left -= 1
            gray = (scene + torch.randint(-1, 2, (H, W), generator=gen, device=dev)).clamp(0, 255).to(torch.uint8)
            batch.append(gray[..., None].expand(H, W, 3))
            p = folder / f"frame_{i:05d}.jpg"
            p.write_bytes(b"placeholder %d" % i)                   # the cache keys a frame by its file's path, size and mtime
            paths.append(str(p))
        cache.put(paths[c0:], torch.stack(batch).contiguous())
    return paths


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def count_host_side(fn):
    """-> (library calls, read-backs) of one host-route call: each hmm_ssim_pairs and hmm_audio_window_sums call is read back."""
    from hippomm_amd import ssim as ssim_home                     # PathScorer looks ssim_launch up on this module
    from hippomm_amd.audio_track import AudioTrack
    calls = {"hmm_ssim_pairs": 0, "hmm_audio_window_sums": 0}
    ssim, sums = ssim_home.ssim_launch, AudioTrack.window_sums

    def counted_ssim(*a, **k):
        calls["hmm_ssim_pairs"] += 1
        return ssim(*a, **k)

    def counted_sums(self, table):
        calls["hmm_audio_window_sums"] += int(len(table) > 0)
        return sums(self, table)
    ssim_home.ssim_launch, AudioTrack.window_sums = counted_ssim, counted_sums
    try:
        fn()
    finally:
        ssim_home.ssim_launch, AudioTrack.window_sums = ssim, sums
    return calls, sum(calls.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "segment_walk.json"))
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("segment_walk_probe needs a GPU: nothing is measured without one")
    from hippomm_amd import _lib
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.frame_cache import FrameCache, PathScorer
    from hippomm_amd.segmentation import segment_sequence
    dev = _lib.require_gpu()
    with tempfile.TemporaryDirectory(prefix="hmm_segment_walk_") as folder:
        cache = FrameCache(cache_bytes=(a.frames + 8) * H * W)
        paths = fill_cache(cache, Path(folder), a.frames, dev)
        times = [float(i) for i in range(a.frames)]
        track = AudioTrack(make_track(a.frames), RATE)
        scorer = PathScorer(cache)
        stats = {}
        sides = {
            "host": lambda: segment_sequence(paths, times, None, RATE, scorer=scorer, audio_track=track, walk="host"),
            "device": lambda: segment_sequence(paths, times, None, RATE, scorer=scorer, audio_track=track, walk="device", stats=stats),
        }
        results = {k: fn() for k, fn in sides.items()}             # warm-up: code objects, allocator
        ms = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():                            # alternating
                ms[k].append(timed(fn)[0])
        host_calls, host_read_backs = count_host_side(sides["host"])
        decodes = cache.decodes
    host, device = results["host"], results["device"]
    equal = [(s.start_time, s.end_time, s.frames) for s in host] == [(s.start_time, s.end_time, s.frames) for s in device]
    report = {"probe": "tools/segment_walk_probe.py", "device": torch.cuda.get_device_name(0), "frames": a.frames,
              "frame_size": [H, W], "track_samples": a.frames * RATE, "sample_rate": RATE, "rounds": a.rounds,
              "method": "host clock around each segment_sequence call, device synchronised before and after, sides alternating after "
                        "one warm-up each; every input resident (cache.decodes stays 0)",
              "segments": len(host), "segments_equal": equal, "decodes": decodes,
              "host": {"ms": {"median": round(statistics.median(ms["host"]), 3), "all": [round(x, 3) for x in ms["host"]]},
                       "library_calls": host_calls, "read_backs": host_read_backs},
              "device": {"ms": {"median": round(statistics.median(ms["device"]), 3), "all": [round(x, 3) for x in ms["device"]]},
                         "library_calls": {"hmm_ssim_pairs": -(-(a.frames - 1) // 64), "hmm_segment_walk": 1},
                         "kernel_launches_of_the_walk": stats.get("launches"), "read_backs": stats.get("read_backs"),
                         "stats": stats},
              "host_over_device": round(statistics.median(ms["host"]) / statistics.median(ms["device"]), 3)}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
