"""What does encoding a frame on the GPU cost against Pillow on one host thread?  (A/B in one session, the two routes alternating.)

    python tools/jpeg_encode_probe.py [--out profiles/jpeg_encode.json]
    python tools/jpeg_encode_probe.py --kernels 8          # workload for `rocprofv3 --kernel-trace --stats --output-format csv`
    python tools/jpeg_encode_probe.py --stats-csv kernel_stats.csv [--out ...]   # add that run's per-kernel times to the profile

Frames: the synthetic video of bench.py's write_synthetic_jpegs (a low-frequency scene plus sensor noise of 4 grey levels; the same
seeds), 1280x720 and 1920x1080, as the uint8 arrays before Pillow sees them.  Quality 95, 4:2:0, the settings of save_frame.
Per size: Pillow on one thread (ms per frame); encode_jpeg from host arrays at 1, 8 and 32 frames per call, upload and read-back
included, with the device route on and off (the module's private switch; off is Pillow behind the same call); the same from
resident tensors; and the kernels alone between two device events.  Median of 7 after 2 warm calls, legs alternating on/off/on/off,
the smaller median of a route's two legs reported and all four kept."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUALITY, SUBSAMPLING = 95, "4:2:0"
SIZES = ((1280, 720), (1920, 1080))
BATCHES = (1, 8, 32)


def frames(w, h, n):
    """(n, h, w, 3) uint8 on the GPU: bench.py's synthetic frames (write_synthetic_jpegs) before they are encoded."""
    import torch
    from bench import SCENE_LEN
    g = torch.Generator(device="cuda")
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device="cuda")
    scene, scene_id = None, -1
    for i in range(n):
        sid = i // SCENE_LEN
        if sid != scene_id:
            g.manual_seed(1000 + sid)
            base = torch.randn(1, 3, 6, 8, generator=g, device="cuda")
            scene = torch.nn.functional.interpolate(base, size=(h, w), mode="bicubic", align_corners=False)[0] * 50.0 + 128.0
            scene_id = sid
        g.manual_seed(7_000_000 + i)
        frame = scene + 4.0 * torch.randn(3, h, w, generator=g, device="cuda")
        out[i] = frame.clamp_(0, 255).to(torch.uint8).permute(1, 2, 0)
    return out


def _median_ms(fn, reps=7, warm=2):
    import torch
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(times)), 3)


def _ab(call):
    """call() timed with the device route on, off, on, off -> {"device": ms, "pillow": ms, "all": ...} per call."""
    from hippomm_amd import jpeg
    legs = {}
    for on in (True, False, True, False):
        jpeg._encode_route["on"] = on
        legs.setdefault("device" if on else "pillow", []).append(_median_ms(call))
    jpeg._encode_route["on"] = True
    return {"device": min(legs["device"]), "pillow": min(legs["pillow"]), "all_medians": legs}


def kernels(n):
    """n resident 1080p frames through encode_jpeg 5 times (run under rocprofv3 --kernel-trace --stats)."""
    import torch
    from hippomm_amd import encode_jpeg
    dev_frames = frames(1920, 1080, n)
    for _ in range(5):
        encode_jpeg(dev_frames, QUALITY, SUBSAMPLING)
    torch.cuda.synchronize()


def merge_stats(csv_path, out_path):
    """The jpeg_* rows of a rocprofv3 kernel_stats.csv into the profile (the --kernels workload: 5 calls of N 1080p frames)."""
    with open(out_path) as fh:
        result = json.load(fh)
    rows = {}
    with open(csv_path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            if "jpeg_" in name:
                short = name.split("(")[0].split("::")[-1]
                rows[short] = {"calls": int(row["Calls"]), "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1),
                               "average_us": round(float(row["AverageNs"]) / 1e3, 1), "percent_of_trace": float(row["Percentage"])}
    result["kernel_trace_1080p"] = rows
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode.json"))
    ap.add_argument("--kernels", type=int, metavar="N", help="only N resident 1080p frames through encode_jpeg (for a kernel trace)")
    ap.add_argument("--stats-csv", metavar="CSV", help="merge a rocprofv3 kernel_stats.csv of the --kernels run into --out")
    a = ap.parse_args()
    if a.kernels:
        return kernels(a.kernels)
    if a.stats_csv:
        return merge_stats(a.stats_csv, a.out)
    import torch
    from PIL import Image
    import hippomm_amd
    from hippomm_amd import jpeg
    result = {"pillow": Image.__version__, "quality": QUALITY, "subsampling": SUBSAMPLING, "sizes": {}}
    for w, h in SIZES:
        dev_frames = frames(w, h, max(BATCHES))
        host_frames = dev_frames.cpu().numpy()
        files = hippomm_amd.encode_jpeg(dev_frames, QUALITY, SUBSAMPLING, stats=(stats := {}))
        assert files == [jpeg.pillow_encode(f, QUALITY, SUBSAMPLING) for f in host_frames] and stats["device"] == len(files), stats
        row = {"kb_per_file": round(sum(map(len, files)) / len(files) / 1024, 1), "frame_bytes": int(host_frames[0].nbytes),
               "bytes_equal_pillow": True}
        t = time.perf_counter()
        for f in host_frames:
            jpeg.pillow_encode(f, QUALITY, SUBSAMPLING)
        row["pillow_one_thread_ms_per_frame"] = round((time.perf_counter() - t) * 1e3 / len(host_frames), 3)
        for n in BATCHES:
            row[f"host_arrays_n{n}_ms_per_call"] = _ab(lambda: hippomm_amd.encode_jpeg(host_frames[:n], QUALITY, SUBSAMPLING))
            row[f"resident_n{n}_ms_per_call"] = _ab(lambda: hippomm_amd.encode_jpeg(dev_frames[:n], QUALITY, SUBSAMPLING))
            g = jpeg.encode_geometry(h, w, 3, SUBSAMPLING)
            out = torch.empty(n, (jpeg._encode_slot_bytes(g) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
            status = torch.empty(n, 2, dtype=torch.int32, device="cuda")
            ws = torch.empty(jpeg.encode_workspace_bytes(g, n), dtype=torch.uint8, device="cuda")
            times = []
            for k in range(9):
                a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a0.record()
                jpeg.encode_device(dev_frames[:n], g, QUALITY, "RGB", out, status, ws)
                a1.record()
                torch.cuda.synchronize()
                if k >= 2:
                    times.append(a0.elapsed_time(a1))
            row[f"kernels_only_n{n}_ms_per_call"] = round(float(np.median(times)), 3)
        result["sizes"][f"{w}x{h}"] = row
        print(json.dumps({f"{w}x{h}": row}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
