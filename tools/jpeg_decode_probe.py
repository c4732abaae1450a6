"""Host cost of the JPEG device route against Pillow's full decode, and decode_jpeg against the host route (A/B in one session).

    python tools/jpeg_decode_probe.py [--frames 32] [--out profiles/jpeg_decode.json]

Frames: the synthetic 1280x720 q90 frames of bench.py's formation_from_files leg (write_synthetic_jpegs) and 1920x1080 ones.
Records, per size: single-thread host ms per frame of Pillow's full decode and of the entropy pass alone (hmm_jpeg_decode_coefs),
their ratio, the bytes per frame each route uploads for the preprocessing window, and decode_jpeg wall ms per frame with the
device route on and off (the module's private switch)."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames(w, h, n, seed=0):
    """bench.py's synthetic scenes + sensor noise at quality 90 (they are generated on the GPU); without one, upscaled noise."""
    import torch
    from PIL import Image
    if torch.cuda.is_available():
        import tempfile
        sys.path.insert(0, ROOT)
        from bench import write_synthetic_jpegs
        with tempfile.TemporaryDirectory(prefix="hmm_jpeg_probe_") as folder:
            paths, _ = write_synthetic_jpegs(folder, n, h=h, w=w)
            out = []
            for p in paths:
                with open(p, "rb") as fh:
                    out.append(fh.read())
            return out
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        im = Image.fromarray(rng.integers(0, 256, (h // 4, w // 4, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=90)
        out.append(buf.getvalue())
    return out


def best_ms(fn, items, reps=3):
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        for it in items:
            fn(it)
        best = min(best, (time.perf_counter() - t) * 1e3 / len(items))
    return best


def _median_ms(fn, reps):
    import torch
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(times)), 2)


def formation(out_path):
    """extract_features on 32 and 256 paths (and 256 with HMM_DECODE_WORKERS=2, one rank's share of eight on 16 CPUs), device
    route against host route in one session, alternating A / B, median of 7 after 2 warm calls; then segment_sequence on 600
    1080p frames, each leg on a fresh frame cache (median of 3)."""
    import tempfile
    import torch
    from bench import write_synthetic_jpegs
    from hippomm_amd import frame_cache, jpeg, segmentation
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    res = {}
    with tempfile.TemporaryDirectory(prefix="hmm_jpeg_probe_") as folder:
        paths, mean_bytes = write_synthetic_jpegs(folder, 256)
        res["jpeg_mean_bytes_720p"] = int(mean_bytes)
        model = ImageBind(state_dict=synthetic_state_dict(("vision",), seed=1234), towers=("vision",))
        call = lambda ps: model.extract_features({"vision": ps}, ["vision"])["vision"].detach().cpu().numpy()
        for label, ps, workers in (("paths_32", paths[:32], None), ("paths_256", paths, None), ("paths_256_workers2", paths, "2")):
            if workers:
                os.environ["HMM_DECODE_WORKERS"] = workers
            legs = {}
            for on in (True, False, True, False):
                jpeg._route["on"] = on
                for _ in range(2):
                    call(ps)
                legs.setdefault("device" if on else "host", []).append(_median_ms(lambda: call(ps), 7))
            jpeg._route["on"] = True
            os.environ.pop("HMM_DECODE_WORKERS", None)
            row = {k: min(v) for k, v in legs.items()}
            row["all_medians"] = legs
            row["host_over_device"] = round(row["host"] / row["device"], 3)
            res[label] = row
            print(json.dumps({label: row}), flush=True)
    with tempfile.TemporaryDirectory(prefix="hmm_jpeg_probe_seg_") as folder:
        paths, mean_bytes = write_synthetic_jpegs(folder, 600, h=1080, w=1920)
        times = [float(i) for i in range(600)]
        legs = {}
        for on in (True, False, True, False, True, False):
            jpeg._route["on"] = on
            frame_cache._default_cache = None                   # every leg decodes all its frames
            t = _median_ms(lambda: segmentation.segment_sequence(paths, times), 1)
            legs.setdefault("device" if on else "host", []).append(t)
            if on:
                legs["device_decodes"] = segmentation.default_cache().device_decodes
        jpeg._route["on"] = True
        frame_cache._default_cache = None
        row = {"device": min(legs["device"]), "host": min(legs["host"]), "all": legs,
               "jpeg_mean_bytes_1080p": int(mean_bytes)}
        row["host_over_device"] = round(row["host"] / row["device"], 3)
        res["segment_sequence_600_1080p_ms"] = row
        print(json.dumps({"segment_sequence_600_1080p_ms": row}), flush=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


def kernels(n):
    """n 1080p frames through decode_jpeg 5 times (run under rocprofv3 --kernel-trace --stats for the reconstruction kernels)."""
    import torch
    from hippomm_amd import decode_jpeg
    data = frames(1920, 1080, n)
    for _ in range(5):
        decode_jpeg(data, device="cuda")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode.json"))
    ap.add_argument("--formation", metavar="JSON", help="only the extract_features / segment_sequence A/B, written to JSON")
    ap.add_argument("--kernels", type=int, metavar="N", help="only N 1080p frames through decode_jpeg (for a kernel trace)")
    a = ap.parse_args()
    if a.formation:
        return formation(a.formation)
    if a.kernels:
        return kernels(a.kernels)
    import torch
    from PIL import Image
    from hippomm_amd import jpeg, preprocess
    result = {"pillow": Image.__version__, "frames": a.frames, "sizes": {}}
    for w, h in ((1280, 720), (1920, 1080)):
        data = frames(w, h, a.frames)
        g = jpeg.parse(data[0])
        window = preprocess.needed_window(h, w)
        slot = np.zeros(jpeg.slot_bytes(g, window), dtype=np.uint8)
        full = best_ms(lambda d: Image.open(io.BytesIO(d)).convert("RGB").load(), data)
        entropy = best_ms(lambda d: jpeg.decode_coefs(d, g, window, slot), data)
        row = {"kb_per_file": round(sum(map(len, data)) / len(data) / 1024, 1), "window": list(window),
               "host_ms_pillow_full": round(full, 3), "host_ms_entropy_pass": round(entropy, 3),
               "entropy_over_full": round(entropy / full, 3),
               "upload_bytes_rgb_window": window[2] * window[3] * 3, "upload_bytes_coef_slot": int(slot.nbytes)}
        if torch.cuda.is_available():
            for on in (True, False):
                jpeg._route["on"] = on
                jpeg.decode_jpeg(data, device="cuda")
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(3):
                    jpeg.decode_jpeg(data, device="cuda")
                torch.cuda.synchronize()
                row["decode_jpeg_ms_per_frame_" + ("device" if on else "host")] = round((time.perf_counter() - t) * 1e3 / 3 / len(data), 3)
            jpeg._route["on"] = True
            row["decode_workers"] = preprocess.decode_workers()
        result["sizes"][f"{w}x{h}"] = row
        print(json.dumps({f"{w}x{h}": row}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
