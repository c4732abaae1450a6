"""The device entropy pass against the host entropy pass, one session, the two sides alternating -> profiles/jpeg_entropy.json.

    python tools/jpeg_entropy_probe.py [--frames 32] [--out profiles/jpeg_entropy.json]

Per frame, for the 720p and 1080p synthetic q90 frames of tools/jpeg_decode_probe.py: the prepare pass and the host entropy pass on
one thread, the device pass's time per call (HIP events around hmm_jpeg_decode_coefs_device, bitstream slots already on the
device) at 1, 32 and 256 frames, the fixed-point rounds the frames took, bytes uploaded per frame on either route.  Then the
four workloads of DESIGN.md section 12 with HMM_JPEG_ENTROPY=device against host: extract_features on 32 paths, on 256 paths,
the same with HMM_DECODE_WORKERS=2, and segment_sequence on 600 1080p frames.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from jpeg_decode_probe import _median_ms, best_ms, frames  # noqa: E402


def device_ms(jpeg, torch, data, g, window, n):
    """ms per call of the device pass over n frames (the files of `data`, repeated), min of 5 -> (ms, max rounds, all decoded)."""
    stride = max(jpeg.entropy_slot_bytes(len(d)) for d in data)
    host = torch.zeros(n, stride, dtype=torch.uint8)
    for k in range(n):
        assert jpeg.prepare_entropy(data[k % len(data)], g, host[k].numpy()) == jpeg.DECODED
    bits = host.cuda()
    slots = torch.empty(n, jpeg.slot_bytes(g, window), dtype=torch.uint8, device="cuda")
    status = torch.empty(n, 2, dtype=torch.int32, device="cuda")
    best = float("inf")
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        jpeg.decode_coefs_device(bits, g, window, slots, status)
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    st = status.cpu().numpy()
    return round(best, 4), int(st[:, 1].max()), bool((st[:, 0] == jpeg.DECODED).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_entropy.json"))
    a = ap.parse_args()
    import torch
    from hippomm_amd import frame_cache, jpeg, preprocess, segmentation
    result = {"frames": a.frames, "sizes": {}, "workloads": {}}
    for w, h in ((1280, 720), (1920, 1080)):
        data = frames(w, h, a.frames)
        g = jpeg.parse(data[0])
        window = preprocess.needed_window(h, w)
        slot = np.zeros(jpeg.slot_bytes(g, window), dtype=np.uint8)
        bits = torch.zeros(max(jpeg.entropy_slot_bytes(len(d)) for d in data), dtype=torch.uint8).numpy()
        row = {"kb_per_file": round(sum(map(len, data)) / len(data) / 1024, 1), "window": list(window)}
        for leg in range(3):                                               # alternating; best of the legs
            p = best_ms(lambda d: jpeg.prepare_entropy(d, g, bits), data)
            e = best_ms(lambda d: jpeg.decode_coefs(d, g, window, slot), data)
            row["host_ms_prepare_pass"] = round(min(p, row.get("host_ms_prepare_pass", p)), 4)
            row["host_ms_entropy_pass"] = round(min(e, row.get("host_ms_entropy_pass", e)), 4)
        row["upload_bytes_coef_slot"] = int(slot.nbytes)
        row["upload_bytes_bitstream_slot_mean"] = int(np.mean([jpeg.entropy_slot_bytes(len(d)) for d in data]))
        for n in (1, 32, 256):
            ms, rounds, ok = device_ms(jpeg, torch, data, g, window, n)
            row[f"device_ms_per_call_{n}"] = ms
            row[f"device_us_per_frame_{n}"] = round(ms * 1e3 / n, 2)
            row[f"rounds_max_{n}"], row[f"all_decoded_{n}"] = rounds, ok
        result["sizes"][f"{w}x{h}"] = row
        print(json.dumps({f"{w}x{h}": row}), flush=True)

    from bench import write_synthetic_jpegs
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    with tempfile.TemporaryDirectory(prefix="hmm_jpeg_entropy_probe_") as folder:
        paths, _ = write_synthetic_jpegs(folder, 256)
        model = ImageBind(state_dict=synthetic_state_dict(("vision",), seed=1234), towers=("vision",))
        call = lambda ps: model.extract_features({"vision": ps}, ["vision"])["vision"].detach().cpu().numpy()  # noqa: E731
        for label, ps, workers in (("extract_features_32_ms", paths[:32], None), ("extract_features_256_ms", paths, None),
                                   ("extract_features_256_workers2_ms", paths, "2")):
            if workers:
                os.environ["HMM_DECODE_WORKERS"] = workers
            legs = {"device": [], "host": []}
            for mode in ("device", "host") * 2:
                os.environ["HMM_JPEG_ENTROPY"] = mode
                for _ in range(2):
                    call(ps)
                legs[mode].append(_median_ms(lambda: call(ps), 7))
            os.environ.pop("HMM_DECODE_WORKERS", None)
            result["workloads"][label] = {m: min(v) for m, v in legs.items()}
    with tempfile.TemporaryDirectory(prefix="hmm_jpeg_entropy_probe_") as folder:
        paths, _ = write_synthetic_jpegs(folder, 600, h=1080, w=1920)
        times = [float(i) for i in range(600)]
        legs = {"device": [], "host": []}
        for mode in ("device", "host") * 3:
            os.environ["HMM_JPEG_ENTROPY"] = mode
            frame_cache._default_cache = None                             # every leg decodes all its frames
            legs[mode].append(_median_ms(lambda: segmentation.segment_sequence(paths, times), 1))
        result["workloads"]["segment_sequence_600_1080p_ms"] = {m: min(v) for m, v in legs.items()}
    os.environ.pop("HMM_JPEG_ENTROPY", None)
    for row in result["workloads"].values():
        row["host_over_device"] = round(row["host"] / row["device"], 3)
    print(json.dumps(result["workloads"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
