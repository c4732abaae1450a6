"""Inputs of the recall-window tests and the composed oracle route they are compared with: tests/resize_oracle.py -> Pillow
``save(quality=95, subsampling=2)`` of the channel-swapped frame -> Pillow's decode of that file -> OpenCV's BGR2GRAY rule ->
tests/ssim_oracle.py (data_range = max - min of the earlier frame) -> the reference's walk (hippocampal_memory.py:2223-2249),
written out here as the reference writes it.  Everything is generated from seeds; the oracle is computed once per process."""
from __future__ import annotations

import io
from functools import lru_cache

import numpy as np

import resize_oracle as ro
import ssim_oracle as so

SIZE = (320, 180)                                      # cv2's (width, height)
CUT = 0.3
MARGIN = 1e-6                                          # the GPU's SSIM differs from the oracle's by ~1e-11: no decision may be closer
A, B = (360, 640), (400, 640)                          # two source geometries: the 2 x 2 area path and the linear one


def _noise(rng, hw):
    return rng.integers(0, 256, (*hw, 3), dtype=np.uint8)


@lru_cache(maxsize=1)
def windows():
    """-> [(name, [(time, BGR frame)])] in call order."""
    rng = np.random.default_rng(20240611)
    same = _noise(rng, A)
    flat = np.full((*A, 3), 128, np.uint8)
    half = _noise(rng, A)
    half[:, 320:] = 128                                # flat where `flat` is flat too: 0 / 0 in those windows, the mean is NaN
    other, twice = _noise(rng, B), _noise(rng, B)
    return [
        ("identical", [(10.0, same), (11.0, same.copy()), (12.0, same.copy())]),
        ("noise", [(3.0, _noise(rng, A)), (4.0, _noise(rng, A)), (5.0, _noise(rng, A))]),
        ("flat_first", [(0.0, flat), (1.0, half), (2.0, half.copy())]),
        ("single", [(7.5, _noise(rng, A))]),
        ("other_geometry", [(20.0, twice), (21.0, twice.copy()), (22.0, other)]),
        ("mixed_geometries", [(30.0, _noise(rng, B)), (31.0, _noise(rng, A))]),
        ("empty", []),
    ]


def reference_walk(score, m: int):
    """The loop of the reference for one window of m frames: ``score(i, j)`` is _compute_frame_similarity(file i, file j).
    -> (kept indices, the (i, j, score) it consulted)."""
    kept, consulted, prev = [], [], None
    for j in range(m):
        if prev is not None:
            similarity = score(prev, j)
            consulted.append((prev, j, similarity))
            if similarity > CUT:
                continue
        kept.append(j)
        prev = j
    return kept, consulted


def pillow_file(bgr: np.ndarray, quality: int = 95) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1]), "RGB").save(buf, "JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def pillow_gray(data: bytes) -> np.ndarray:
    from PIL import Image
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return so.gray_from_bgr(rgb[..., ::-1])


@lru_cache(maxsize=1)
def expected():
    """-> [dict(name, kept, times, files (of the kept frames), all_files (of every frame), consulted)] per window."""
    out = []
    for name, window in windows():
        small = [ro.resize(frame[None], SIZE)[0] for _, frame in window]
        files = [pillow_file(s) for s in small]
        grays = [pillow_gray(f) for f in files]
        kept, consulted = reference_walk(lambda i, j: so.ssim(grays[i], grays[j]), len(window))
        out.append(dict(name=name, kept=kept, times=[window[i][0] for i in kept], files=[files[i] for i in kept], all_files=files,
                        consulted=consulted))
    return out
