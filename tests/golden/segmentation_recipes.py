"""Seeded frame and audio recipes for the SSIM / segmentation golden (segmentation_golden.json): make_segmentation_golden.py runs
the reference on them, the tests regenerate the same inputs.  Frames are gray-replicated BGR (B = G = R), so OpenCV's BGR2GRAY
of a frame is its channel 0 exactly and the golden generator can stand in for cv2 without changing a bit."""
from __future__ import annotations

import hashlib

import numpy as np


def sha256(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _scene(seed: int, h: int, w: int) -> np.ndarray:
    """A smooth random picture (float, 0..255): a few low-frequency cosines plus a coarse blocky texture."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), rng.uniform(60, 190))
    for _ in range(4):
        fy, fx, ph = rng.uniform(0.5, 4) / h, rng.uniform(0.5, 4) / w, rng.uniform(0, 2 * np.pi)
        img += rng.uniform(10, 40) * np.cos(2 * np.pi * (fy * y + fx * x) + ph)
    blocks = rng.uniform(-25, 25, (h // 8 + 1, w // 8 + 1))
    img += np.kron(blocks, np.ones((8, 8)))[:h, :w]
    return img


def gray_frame(scene: int, index: int, h: int, w: int, noise: float = 2.0, shift: int = 1) -> np.ndarray:
    """Frame `index` of `scene`: the scene picture shifted by index * shift columns plus seeded noise, uint8 (h, w)."""
    base = _scene(scene, h, w + 64)
    off = (index * shift) % 64
    rng = np.random.default_rng(scene * 100003 + index)
    img = base[:, off:off + w] + rng.normal(0, noise, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def bgr(gray: np.ndarray) -> np.ndarray:
    return np.repeat(gray[..., None], 3, axis=2)


# ---------------------------------------------------------------------------------------------------------- SSIM pairs
PAIR_CASES = ["7x7_random", "7x7_same", "9x13_scene", "15x21_cut", "120x160_scene", "120x160_cut", "120x160_noisy",
              "120x160_flat_a", "120x160_flat_both", "120x160_range1", "120x160_range1_bright", "64x64_dark_bright",
              "1080x1920_scene"]


def pair_case(name: str):
    """-> (a, b) uint8 gray frames of one shape; a plays skimage's im1."""
    h, w = (int(v) for v in name.split("_")[0].split("x"))
    kind = name.split("_", 1)[1]
    rng = np.random.default_rng(sha256(np.frombuffer(name.encode(), np.uint8)).encode()[0] * 7 + len(name))
    if kind == "random":
        return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "same":
        a = rng.integers(0, 256, (h, w), dtype=np.uint8)
        return a, a.copy()
    if kind == "scene":
        return gray_frame(11, 1, h, w), gray_frame(11, 0, h, w)
    if kind == "cut":
        return gray_frame(12, 0, h, w), gray_frame(13, 0, h, w)
    if kind == "noisy":
        return gray_frame(14, 0, h, w, noise=40.0), gray_frame(14, 1, h, w, noise=40.0)
    if kind == "flat_a":
        return np.full((h, w), 77, np.uint8), gray_frame(15, 0, h, w)
    if kind == "flat_both":
        return np.full((h, w), 77, np.uint8), np.full((h, w), 201, np.uint8)
    if kind == "range1":
        return rng.integers(100, 102, (h, w), dtype=np.uint8), rng.integers(100, 102, (h, w), dtype=np.uint8)
    if kind == "range1_bright":
        return rng.integers(254, 256, (h, w), dtype=np.uint8), rng.integers(253, 256, (h, w), dtype=np.uint8)
    if kind == "dark_bright":
        return rng.integers(0, 4, (h, w), dtype=np.uint8), rng.integers(250, 256, (h, w), dtype=np.uint8)
    raise KeyError(name)


def consecutive_1080p(n: int = 17, seed: int = 21):
    """n consecutive 1080p gray frames of one slowly moving scene with a cut in the middle (for the n - 1 adjacent pairs)."""
    return np.stack([gray_frame(seed + (i >= n // 2), i, 1080, 1920, noise=3.0, shift=2) for i in range(n)])


# ---------------------------------------------------------------------------------------------------------- frame differences
# compute_frame_difference cases beyond PAIR_CASES (each run with frames as BGR and as gray): the fallbacks of the reference
DIFF_FALLBACK_CASES = ["5x5_small", "shape_broadcast", "shape_mismatch"]


def diff_fallback_case(name: str):
    rng = np.random.default_rng(len(name) * 31)
    if name == "5x5_small":
        return rng.integers(0, 256, (5, 5), dtype=np.uint8), rng.integers(0, 256, (5, 5), dtype=np.uint8)
    if name == "shape_broadcast":
        return rng.integers(0, 256, (20, 30), dtype=np.uint8), rng.integers(0, 256, (1, 30), dtype=np.uint8)
    if name == "shape_mismatch":
        return rng.integers(0, 256, (20, 30), dtype=np.uint8), rng.integers(0, 256, (24, 30), dtype=np.uint8)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------- segmentation
SEG_CASES = ["cuts_default", "static_default", "cuts_config", "static_config", "irregular_unsorted", "base_offset",
             "duplicate_times", "flat_frames", "range1_frames", "odd_size", "size7", "audio_only", "video_audio",
             "video_audio_config", "mismatch_consulted", "mismatch_unconsulted"]

DEFAULT_PARAMS = (10.0, 5.0, 0.95, -40)          # the reference's __init__ defaults (hippocampal_memory.py:263-266)
CONFIG_PARAMS = (30.0, 10.0, 0.95, -40)          # the shipped config


def _times(n, kind, rng):
    if kind == "regular":
        return [float(i) for i in range(n)]
    if kind == "irregular":
        return [float(round(t, 3)) for t in np.cumsum(rng.uniform(0.3, 2.2, n)) - 0.5]
    raise KeyError(kind)


def _audio(seconds: float, sr: int, silences, seed: int) -> np.ndarray:
    """float32 noise at about -23 dB with quiet stretches (about -66 dB) and exact zeros, [(start s, end s, 'quiet'|'zero')]."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(int(seconds * sr)) * 0.07).astype(np.float32)
    for s, e, kind in silences:
        a, b = int(s * sr), int(e * sr)
        x[a:b] = 0.0 if kind == "zero" else x[a:b] * np.float32(0.007)
    return x


def seg_case(name: str):
    """-> dict(frames=[uint8 (h, w) gray per frame] or None, times=list or None, audio=float32 array or None, sr, params)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    h, w = 48, 64
    params = CONFIG_PARAMS if name.endswith("_config") else DEFAULT_PARAMS
    frames = times = audio = None
    sr = None
    if name in ("cuts_default", "cuts_config", "video_audio", "video_audio_config", "mismatch_consulted",
                "mismatch_unconsulted", "odd_size"):
        if name == "odd_size":
            h, w = 15, 21
        n = 70 if name.endswith("_config") else 40
        cut_every = [5, 9, 6, 13, 4, 8, 11, 7, 3, 12, 6]
        scene, left, frames = 100, cut_every[0], []
        for i in range(n):
            if left == 0:
                scene += 1
                left = cut_every[(scene - 100) % len(cut_every)]
            frames.append(gray_frame(scene, i, h, w))
            left -= 1
        times = _times(n, "regular", rng)
    elif name in ("static_default", "static_config"):
        n = 26 if name == "static_default" else 64
        frames = [gray_frame(200, 0, h, w, noise=1.0, shift=0) for _ in range(n)]
        frames = [np.clip(f.astype(int) + (i % 2), 0, 255).astype(np.uint8) for i, f in enumerate(frames)]
        times = _times(n, "regular", rng)
    elif name == "irregular_unsorted":
        n = 36
        frames = [gray_frame(300 + i // 6, i, h, w) for i in range(n)]
        times = _times(n, "irregular", rng)
        for a, b in ((3, 4), (10, 12), (20, 21)):
            times[a], times[b] = times[b], times[a]
    elif name == "base_offset":
        n = 30
        frames = [gray_frame(400 + i // 7, i, h, w) for i in range(n)]
        times = [100.0 + t for t in _times(n, "regular", rng)]
    elif name == "duplicate_times":
        n = 34
        frames = [gray_frame(500 + i // 5, i, h, w) for i in range(n)]
        times = [float(i // 2) * 1.5 for i in range(n)]
    elif name == "flat_frames":
        n = 24
        frames = [np.full((h, w), 40 + 3 * (i // 6), np.uint8) for i in range(n)]
        times = _times(n, "regular", rng)
    elif name == "range1_frames":
        n = 24
        frames = [rng.integers(120, 122, (h, w), dtype=np.uint8) for i in range(n)]
        times = _times(n, "regular", rng)
    elif name == "size7":
        n = 22
        frames = [gray_frame(600 + i // 4, i, 7, 7, noise=20.0) for i in range(n)]
        times = _times(n, "regular", rng)
    if name in ("audio_only", "video_audio", "video_audio_config"):
        sr = 16000
        seconds = 40.0 if name == "audio_only" else (len(times) - 1) + 0.5
        audio = _audio(seconds, sr, [(3.2, 4.1, "quiet"), (12.0, 13.3, "zero"), (21.6, 22.4, "quiet"), (33.0, 33.9, "quiet"),
                                     (47.0, 48.0, "zero"), (58.0, 59.5, "quiet")], seed=len(name))
    if name == "mismatch_consulted":
        frames[9] = gray_frame(100, 9, h + 2, w)            # the window [5, 15] consults (9, 8) before it breaks: raises
    if name == "mismatch_unconsulted":
        frames[1] = gray_frame(100, 1, h, w + 4)            # window [0, 10] breaks at the cut (5, 4) first: never consulted
    return dict(frames=frames, times=times, audio=audio, sr=sr, params=params)


def frame_name(i: int, ext: str = "png") -> str:
    return f"frame_{i:04d}.{ext}"
