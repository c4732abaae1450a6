"""Host statements of the audio-track recipe (hippomm_amd/audio_track.py, csrc/audio_track.hip), for the tests only.

reference_segment   the reference's own steps on one span (hippomm/core/hippocampal_memory.py:1205-1216): slice, mean, astype,
                    normalise -- what it then writes to a wav
resident_segment    the resident recipe: the whole track made mono and narrowed ONCE, then per span the peak and the division
resample_fp64       the polyphase windowed-sinc resampler of torchaudio.functional.resample stated in float64 on the float32 taps
                    of preprocess._resample_kernel, together with the magnitude sum  sum_t |taps_t| |x_t|  that bounds the error
                    of any fp32 evaluation of that dot product: (T + 2) 2^-24 times it
make_track          the seeded test track: tones of amplitude 0.1 plus noise, loud (spans there are scaled) but for one quiet stretch
"""
from __future__ import annotations

import math

import numpy as np

SR = 16000
N_TRACK = 41 * SR + 777
QUIET = (300000, 340000)                                         # |x| < 1 here; elsewhere peaks reach about 2.5
SPANS = [(0, 32000), (12345, 172345), (305000, 325800), (N_TRACK - 50000, N_TRACK), (100001, 132000), (200000, 200320)]
LAYOUTS = ("f64_n1", "f64_n", "f64_stereo", "f32_n")


def make_track(layout: str, n: int = N_TRACK, rate: int = SR, quiet=QUIET, seed: int = 7) -> np.ndarray:
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    noise = 0.6 * rng.standard_normal(n)
    noise[quiet[0]:quiet[1]] *= 0.2                               # the tones keep their amplitude: no mel bin falls to the log floor
    x = 0.1 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * np.sin(2 * np.pi * 1250.0 * t) + noise
    if layout == "f64_n1":
        return x[:, None].copy()
    if layout == "f64_n":
        return x
    if layout == "f32_n":
        return x.astype(np.float32)
    if layout == "f64_stereo":
        other = 0.5 * rng.standard_normal(n)
        return np.stack([x + other, x - other], axis=1)
    raise KeyError(layout)


def reference_segment(audio_data: np.ndarray, a: int, b: int) -> np.ndarray:
    seg = audio_data[a:b]
    mono = seg.mean(axis=1) if len(seg.shape) > 1 else seg
    if mono.dtype != np.float32:
        mono = mono.astype(np.float32)
    if np.abs(mono).max() > 1.0:
        mono = mono / np.abs(mono).max()
    return mono


def narrowed_track(audio_data: np.ndarray) -> np.ndarray:
    x = np.asarray(audio_data)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float32)
    if x.ndim == 2:
        x = x.reshape(-1) if x.shape[1] == 1 else x.mean(axis=1)
    return x.astype(np.float32)


def resident_segment(track_f32: np.ndarray, a: int, b: int):
    """-> (samples fp32, peak fp32, scaled?)"""
    x = track_f32[a:b]
    p = np.abs(x).max()
    if p > np.float32(1.0):
        return x / p, p, True
    return x, p, False


def resample_fp64(x_f32: np.ndarray, rate: int):
    """x: one span's fp32 samples at `rate`, a file of its own -> (y fp64 at 16 kHz, magnitude sum per sample, tap count T)."""
    import torch
    from hippomm_amd.preprocess import _resample_kernel
    g = math.gcd(int(rate), SR)
    orig, new = int(rate) // g, SR // g
    if orig == new:
        return x_f32.astype(np.float64), np.abs(x_f32.astype(np.float64)), 1
    kernels, width = _resample_kernel(orig, new)
    taps = kernels[:, 0].to(torch.float64).numpy()               # (new, T), the fp32 values exactly
    T = taps.shape[1]
    n = x_f32.shape[0]
    n_out = -(-new * n // orig)
    frames = -(-n_out // new)
    pad = np.zeros(width + (frames - 1) * orig + T, dtype=np.float64)
    pad[width:width + n] = x_f32.astype(np.float64)[: pad.shape[0] - width]
    win = np.lib.stride_tricks.sliding_window_view(pad, T)[::orig][:frames]          # (frames, T)
    y = (win @ taps.T).reshape(-1)[:n_out]
    mag = (np.abs(win) @ np.abs(taps).T).reshape(-1)[:n_out]
    return y, mag, T
