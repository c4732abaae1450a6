"""CPU: the order of hmm_audio_window_sums, stated as a numpy model (tests/audio_levels_model.py), is numpy's own -- the model's mean
of squares equals np.mean(np.square(mono)) bit for bit on every length at which numpy's summation takes another path (under 8, the
eight accumulators with and without a tail, the first split, 8192-element chunks and what follows them), at slice offsets 0, 1 and 3
and for 1-D, (n, 1) and (n, 2) input, in float32 and float64 -- and the host half of AudioTrack.window_levels (sum -> dB,
audio_track.levels_from_sums) returns what segmentation.audio_level returns on the same windows.  Four wrong orders are each told
apart by the same comparison, so the comparison can see what it is there to pin."""
import warnings

import numpy as np
import pytest

import audio_levels_model as model

LENGTHS = list(range(1, 300)) + [4000, 8000, 8191, 8192, 8193, 8199, 8200, 11025, 16384, 16385, 22049, 22050, 24000, 48000, 96000]
OFFSETS = (0, 1, 3)
SHAPES = ("n", "n1", "n2")
N_TRACK = max(LENGTHS) + max(OFFSETS)


def _bits(v):
    return np.asarray(v).view(np.uint32 if np.asarray(v).dtype == np.float32 else np.uint64)


def make_track(shape: str, dtype, n: int = N_TRACK, seed: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed)
    x = 0.3 * rng.standard_normal(n) + 0.1 * np.sin(2 * np.pi * 440.0 * np.arange(n) / 16000.0)
    if shape == "n":
        return x.astype(dtype)
    if shape == "n1":
        return x[:, None].astype(dtype)
    other = 0.2 * rng.standard_normal(n)
    return np.stack([x + other, x - other], axis=1).astype(dtype)


def mono_of(track: np.ndarray) -> np.ndarray:
    """What AudioTrack keeps: the whole track mixed down once."""
    if track.ndim == 1:
        return track
    return np.ascontiguousarray(track.reshape(-1) if track.shape[1] == 1 else track.mean(axis=1))


def numpy_mean_square(window: np.ndarray):
    """The reference's expression up to the mean (hippocampal_memory.py:995-997)."""
    mono = window.mean(axis=1) if window.ndim > 1 else window
    return np.mean(np.square(mono))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_model_equals_numpy_bit_for_bit_and_levels_equal_audio_level(shape, dtype):
    from hippomm_amd.audio_track import levels_from_sums
    from hippomm_amd.segmentation import audio_level
    track = make_track(shape, dtype)
    mono = mono_of(track)
    assert mono.dtype == dtype and mono.ndim == 1
    bad = []
    for off in OFFSETS:
        for n in LENGTHS:
            want = numpy_mean_square(track[off:off + n])
            got = model.mean_square(mono[off:off + n])
            if type(got) is not type(want) or _bits(got) != _bits(want):
                bad.append((off, n, got, want))
            s = model.sum_squares(mono[off:off + n])
            level, = levels_from_sums(np.array([s]), [n])
            ref = audio_level(track[off:off + n], 16000)
            if type(level) is not type(ref) or _bits(np.float64(level)) != _bits(np.float64(ref)):
                bad.append(("level", off, n, level, ref))
    assert not bad, bad[:5]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_host_half_on_zero_nan_single_and_empty_windows(dtype):
    from hippomm_amd.audio_track import levels_from_sums
    from hippomm_amd.segmentation import audio_level
    rng = np.random.default_rng(9)
    loud = (0.4 * rng.standard_normal(8000)).astype(dtype)
    with_nan = loud.copy()
    with_nan[4321] = np.nan
    tiny = np.full(300, 1e-30, dtype=dtype)                        # fp32: the squares underflow to 0, the level is -100
    windows = [np.zeros(8000, dtype), with_nan, loud[:1], np.zeros(1, dtype), loud, tiny, np.full(7, 1e-3, dtype), loud[:0]]
    sums = np.array([model.sum_squares(w) for w in windows], dtype=dtype)
    assert sums[0] == 0 and np.isnan(sums[1]) and sums[7] == 0
    got = levels_from_sums(sums, [w.shape[0] for w in windows])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # numpy's "Mean of empty slice" for the last one
        want = [audio_level(w, 16000) for w in windows]
        want_2d = [audio_level(w[:, None], 16000) for w in windows]
    assert want[0] == -100 and type(want[0]) is int and want[1] == -100 and want[3] == -100 and want[7] == -100
    assert type(want[2]) is dtype and np.isfinite(want[4])
    for g, w, w2 in zip(got, want, want_2d):
        assert type(g) is type(w) is type(w2)
        assert _bits(np.float64(g)) == _bits(np.float64(w)) == _bits(np.float64(w2))


def test_window_table_clips_like_a_slice():
    from hippomm_amd.audio_track import window_table
    t = window_table([0, 5, 990, 1000, 1200], 20, 1000)
    assert t.dtype == np.int64 and t.tolist() == [[0, 20], [5, 20], [990, 10], [1000, 0], [1000, 0]]
    for lo, (a, n) in zip([0, 5, 990, 1000, 1200], t.tolist()):
        assert np.arange(1000)[lo:lo + 20].tolist() == list(range(a, a + n))
    assert window_table([], 20, 1000).shape == (0, 2)
    assert window_table([3], 0, 1000).tolist() == [[3, 0]]
    with pytest.raises(ValueError, match="negative"):
        window_table([4, -1], 20, 1000)
    with pytest.raises(ValueError, match="negative"):
        window_table([4], -20, 1000)


# ---- the comparison tells wrong orders apart ------------------------------------------------------------------------------
# variant -> the lengths of LENGTHS it is run on (at offset 0 of the 1-D track); the comparison must reject it on at least one
WRONG = {
    "no 8192 chunking": (dict(chunk=None), [8193, 8199, 8200, 11025, 16384, 16385, 22049, 22050, 24000, 48000, 96000]),
    "fused multiply-add": (dict(fused=True), list(range(1, 300))),   # one ulp of a partial sum often vanishes in the next rounding
    "left-to-right leaf": (dict(leaf="running"), list(range(1, 300))),
    "split not a multiple of 8": (dict(split_multiple=1), [257, 299, 4000, 8191]),
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(WRONG))
def test_wrong_orders_are_rejected(name, dtype):
    variant, lengths = WRONG[name]
    track = make_track("n", dtype)
    rejected = []
    for n in lengths:
        assert n in LENGTHS
        want = np.mean(np.square(track[:n]))
        assert _bits(model.mean_square(track[:n])) == _bits(want)
        if _bits(model.mean_square(track[:n], **variant)) != _bits(want):
            rejected.append(n)
    print(f"{name}, {np.dtype(dtype).name}: rejected at {len(rejected)} of {len(lengths)} lengths, first {rejected[:8]}")
    assert rejected, name
