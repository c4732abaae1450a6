"""GPU: hmm_audio_window_sums gives, per window, the bits of the numpy model of its order (tests/audio_levels_model.py) and through
them numpy's -- T(sum / n) is np.mean(np.square(window)) bit for bit -- for float32 and float64 tracks, on every window length at
which the order takes another path (under 8; eight accumulators with and without a tail; the first split, 129; a split off a
multiple of 8; one chunk of 8192 less one, exactly, plus one, plus a leaf; two chunks and five samples; the 500 ms windows of 22.05,
44.1 and 48 kHz) and at window starts 0, 1, 3 (no alignment may be assumed) and the one that ends on the track's last sample.
AudioTrack.window_levels equals segmentation.audio_level on the host slices.  A window's bits do not depend on the batch or the run."""
import warnings

import numpy as np
import pytest

import audio_levels_model as model

pytestmark = pytest.mark.gpu

LENGTHS = [1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 4000, 8191, 8192, 8193, 8200, 11025, 16389, 22050, 24000]
N = 24000 + 6011                                                  # odd: no window ends where a 16-byte load would
DTYPES = [np.float64, np.float32]
_cache = {}


def _bits(v):
    v = np.asarray(v)
    return v.view(np.uint32 if v.dtype == np.float32 else np.uint64)


def _samples(dtype) -> np.ndarray:
    rng = np.random.default_rng(21)
    x = 0.25 * rng.standard_normal(N) + 0.1 * np.sin(2 * np.pi * 440.0 * np.arange(N) / 16000.0)
    return x.astype(dtype)


def _grid():
    return np.array([(a, n) for n in LENGTHS for a in (0, 1, 3, N - n)], dtype=np.int64)


def _track(dtype):
    """One resident track, its host samples, the grid's sums from ONE launch and the model's sums: computed once, never changed."""
    from hippomm_amd.audio_track import AudioTrack
    key = np.dtype(dtype).name
    if key not in _cache:
        x = _samples(dtype)
        track = AudioTrack(x, 16000)
        table = _grid()
        got = track.window_sums(table)
        want = np.array([model.sum_squares(x[a:a + n]) for a, n in table.tolist()], dtype=dtype)
        for arr in (x, got, want):
            arr.setflags(write=False)
        _cache[key] = (track, x, table, got, want)
    return _cache[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_window_sums_are_the_models_bits_and_numpys(dtype):
    track, x, table, got, want = _track(dtype)
    assert got.dtype == dtype and got.shape == (len(LENGTHS) * 4,)
    bad = [(a, n, g, w) for (a, n), g, w in zip(table.tolist(), got, want) if _bits(g) != _bits(w)]
    assert not bad, bad[:5]
    bad = []
    for (a, n), s in zip(table.tolist(), got):
        mean = s.dtype.type(s / np.intp(n))
        ref = np.mean(np.square(x[a:a + n]))
        if type(mean) is not type(ref) or _bits(mean) != _bits(ref):
            bad.append((a, n, mean, ref))
    assert not bad, bad[:5]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_same_bits_alone_in_a_batch_of_59_and_on_a_repeated_call(dtype):
    track, x, table, got, _ = _track(dtype)
    again = track.window_sums(table)
    assert np.array_equal(_bits(again), _bits(got))
    rng = np.random.default_rng(3)
    for k in (0, 27, 45, 58, 67, 79):                              # lengths 1, 129, 4000, 8193, 11025 and 24000
        a, n = table[k].tolist()
        alone = track.window_sums(np.array([[a, n]], dtype=np.int64))
        assert _bits(alone[0]) == _bits(got[k]), (a, n)
        others = [(int(s), int(rng.integers(0, 12000))) for s in rng.integers(0, N - 12000, 58)]
        for pos in (0, 31, 58):
            batch = np.array(others[:pos] + [(a, n)] + others[pos:], dtype=np.int64)
            assert batch.shape == (59, 2)
            assert _bits(track.window_sums(batch)[pos]) == _bits(got[k]), (a, n, pos)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_empty_zero_nan_and_clipped_windows(dtype):
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.segmentation import audio_level
    x = _samples(dtype)[:20000].copy()
    x[5000:9000] = 0
    x[12345] = np.nan
    track = AudioTrack(x, 16000)
    table = np.array([(100, 0), (20000, 0), (5000, 4000), (5001, 3999), (12000, 1000), (12345, 1), (12346, 7654), (4990, 20)],
                     dtype=np.int64)
    s = track.window_sums(table)
    assert _bits(s[0]) == 0 and _bits(s[1]) == 0 and _bits(s[2]) == 0 and _bits(s[3]) == 0          # +0.0, not -0.0
    assert np.isnan(s[4]) and np.isnan(s[5])
    for k in (6, 7):
        a, n = table[k].tolist()
        assert _bits(s[k]) == _bits(model.sum_squares(x[a:a + n]))
    # window_levels clips to the track as the slice does: a window that crosses the end, one that starts on it, one past it
    starts = [19000, 19999, 20000, 30000, 5000, 12000, 0]
    got = track.window_level_values(starts, 4000)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # numpy's "Mean of empty slice"
        want = [audio_level(x[lo:lo + 4000], 16000) for lo in starts]
    assert want[2] == -100 and want[3] == -100 and want[4] == -100 and want[5] == -100 and np.isfinite(want[0])
    for g, w in zip(got, want):
        assert type(g) is type(w) and _bits(np.float64(g)) == _bits(np.float64(w))
    levels = track.window_levels(starts, 4000)
    assert levels.dtype == dtype and np.array_equal(_bits(levels), _bits(np.asarray(want, dtype=dtype)))
    assert track.window_levels([], 4000).shape == (0,)


def test_fp32_squares_that_are_subnormal_are_kept():
    """The squares lie between 1e-42 and 1e-39, below the smallest normal float32: with denormals flushed every sum would be 0."""
    from hippomm_amd.audio_track import AudioTrack
    rng = np.random.default_rng(8)
    x = (rng.uniform(1e-21, 3e-20, 9000) * rng.choice([-1.0, 1.0], 9000)).astype(np.float32)
    sq = np.square(x)
    assert np.all(sq > 0) and np.all(sq < np.finfo(np.float32).tiny)
    table = np.array([(0, 9000), (1, 8192), (3, 129), (8000, 7), (17, 1000)], dtype=np.int64)
    got = AudioTrack(x, 16000).window_sums(table)
    for (a, n), s in zip(table.tolist(), got):
        assert s > 0
        assert _bits(s) == _bits(model.sum_squares(x[a:a + n])), (a, n)
        assert _bits(np.float32(s / np.intp(n))) == _bits(np.mean(sq[a:a + n])), (a, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", ["n", "n1", "n2"])
def test_window_levels_equal_audio_level_on_the_host_slices(shape, dtype):
    from hippomm_amd.audio_track import AudioTrack
    from hippomm_amd.segmentation import audio_level
    rng = np.random.default_rng(13)
    n, rate = 3 * 22050 + 5, 22050
    x = 0.05 * rng.standard_normal(n)
    x[30000:45000] *= 1e-3                                        # a quiet stretch: levels on both sides of -40 dB
    if shape == "n":
        audio = x.astype(dtype)
    elif shape == "n1":
        audio = x[:, None].astype(dtype)
    else:
        other = 0.02 * rng.standard_normal(n)
        audio = np.stack([x + other, x - other], axis=1).astype(dtype)
    window = int(0.5 * rate)
    starts = list(range(n - window, 0, -window)) + [1, 3, n - 100]
    got = AudioTrack(audio, rate).window_level_values(starts, window)
    want = [audio_level(audio[lo:lo + window], rate) for lo in starts]
    assert min(want) < -40 < max(want)
    for lo, g, w in zip(starts, got, want):
        assert type(g) is type(w) is dtype and _bits(g) == _bits(w), (lo, g, w)


def test_a_track_that_was_not_float_at_its_source_is_refused():
    from hippomm_amd.audio_track import AudioTrack
    track = AudioTrack((1000 * np.sin(np.arange(16000))).astype(np.int16), 16000)
    with pytest.raises(TypeError, match="float32 or float64"):
        track.window_levels([0, 8000], 8000)
