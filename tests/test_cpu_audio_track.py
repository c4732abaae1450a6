"""CPU: the audio track's C ABI (hmm_audio_span_peaks, hmm_audio_gather_clips) -- declared, exported, bound, ABI version unchanged,
every argument error a status code with the function's name on a host without a GPU, zero counts HMM_OK -- and the host side of
the recipe: the resident statement (narrow the whole track once, peak per span) against the reference's per-segment wav round
trip bit for bit, the fp64 resampling oracle against the existing resample_waveform within the fp32 dot-product bound, and the
span / clip table builders."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import audio_track_oracle as ato

ROOT = Path(__file__).resolve().parent.parent
NEW = ["hmm_audio_span_peaks", "hmm_audio_gather_clips"]
HMM_OK, HMM_E_INVALID = 0, -1
ONE = 1 << 20                                                    # a 16-byte aligned non-null dummy
FAR = 1 << 40                                                    # another one, far from the first


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def _table(rows):
    t = np.ascontiguousarray(rows, dtype=np.int64)
    return t, t.ctypes.data


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(build.build()))
    for name in NEW:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _lib._SIGNATURES, name
    assert _lib.load().hmm_abi_version() == 7


def test_span_peaks_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call, name = lib.hmm_audio_span_peaks, b"audio_span_peaks"
    keep, good = _table([[0, 100], [50, 1000]])

    def refused(*args, say):
        assert call(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg

    #      track, dtype, track_len, spans_host, spans_dev, n_spans, peaks, stream
    refused(ONE, 2, 1000, good, FAR, 2, 2 * FAR, None, say=b"track_dtype")
    refused(ONE, -1, 1000, good, FAR, 2, 2 * FAR, None, say=b"track_dtype")
    refused(ONE, 0, -1, good, FAR, 2, 2 * FAR, None, say=b"negative")
    refused(ONE, 0, 1000, good, FAR, -2, 2 * FAR, None, say=b"negative")
    for missing in range(4):
        p = [None if i == missing else v for i, v in enumerate((ONE, good, FAR, 2 * FAR))]
        refused(p[0], 0, 1000, p[1], p[2], 2, p[3], None, say=b"null pointer")
    refused(ONE + 4, 0, 1000, good, FAR, 2, 2 * FAR, None, say=b"aligned")
    refused(ONE, 0, 1000, good, FAR + 4, 2, 2 * FAR, None, say=b"aligned")
    refused(ONE, 0, 1000, good, FAR, 2, 2 * FAR + 2, None, say=b"aligned")
    for bad in ([[0, 100], [50, 1001]], [[-1, 100], [0, 1]], [[0, 100], [60, 50]], [[1001, 1001], [0, 1]]):
        k, ptr = _table(bad)
        refused(ONE, 0, 1000, ptr, FAR, 2, 2 * FAR, None, say=b"outside the track")
    for dtype, size in ((0, 4), (1, 8)):                         # the peaks inside the track's bytes: its first and its last four
        refused(ONE, dtype, 1000, good, FAR, 2, ONE, None, say=b"overlaps")
        refused(ONE, dtype, 1000, good, FAR, 2, ONE + 1000 * size - 4, None, say=b"overlaps")
        refused(ONE, dtype, 1000, good, FAR, 2, ONE - 4, None, say=b"overlaps")
    del keep


def test_gather_clips_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call, name = lib.hmm_audio_gather_clips, b"audio_gather_clips"
    track, tab, peaks, taps, out = ONE, FAR, 2 * FAR, 3 * FAR, 4 * FAR
    keep, good = _table([[0, 40000, 0, 0], [0, 40000, 4000, 0], [10000, 40000, 8000, 1]])

    def refused(*args, say):
        assert call(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg

    #      track, dtype, track_len, clips_host, clips_dev, n_clips, peaks, n_spans, clip_len, orig, new, width, taps, out, stream
    refused(track, 2, 50000, good, tab, 3, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"track_dtype")
    refused(track, 0, -5, good, tab, 3, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"negative")
    refused(track, 0, 50000, good, tab, -3, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"negative")
    refused(track, 0, 50000, good, tab, 3, peaks, -2, 32000, 1, 1, 0, None, out, None, say=b"negative")
    refused(track, 0, 50000, good, tab, 3, peaks, 2, -32000, 1, 1, 0, None, out, None, say=b"negative")
    refused(track, 0, 50000, good, tab, 3, peaks, 2, 32000, 3, 1, -19, taps, out, None, say=b"negative")
    refused(track, 0, 50000, good, tab, 3, peaks, 2, 32000, 0, 1, 0, None, out, None, say=b"at least 1")
    refused(track, 0, 50000, good, tab, 3, peaks, 2, 32000, 1, 0, 0, None, out, None, say=b"at least 1")
    refused(track, 0, 50000, good, tab, 3, peaks, 2, 32000, -441, 160, 17, taps, out, None, say=b"at least 1")
    for missing in range(5):
        p = [None if i == missing else v for i, v in enumerate((track, good, tab, peaks, out))]
        refused(p[0], 0, 50000, p[1], p[2], 3, p[3], 2, 32000, 1, 1, 0, None, p[4], None, say=b"null pointer")
    refused(track, 0, 50000, good, tab, 3, peaks, 2, 10000, 3, 1, 19, None, out, None, say=b"taps must be given")
    refused(track + 8, 0, 50000, good, tab, 3, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"aligned")
    refused(track, 0, 50000, good, tab + 4, 3, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"aligned")
    refused(track, 0, 50000, good, tab, 3, peaks, 2, 32000, 1, 1, 0, None, out + 2, None, say=b"aligned")
    # a span outside [0, track_len]
    refused(track, 0, 49999, good, tab, 3, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"outside the track")
    for bad in ([-1, 40000, 0, 0], [0, -4, 0, 0], [50001, 0, 0, 0], [2 ** 62, 2 ** 62, 0, 0]):
        k, ptr = _table([bad])
        refused(track, 0, 50000, ptr, tab, 1, peaks, 2, 1, 1, 1, 0, None, out, None, say=b"outside the track")
    for span in (-1, 2):
        k, ptr = _table([[0, 40000, 0, span]])
        refused(track, 0, 50000, ptr, tab, 1, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"span index")
    # clip_len past the span's output length: 40000 samples at 16 kHz; 13334 = ceil(40000 / 3) from 48 kHz; 14513 from 44.1 kHz
    refused(track, 0, 50000, good, tab, 3, peaks, 2, 32001, 1, 1, 0, None, out, None, say=b"reach past")
    k, ptr = _table([[0, 40000, 8001, 0]])
    refused(track, 0, 50000, ptr, tab, 1, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"reach past")
    k, ptr = _table([[0, 40000, -1, 0]])
    refused(track, 0, 50000, ptr, tab, 1, peaks, 2, 32000, 1, 1, 0, None, out, None, say=b"reach past")
    k, ptr = _table([[0, 40000, 0, 0]])
    refused(track, 0, 50000, ptr, tab, 1, peaks, 2, 13335, 3, 1, 19, taps, out, None, say=b"reach past")
    refused(track, 0, 50000, ptr, tab, 1, peaks, 2, 14514, 441, 160, 17, taps, out, None, say=b"reach past")
    # a ratio whose window does not fit the LDS
    refused(track, 0, 50000, ptr, tab, 1, peaks, 2, 10, 44101, 16000, 1671, taps, out, None, say=b"window")
    # the output inside the track's bytes
    for dtype, size in ((0, 4), (1, 8)):
        refused(track, dtype, 50000, good, tab, 3, peaks, 2, 32000, 1, 1, 0, None, track, None, say=b"overlaps")
        refused(track, dtype, 50000, good, tab, 3, peaks, 2, 32000, 1, 1, 0, None, track + 50000 * size - 4, None, say=b"overlaps")
        refused(track, dtype, 50000, good, tab, 3, peaks, 2, 32000, 1, 1, 0, None, track - 3 * 32000 * 4 + 4, None, say=b"overlaps")
    del keep


def test_zero_counts_return_ok_without_a_launch():
    """No GPU on this host: a launch would fail, HMM_OK means none was tried."""
    lib = _lib()
    assert lib.hmm_audio_span_peaks(ONE, 0, 1000, None, None, 0, None, None) == HMM_OK
    assert lib.hmm_audio_span_peaks(None, 1, 0, None, None, 0, None, None) == HMM_OK
    assert lib.hmm_audio_gather_clips(ONE, 0, 50000, None, None, 0, None, 0, 32000, 1, 1, 0, None, None, None) == HMM_OK
    assert lib.hmm_audio_gather_clips(ONE, 1, 50000, None, None, 0, None, 2, 32000, 441, 160, 17, FAR, None, None) == HMM_OK
    k, ptr = _table([[0, 40000, 0, 0]])
    assert lib.hmm_audio_gather_clips(ONE, 0, 50000, ptr, FAR, 1, 2 * FAR, 1, 0, 1, 1, 0, None, 3 * FAR, None) == HMM_OK


# ---- the recipe against the reference's steps -----------------------------------------------------------------------------
def _reference_clips(audio_data, a, b, folder, tag):
    """slice, mean, astype, normalise, wavfile.write, _read_wav_raw, audio_clip_bounds: the clips the file route cuts."""
    from scipy.io import wavfile
    from hippomm_amd.preprocess import _read_wav_raw, audio_clip_bounds
    path = str(folder / f"{tag}.wav")
    wavfile.write(path, ato.SR, ato.reference_segment(audio_data, a, b))
    data, rate = _read_wav_raw(path)
    assert rate == ato.SR and data.dtype == np.float32 and data.ndim == 1
    return [data[s:e] for s, e in audio_clip_bounds(data.shape[0], ato.SR)]


@pytest.mark.parametrize("layout", ato.LAYOUTS)
def test_resident_recipe_reproduces_the_wav_round_trip_bit_for_bit(layout, tmp_path):
    from hippomm_amd.audio_track import clip_spans, clip_tables
    audio = ato.make_track(layout)
    track = ato.narrowed_track(audio)
    assert track.dtype == np.float32 and track.shape == (ato.N_TRACK,)
    assert ato.SPANS[3][1] == ato.N_TRACK and ato.SPANS[2][1] - ato.SPANS[2][0] == 20800 and ato.SPANS[5][1] - ato.SPANS[5][0] == 320
    spans = clip_spans(ato.SPANS, ato.N_TRACK)
    tables = clip_tables(spans, 1, 1)
    scaled, lengths = [], set()
    for length, (positions, table) in tables.items():
        for i, s in enumerate(positions):
            a, b = ato.SPANS[s]
            x, p, was_scaled = ato.resident_segment(track, a, b)
            scaled.append(was_scaled)
            want = _reference_clips(audio, a, b, tmp_path, f"s{s}")
            for c in range(3):
                start, span_len, first, span = table[3 * i + c].tolist()
                assert (start, span_len, span) == (a, b - a, s)
                got = x[first:first + length]
                lengths.add(length)
                assert got.shape == want[c].shape
                assert np.array_equal(got.view(np.uint32), want[c].view(np.uint32)), (layout, s, c)
    assert any(scaled) and not all(scaled) and len(lengths) >= 2


# ---- fp64 resampling oracle against the existing resample_waveform --------------------------------------------------------
@pytest.mark.parametrize("rate", [44100, 48000, 22050, 8000])
def test_fp64_oracle_bounds_the_existing_resampler(rate):
    from hippomm_amd.preprocess import resample_waveform
    rng = np.random.default_rng(rate)
    n = 9 * rate
    track = (0.5 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 300.0 * np.arange(n) / rate)).astype(np.float32)
    a = int(2.8 * rate) + 3
    b = a + int(3.37 * rate)
    assert np.all(track[a - 64:a] != 0) and np.all(track[b:b + 64] != 0)          # what a leak would pick up
    x = track[a:b]
    got = resample_waveform(torch.from_numpy(x.copy())[None], rate)[0].numpy().astype(np.float64)
    want, mag, T = ato.resample_fp64(x, rate)
    assert got.shape == want.shape
    bound = (T + 2) * 2.0 ** -24 * mag
    ratio = np.abs(got - want) / bound
    print(f"rate {rate}: T {T}, worst |err| / bound {ratio.max():.3f}")
    assert np.all(np.abs(got - want) <= bound)
    # the bound discriminates: the same span with the track's neighbours leaking in misses it by orders of magnitude
    orig = rate // np.gcd(rate, ato.SR)
    pad = 4 * orig
    leaky = resample_waveform(torch.from_numpy(track[a - pad:b + pad].copy())[None], rate)[0].numpy().astype(np.float64)
    off = pad * (ato.SR // np.gcd(rate, ato.SR)) // orig
    leaky = leaky[off:off + want.shape[0]]
    assert (np.abs(leaky - want) / bound).max() > 100.0


# ---- span and clip tables -------------------------------------------------------------------------------------------------
def test_spans_of_uses_the_reference_truncation():
    from hippomm_amd.audio_track import spans_of
    segs = [SimpleNamespace(start_time=0.0, end_time=10.0), SimpleNamespace(start_time=10.03, end_time=27.7777),
            SimpleNamespace(start_time=1 / 3, end_time=2 / 3)]
    for rate in (16000, 44100):
        assert spans_of(segs, rate) == [(int(s.start_time * rate), int(s.end_time * rate)) for s in segs]
    assert spans_of(segs, 16000)[1] == (160480, 444443)
    assert spans_of([], 16000) == []


def test_clip_spans_clip_like_a_slice_and_refuse_empty_and_negative_spans():
    from hippomm_amd.audio_track import clip_spans
    got = clip_spans([(0, 10), (5, 2000), (999, 10 ** 12)], 1000)
    assert got.dtype == np.int64 and got.tolist() == [[0, 10], [5, 1000], [999, 1000]]
    for a, b in ((0, 10), (5, 2000), (999, 10 ** 12)):
        assert np.arange(1000)[a:b].tolist() == list(range(*clip_spans([(a, b)], 1000)[0]))
    assert clip_spans([], 1000).shape == (0, 2)
    for bad in ((-1, 10), (0, -1), (-5, -1)):
        with pytest.raises(ValueError, match="negative"):
            clip_spans([(0, 10), bad], 1000)
    for bad in ((10, 10), (20, 10), (1000, 2000), (5000, 6000)):
        with pytest.raises(ValueError, match=r"span 1 = \(%d, %d\) is empty" % bad):
            clip_spans([(0, 10), bad], 1000)


@pytest.mark.parametrize("rate", [16000, 44100, 48000, 22050, 8000])
def test_clip_tables_follow_audio_clip_bounds(rate):
    from hippomm_amd.audio_track import clip_spans, clip_tables, rate_ratio, resampled_length
    from hippomm_amd.preprocess import _audio_clip_bounds
    orig, new = rate_ratio(rate)
    assert orig * 16000 == new * rate
    n = 45 * rate + 13
    spans = clip_spans([(0, 10 * rate), (7, rate + 7), (3 * rate + 1, 30 * rate), (44 * rate, 50 * rate), (5 * rate, 7 * rate + 1),
                        (100, 100 + rate // 50), (20 * rate, 22 * rate)], n)
    tables = clip_tables(spans, orig, new)
    seen = []
    for length, (positions, table) in tables.items():
        assert table.dtype == np.int64 and table.shape == (3 * len(positions), 4) and positions == sorted(positions)
        for i, s in enumerate(positions):
            a, b = spans[s].tolist()
            n16 = -(-new * (b - a) // orig)
            assert n16 == resampled_length(b - a, orig, new)
            bounds = _audio_clip_bounds(n16, 16000)
            assert table[3 * i:3 * i + 3].tolist() == [[a, b - a, f, s] for f, _ in bounds]
            assert all(e - f == length and e <= n16 for f, e in bounds)
            seen.append(s)
    assert sorted(seen) == list(range(len(spans))) and len(tables) >= 2
    assert spans[3].tolist() == [44 * rate, n]                   # crossed the track's end: clipped
    assert 32000 in tables


def test_audio_track_refuses_a_host_device():
    from hippomm_amd.audio_track import AudioTrack
    with pytest.raises(ValueError, match="GPU"):
        AudioTrack(np.zeros(100), 16000, device="cpu")
