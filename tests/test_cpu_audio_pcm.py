"""CPU: the 16-bit audio track without a device -- the C ABI of hmm_audio_pcm16_gather_clips, hmm_audio_pcm16_window_sums and
hmm_segment_walk_pcm16 (declared, exported, bound, ABI version unchanged; every argument error a status code with the function's name;
the four float entry points still refuse track_dtype 2), read_wav_pcm16 against scipy.io.wavfile and on hand-built headers, and the
numpy model of the exactness the kernels rest on: for int16 samples x and f = x / 32768.0, over the window lengths the GPU tests use,
the integer sum of squares times 2^-30 IS np.add.reduce(np.square(f)), np.mean is that sum divided by n, and f survives float32."""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
HMM_OK, HMM_E_INVALID = 0, -1
ONE = 1 << 20                                                    # a 16-byte aligned non-null dummy
FAR = 1 << 40                                                    # another one, far from the first
NEW = ("hmm_audio_pcm16_gather_clips", "hmm_audio_pcm16_window_sums", "hmm_segment_walk_pcm16")
WINDOW_LENGTHS = (0, 1, 7, 8, 9, 127, 128, 129, 8000, 8192, 8193, 1 << 22)


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def _table(rows):
    t = np.ascontiguousarray(rows, dtype=np.int64)
    return t, t.ctypes.data


def _refuser(lib, call, name):
    def refused(*args, say):
        assert call(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg
    return refused


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(build.build()))
    for name in NEW:
        assert name in declared and hasattr(raw, name) and name in _lib._SIGNATURES, name
    assert _lib.load().hmm_abi_version() == 7


def test_window_sums_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call = lib.hmm_audio_pcm16_window_sums
    refused = _refuser(lib, call, b"audio_pcm16_window_sums")
    keep, good = _table([[0, 100], [50, 950], [1000, 0]])
    #      track, track_len, windows_host, windows_dev, n_windows, sums, stream
    refused(ONE, -1, good, FAR, 3, 2 * FAR, None, say=b"negative")
    refused(ONE, 1000, good, FAR, -3, 2 * FAR, None, say=b"negative")
    for missing in range(4):
        p = [None if i == missing else v for i, v in enumerate((ONE, good, FAR, 2 * FAR))]
        refused(p[0], 1000, p[1], p[2], 3, p[3], None, say=b"null pointer")
    refused(ONE + 8, 1000, good, FAR, 3, 2 * FAR, None, say=b"aligned")               # the track: 16 bytes, not 8
    refused(ONE, 1000, good, FAR + 4, 3, 2 * FAR, None, say=b"aligned")
    refused(ONE, 1000, good, FAR, 3, 2 * FAR + 4, None, say=b"aligned")               # fp64 sums
    for bad in ([[0, 100], [50, 951]], [[-1, 100], [0, 1]], [[0, 100], [60, -1]], [[1001, 0], [0, 1]], [[2 ** 62, 2 ** 62], [0, 1]]):
        k, ptr = _table(bad)
        refused(ONE, 1000, ptr, FAR, 2, 2 * FAR, None, say=b"outside the track")
    k, ptr = _table([[0, 1 << 22], [5, (1 << 22) + 1]])                               # inside the track, but no longer exact
    refused(ONE, 1 << 23, ptr, FAR, 2, 2 * FAR, None, say=b"2^22")
    refused(ONE, 1000, good, FAR, 3, ONE, None, say=b"overlaps")                      # the sums inside the track's 2000 bytes
    refused(ONE, 1000, good, FAR, 3, ONE + 1992, None, say=b"overlaps")
    refused(ONE, 1000, good, FAR, 3, ONE - 8, None, say=b"overlaps")
    assert call(ONE, 1000, None, None, 0, None, None) == HMM_OK                       # no GPU here: HMM_OK means nothing was launched
    assert call(None, 0, None, None, 0, None, None) == HMM_OK
    del keep


def test_gather_clips_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call = lib.hmm_audio_pcm16_gather_clips
    refused = _refuser(lib, call, b"audio_pcm16_gather_clips")
    keep, good = _table([[0, 1000, 0, 0], [100, 900, 300, 0]])
    #      track, track_len, clips_host, clips_dev, n_clips, clip_len, orig, new, width, taps, out, stream
    refused(ONE, -1, good, FAR, 2, 500, 1, 1, 0, None, 2 * FAR, None, say=b"negative")
    refused(ONE, 1000, good, FAR, -2, 500, 1, 1, 0, None, 2 * FAR, None, say=b"negative")
    refused(ONE, 1000, good, FAR, 2, -5, 1, 1, 0, None, 2 * FAR, None, say=b"negative")
    refused(ONE, 1000, good, FAR, 2, 500, 0, 1, 0, None, 2 * FAR, None, say=b"at least 1")
    for missing in range(4):
        p = [None if i == missing else v for i, v in enumerate((ONE, good, FAR, 2 * FAR))]
        refused(p[0], 1000, p[1], p[2], 2, 500, 1, 1, 0, None, p[3], None, say=b"null pointer")
    refused(ONE, 1000, good, FAR, 2, 100, 441, 160, 6, None, 2 * FAR, None, say=b"null pointer")      # resampling without taps
    refused(ONE + 8, 1000, good, FAR, 2, 500, 1, 1, 0, None, 2 * FAR, None, say=b"aligned")
    refused(ONE, 1000, good, FAR + 4, 2, 500, 1, 1, 0, None, 2 * FAR, None, say=b"aligned")
    refused(ONE, 1000, good, FAR, 2, 500, 1, 1, 0, None, 2 * FAR + 2, None, say=b"aligned")
    for bad in ([[0, 1001, 0, 0]], [[-1, 10, 0, 0]], [[1001, 0, 0, 0]], [[5, -1, 0, 0]], [[2 ** 62, 2 ** 62, 0, 0]]):
        k, ptr = _table(bad)
        refused(ONE, 1000, ptr, FAR, 1, 1, 1, 1, 0, None, 2 * FAR, None, say=b"outside the track")
    for bad in ([[0, 1000, 501, 0]], [[0, 1000, -1, 0]], [[100, 400, 0, 0]]):
        k, ptr = _table(bad)
        refused(ONE, 1000, ptr, FAR, 1, 500, 1, 1, 0, None, 2 * FAR, None, say=b"reach past")
    refused(ONE, 1000, good, FAR, 2, 500, 1, 1, 0, None, ONE + 1996, None, say=b"overlaps")
    refused(ONE, 1000, good, FAR, 2, 500, 1, 1, 0, None, ONE - 4, None, say=b"overlaps")
    assert call(ONE, 1000, None, None, 0, 500, 1, 1, 0, None, None, None) == HMM_OK
    assert call(ONE, 1000, good, FAR, 2, 0, 1, 1, 0, None, None, None) == HMM_OK
    del keep


def _walk_args(**over):
    a = dict(scores=None, flags=None, times_dev=None, times_host=None, n_frames=0, track=ONE, track_len=16000, rate=1000, total=16.0,
             max_dur=10.0, min_dur=1.0, sim=0.95, rms_cut=1e-2, silent=1, max_windows=32, max_steps=20, records=FAR, state=2 * FAR,
             ws=3 * FAR, ws_bytes=1 << 20, stream=None)
    a.update(over)
    return tuple(a.values())


def test_segment_walk_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call = lib.hmm_segment_walk_pcm16
    refused = _refuser(lib, call, b"segment_walk_pcm16")
    refused(*_walk_args(records=None), say=b"null pointer")
    refused(*_walk_args(state=None), say=b"null pointer")
    refused(*_walk_args(ws=None), say=b"null pointer")
    refused(*_walk_args(n_frames=-1), say=b"negative")
    refused(*_walk_args(n_frames=3), say=b"null pointer")
    refused(*_walk_args(track_len=-1), say=b"track_len")
    refused(*_walk_args(rate=1), say=b"sample_rate")
    refused(*_walk_args(max_windows=0), say=b"max_windows")
    refused(*_walk_args(max_steps=0), say=b"max_steps")
    refused(*_walk_args(min_dur=0.0), say=b"min_segment_duration")
    refused(*_walk_args(total=float("inf")), say=b"not finite")
    refused(*_walk_args(rms_cut=float("nan")), say=b"NaN")
    refused(*_walk_args(track=ONE + 8), say=b"misaligned")
    refused(*_walk_args(records=FAR + 4), say=b"misaligned")
    refused(*_walk_args(rate=2 * (1 << 22) + 2, total=1.0), say=b"2^22")              # window = 2^22 + 1
    refused(*_walk_args(records=ONE + 16), say=b"overlaps the track")
    refused(*_walk_args(state=ONE + 31984), say=b"overlaps the track")
    refused(*_walk_args(ws=ONE - 8), say=b"overlaps the track")
    assert call(*_walk_args(ws_bytes=8)) == -2                                        # HMM_E_WORKSPACE
    assert b"segment_walk_pcm16" in lib.hmm_last_error()
    assert call(*_walk_args(rate=2 * (1 << 22), total=1.0, ws_bytes=8)) == -2         # a window of exactly 2^22 passes the bound


def test_the_float_entry_points_still_refuse_other_dtypes():
    lib = _lib()
    keep, table = _table([[0, 100, 0, 0]])
    for dtype in (2, -1):
        assert lib.hmm_audio_span_peaks(ONE, dtype, 1000, table, FAR, 1, 2 * FAR, None) == HMM_E_INVALID
        assert b"audio_span_peaks" in lib.hmm_last_error() and b"track_dtype" in lib.hmm_last_error()
        assert lib.hmm_audio_gather_clips(ONE, dtype, 1000, table, FAR, 1, 3 * FAR, 1, 50, 1, 1, 0, None, 2 * FAR, None) == HMM_E_INVALID
        assert b"audio_gather_clips" in lib.hmm_last_error() and b"track_dtype" in lib.hmm_last_error()
        assert lib.hmm_audio_window_sums(ONE, dtype, 1000, table, FAR, 1, 2 * FAR, None) == HMM_E_INVALID
        assert b"audio_window_sums" in lib.hmm_last_error() and b"track_dtype" in lib.hmm_last_error()
        assert lib.hmm_segment_walk(None, None, None, None, 0, ONE, dtype, 16000, 1000, 16.0, 10.0, 1.0, 0.95, 1e-2, 1, 32, 20, FAR, 2 * FAR,
                                    3 * FAR, 1 << 20, None) == HMM_E_INVALID
        assert b"segment_walk:" in lib.hmm_last_error() and b"track_dtype" in lib.hmm_last_error()
    del keep


# ---- read_wav_pcm16 ------------------------------------------------------------------------------------------------------------
def _samples(frames, channels, seed=3):
    x = np.random.default_rng(seed).integers(-32768, 32768, size=(frames, channels), dtype=np.int64).astype(np.int16)
    if frames:
        x[0, 0], x[-1, -1] = -32768, 32767
    return x


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("frames", [0, 1, 56005])
def test_read_wav_pcm16_agrees_with_scipy(frames, channels, tmp_path):
    from scipy.io import wavfile
    from hippomm_amd.audio_track import read_wav_pcm16
    x = _samples(frames, channels)
    path = tmp_path / "a.wav"
    wavfile.write(path, 16000, x[:, 0] if channels == 1 else x)
    want_rate, want = wavfile.read(path)
    rate, got = read_wav_pcm16(path)
    assert rate == want_rate == 16000
    assert got.dtype == np.int16 and got.shape == (frames, channels)
    assert np.array_equal(np.asarray(got), want.reshape(frames, channels)) and np.array_equal(np.asarray(got), x)
    assert frames == 0 or isinstance(got, np.memmap)


def _fmt(tag=1, channels=1, rate=16000, bits=16, align=None, extensible_of=None):
    align = channels * bits // 8 if align is None else align
    base = struct.pack("<HHIIHH", 0xFFFE if extensible_of is not None else tag, channels, rate, rate * align, align, bits)
    if extensible_of is None:
        return base
    return base + struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", extensible_of) + bytes.fromhex("000000001000800000aa00389b71")


def _chunk(tag, body, size=None):
    return tag + struct.pack("<I", len(body) if size is None else size) + body + (b"\0" if len(body) & 1 else b"")


def _riff(*chunks, magic=b"RIFF"):
    body = b"WAVE" + b"".join(chunks)
    return magic + struct.pack("<I", len(body)) + body


def _write(tmp_path, data: bytes):
    path = tmp_path / "h.wav"
    path.write_bytes(data)
    return path


def test_read_wav_pcm16_walks_hand_built_headers(tmp_path):
    from hippomm_amd.audio_track import read_wav_pcm16
    x = _samples(301, 1, seed=4)
    pcm = x.tobytes()
    # an odd-sized LIST chunk (with its pad byte) between fmt and data, as ffmpeg writes it
    rate, got = read_wav_pcm16(_write(tmp_path, _riff(_chunk(b"fmt ", _fmt()), _chunk(b"LIST", b"INFOISFT\x05\0\0\0Lavf\0"[:17]), _chunk(b"data", pcm))))
    assert rate == 16000 and np.array_equal(got, x)
    # the extensible format, stereo
    s = _samples(150, 2, seed=5)
    rate, got = read_wav_pcm16(_write(tmp_path, _riff(_chunk(b"fmt ", _fmt(channels=2, rate=44100, extensible_of=1)), _chunk(b"data", s.tobytes()))))
    assert rate == 44100 and got.shape == (150, 2) and np.array_equal(got, s)
    # a streamed file: data size 0xFFFFFFFF means to the end of the file
    rate, got = read_wav_pcm16(_write(tmp_path, _riff(_chunk(b"fmt ", _fmt()), _chunk(b"data", pcm, size=0xFFFFFFFF))))
    assert np.array_equal(got, x)
    # a file truncated in the middle of a frame: whole frames only
    whole = _riff(_chunk(b"fmt ", _fmt(channels=2)), _chunk(b"data", s.tobytes()))
    rate, got = read_wav_pcm16(_write(tmp_path, whole[:-5]))
    assert got.shape == (148, 2) and np.array_equal(got, s[:148])
    # a chunk behind data is not read as samples
    rate, got = read_wav_pcm16(_write(tmp_path, _riff(_chunk(b"fmt ", _fmt()), _chunk(b"data", pcm), _chunk(b"LIST", b"abcd"))))
    assert np.array_equal(got, x)


@pytest.mark.parametrize("name, data, say", [
    ("8 bit", _riff(_chunk(b"fmt ", _fmt(bits=8)), _chunk(b"data", b"\0" * 8)), "8-bit"),
    ("24 bit", _riff(_chunk(b"fmt ", _fmt(bits=24)), _chunk(b"data", b"\0" * 12)), "24-bit"),
    ("32 bit", _riff(_chunk(b"fmt ", _fmt(bits=32)), _chunk(b"data", b"\0" * 8)), "32-bit"),
    ("float", _riff(_chunk(b"fmt ", _fmt(tag=3, bits=32)), _chunk(b"data", b"\0" * 8)), "format tag 3"),
    ("extensible float", _riff(_chunk(b"fmt ", _fmt(bits=32, extensible_of=3)), _chunk(b"data", b"\0" * 8)), "format tag 3"),
    ("rf64", _riff(_chunk(b"fmt ", _fmt()), _chunk(b"data", b"\0" * 8), magic=b"RF64"), "RF64"),
    ("data first", _riff(_chunk(b"data", b"\0" * 8), _chunk(b"fmt ", _fmt())), "before any fmt"),
    ("block align", _riff(_chunk(b"fmt ", _fmt(channels=2, align=2)), _chunk(b"data", b"\0" * 8)), "block align 2"),
    ("no data", _riff(_chunk(b"fmt ", _fmt())), "no data chunk"),
    ("not riff", b"OggS" + b"\0" * 40, "not a RIFF/WAVE"),
])
def test_read_wav_pcm16_refuses_by_name(name, data, say, tmp_path):
    from hippomm_amd.audio_track import read_wav_pcm16
    with pytest.raises(ValueError, match=say):
        read_wav_pcm16(_write(tmp_path, data))


# ---- the numpy model of the sums -------------------------------------------------------------------------------------------------
def test_the_sum_of_squares_of_pcm_samples_is_exact_in_numpys_order():
    rng = np.random.default_rng(8)
    worst = np.full(1 << 22, -32768, dtype=np.int16)
    for n in WINDOW_LENGTHS:
        for x in (rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16), worst[:n]):
            f = x.astype(np.float64) / 32768.0
            exact = int(np.sum(np.square(x.astype(np.int64)), dtype=np.int64))                  # at most 2^52
            total = np.add.reduce(np.square(f))
            assert total == exact * 2.0 ** -30 and float(total).hex() == (exact * 2.0 ** -30).hex(), n
            assert np.array_equal(f.astype(np.float32).astype(np.float64), f), n
            if n:
                assert np.mean(np.square(f)) == np.float64(total / np.intp(n)), n
    assert np.add.reduce(np.square(worst.astype(np.float64) / 32768.0)) == 2.0 ** 22
