"""CPU: the C ABI of hmm_audio_window_sums -- declared, exported, bound, ABI version unchanged; every argument error a status code with
the function's name on a host without a GPU; zero windows HMM_OK with nothing launched -- and the host route of the segmentation
untouched by the new keyword: an audio-only call without a track still needs no GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
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


def test_symbol_is_declared_exported_and_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    assert "hmm_audio_window_sums" in set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    assert hasattr(ctypes.CDLL(str(build.build())), "hmm_audio_window_sums")
    assert "hmm_audio_window_sums" in _lib._SIGNATURES
    assert _lib.load().hmm_abi_version() == 7


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call = lib.hmm_audio_window_sums
    keep, good = _table([[0, 100], [50, 950], [1000, 0]])

    def refused(*args, say):
        assert call(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert b"audio_window_sums" in msg and say in msg, msg

    #      track, dtype, track_len, windows_host, windows_dev, n_windows, sums, stream
    refused(ONE, 2, 1000, good, FAR, 3, 2 * FAR, None, say=b"track_dtype")
    refused(ONE, -1, 1000, good, FAR, 3, 2 * FAR, None, say=b"track_dtype")
    refused(ONE, 0, -1, good, FAR, 3, 2 * FAR, None, say=b"negative")
    refused(ONE, 0, 1000, good, FAR, -3, 2 * FAR, None, say=b"negative")
    for missing in range(4):
        p = [None if i == missing else v for i, v in enumerate((ONE, good, FAR, 2 * FAR))]
        refused(p[0], 0, 1000, p[1], p[2], 3, p[3], None, say=b"null pointer")
    refused(ONE + 4, 0, 1000, good, FAR, 3, 2 * FAR, None, say=b"aligned")
    refused(ONE, 0, 1000, good, FAR + 4, 3, 2 * FAR, None, say=b"aligned")
    refused(ONE, 0, 1000, good, FAR, 3, 2 * FAR + 2, None, say=b"aligned")
    refused(ONE, 1, 1000, good, FAR, 3, 2 * FAR + 4, None, say=b"aligned")          # fp64 sums need 8 bytes
    for bad in ([[0, 100], [50, 951]], [[-1, 100], [0, 1]], [[0, 100], [60, -1]], [[1001, 0], [0, 1]], [[2 ** 62, 2 ** 62], [0, 1]]):
        k, ptr = _table(bad)
        refused(ONE, 0, 1000, ptr, FAR, 2, 2 * FAR, None, say=b"outside the track")
    for dtype, size in ((0, 4), (1, 8)):                         # the sums inside the track's bytes: its first and its last element
        refused(ONE, dtype, 1000, good, FAR, 3, ONE, None, say=b"overlaps")
        refused(ONE, dtype, 1000, good, FAR, 3, ONE + 1000 * size - size, None, say=b"overlaps")
        refused(ONE, dtype, 1000, good, FAR, 3, ONE - size, None, say=b"overlaps")
    del keep


def test_zero_windows_return_ok_without_a_launch():
    """No GPU on this host: a launch would fail, HMM_OK means none was tried."""
    lib = _lib()
    assert lib.hmm_audio_window_sums(ONE, 0, 1000, None, None, 0, None, None) == HMM_OK
    assert lib.hmm_audio_window_sums(None, 1, 0, None, None, 0, None, None) == HMM_OK


def test_the_host_route_takes_the_keyword_and_needs_no_gpu():
    from hippomm_amd.segmentation import segment_sequence, walk_segments
    rng = np.random.default_rng(2)
    audio = 0.05 * rng.standard_normal((12 * 8000, 1))
    audio[int(7.4 * 8000):int(8.1 * 8000)] = 0
    plain = segment_sequence(None, None, audio, 8000)
    keyed = walk_segments(None, None, audio, 8000, None, audio_track=None)
    assert [(s.start_time, s.end_time) for s in plain] == [(s.start_time, s.end_time) for s in keyed] == [(0.0, 7.5), (7.5, 12.0)]
    assert all(np.shares_memory(s.audio_data, audio) for s in plain)
    assert segment_sequence(None, None, None, 8000) == []
