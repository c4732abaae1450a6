"""GPU: the memory contract of hmm_audio_window_sums in the guarded arena (tests/arena.py).  The track, the window table and the sums
are carved at exactly their size under the three poison patterns: every guard still holds its pattern afterwards, the sums are the
same bits under all three (a sample read before a window's first or behind its last -- windows start at samples 0, 1 and 3 and
end on the track's last sample, and the track's length is odd -- or a sum left unwritten would differ between two of them), and
nothing but sums_out[0 : n_windows] is written.  A device table that disagrees with the checked host copy is survived; a host
table that reaches outside the track is refused before anything is written."""
import numpy as np
import pytest
import torch

import arena as A
import audio_levels_model as model

pytestmark = pytest.mark.gpu

N = 20011
HMM_E_INVALID = -1


def _samples(dtype):
    rng = np.random.default_rng(31)
    return (0.3 * rng.standard_normal(N)).astype(dtype)


def _windows():
    return np.array([(0, N), (1, 8193), (3, 129), (N - 8200, 8200), (N - 1, 1), (7, 0), (N, 0), (5, 7), (2, 16389)], dtype=np.int64)


def _arena(pattern, x, table_dev, out_elems):
    from hippomm_amd import _lib
    dev = _lib.require_gpu()
    ar = A.GuardedArena(A.needed_bytes([x.nbytes, table_dev.nbytes, out_elems * x.itemsize]), dev, A.PATTERNS[pattern])
    track = ar.put(torch.from_numpy(x), "track")
    windows = ar.put(torch.from_numpy(table_dev), "windows")
    sums = ar.carve(out_elems * x.itemsize, "sums")
    return ar, track, windows, sums


def _call(ar, track, windows, sums, x, table_host, n_windows):
    from hippomm_amd import _lib
    lib = _lib.load()
    status = lib.hmm_audio_window_sums(ar.address(track), 1 if x.dtype == np.float64 else 0, x.shape[0], table_host.ctypes.data,
                                       ar.address(windows), n_windows, ar.address(sums), _lib.stream_ptr())
    torch.cuda.synchronize()
    return status


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_guards_hold_and_sums_do_not_depend_on_the_poison(dtype):
    x, table = _samples(dtype), _windows()
    want = np.array([model.sum_squares(x[a:a + n]) for a, n in table.tolist()], dtype=dtype)
    int_t = torch.int64 if dtype == np.float64 else torch.int32
    runs = {}
    for pattern in A.PATTERNS:
        ar, track, windows, sums = _arena(pattern, x, table, len(table))
        assert _call(ar, track, windows, sums, x, table, len(table)) == 0
        ar.check_guards()
        assert torch.equal(track.cpu(), torch.from_numpy(x).view(torch.uint8))                 # inputs are not written
        assert torch.equal(windows.cpu(), torch.from_numpy(table).view(torch.uint8).reshape(-1))
        runs[pattern] = sums.clone().view(int_t).cpu()
    for pattern, bits in runs.items():
        assert torch.equal(bits, runs["ones"]), pattern
    assert np.array_equal(runs["ones"].numpy().view(dtype).view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_nothing_is_written_outside_the_first_n_windows_sums(dtype):
    x, table = _samples(dtype), _windows()
    for pattern in A.PATTERNS:
        ar, track, windows, sums = _arena(pattern, x, table, len(table))
        assert _call(ar, track, windows, sums, x, table, 4) == 0
        ar.check_guards()
        assert ar.is_pattern(sums, start=4 * x.itemsize), pattern
        got = sums[:4 * x.itemsize].cpu().numpy().view(dtype)
        want = np.array([model.sum_squares(x[a:a + n]) for a, n in table[:4].tolist()], dtype=dtype)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
        assert _call(ar, track, windows, sums, x, table, 0) == 0                               # and nothing at all for no windows
        assert ar.is_pattern(sums, start=4 * x.itemsize)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_a_device_table_poisoned_past_the_track_is_survived(dtype):
    """The host copy is valid; the device copy holds the poison itself (-1, 0 or 0x7F7F...7F in every field) in some rows and
    windows that reach past the track in others.  Those rows' sums are unspecified; the rows that agree keep their bits."""
    x, table = _samples(dtype), _windows()
    want = np.array([model.sum_squares(x[a:a + n]) for a, n in table.tolist()], dtype=dtype)
    for pattern, word in A.PATTERNS.items():
        poison = np.array([word | (word << 32)], dtype=np.uint64).view(np.int64)[0]
        bad = table.copy()
        bad[0] = (poison, poison)
        bad[2] = (3, 2 ** 62)                                      # a length far past the track
        bad[4] = (N + 5, 10)                                       # a start past the track
        bad[5] = (-9, 100)                                         # a negative start
        bad[7] = (N - 3, 2 ** 40)
        ar, track, windows, sums = _arena(pattern, x, bad, len(table))
        assert _call(ar, track, windows, sums, x, table, len(table)) == 0
        ar.check_guards()
        assert torch.equal(track.cpu(), torch.from_numpy(x).view(torch.uint8))
        got = sums.cpu().numpy().view(dtype)
        for k in (1, 3, 6, 8):
            assert got[k:k + 1].view(np.uint8).tolist() == want[k:k + 1].view(np.uint8).tolist(), (pattern, k)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_an_invalid_host_table_is_refused_with_nothing_written(dtype):
    from hippomm_amd import _lib
    x, table = _samples(dtype), _windows()
    ar, track, windows, sums = _arena("ones", x, table, len(table))
    for row in ((-1, 10), (0, N + 1), (N - 9, 10), (N + 1, 0), (5, -2), (2 ** 62, 2 ** 62)):
        bad = table.copy()
        bad[3] = row
        assert _call(ar, track, windows, sums, x, bad, len(table)) == HMM_E_INVALID, row
        msg = _lib.load().hmm_last_error()
        assert b"audio_window_sums" in msg and b"outside the track" in msg, msg
        assert ar.is_pattern(sums), row
    ar.check_guards()
