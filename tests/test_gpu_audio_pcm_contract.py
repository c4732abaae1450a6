"""GPU: the memory contract of hmm_audio_pcm16_gather_clips and hmm_audio_pcm16_window_sums in the guarded arena (tests/arena.py).
The int16 track, the tables, the taps and the outputs are carved at exactly their size under the three poison patterns: every guard
still holds its pattern afterwards, the outputs are the same bits under all three -- a sample read before a clip's or a window's
first or behind its last (they start at samples 0, 1, 3 and 7 and end on the track's last sample; the track's length is odd, so no
16-byte load ends on its last byte) or an output left unwritten would differ between two of them -- nothing outside the
documented extent of an output is written, and a device table that disagrees with the checked host copy writes less, never
elsewhere."""
import numpy as np
import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu

HMM_E_INVALID = -1


def _track(n, seed=41):
    x = np.random.default_rng(seed).integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
    x[0], x[n - 1] = -32768, 32767
    return x


def _lib():
    from hippomm_amd import _lib as L
    return L.load(), L, L.require_gpu()


# ---- gather ----------------------------------------------------------------------------------------------------------------------
def _gather(pattern, x, rate, spans, poison_rows=None, n_clips=None):
    """-> {clip length: (table, the whole carved output as int32 bits, the arena, the output view)}"""
    from hippomm_amd.audio_track import clip_spans, clip_tables, rate_ratio
    from hippomm_amd.preprocess import _resample_kernel
    lib, L, dev = _lib()
    n = x.shape[0]
    orig, new = rate_ratio(rate)
    tables = clip_tables(clip_spans(spans, n), orig, new)
    taps_host, width = (None, 0) if orig == new else _resample_kernel(orig, new)
    sizes = [x.nbytes] + ([taps_host.numel() * 4] if taps_host is not None else [])
    for length, (_, t) in tables.items():
        sizes += [t.nbytes, 4 * t.shape[0] * length]
    ar = A.GuardedArena(A.needed_bytes(sizes), dev, A.PATTERNS[pattern])
    track = ar.put(torch.from_numpy(x), "track")
    taps = None if taps_host is None else ar.put(taps_host[:, 0].t().contiguous(), "taps")
    out = {}
    for length, (positions, table) in tables.items():
        on_device = table.copy()
        for row, value in (poison_rows or {}).get(length, {}).items():
            on_device[row] = value
        table_dev = ar.put(torch.from_numpy(on_device), f"clips table {length}")
        clips = ar.carve(4 * table.shape[0] * length, f"clips {length}")
        count = table.shape[0] if n_clips is None else n_clips
        L.check(lib.hmm_audio_pcm16_gather_clips(ar.address(track), n, table.ctypes.data, ar.address(table_dev), count, length, orig,
                                                 new, width, None if taps is None else ar.address(taps), ar.address(clips),
                                                 L.stream_ptr()), "hmm_audio_pcm16_gather_clips")
        out[length] = (table, clips, ar)
    torch.cuda.synchronize()
    ar.check_guards()
    assert torch.equal(track.cpu(), torch.from_numpy(x).view(torch.uint8))                        # inputs are not written
    return {length: (table, clips.clone().view(torch.int32).cpu(), ar, clips) for length, (table, clips, ar) in out.items()}


@pytest.mark.parametrize("rate", [16000, 44100])
def test_gather_guards_hold_and_clips_do_not_depend_on_the_poison(rate):
    n = 3 * rate + 1
    x = _track(n)
    spans = [(0, n), (1, n), (3, 3 + rate // 2), (7, n), (n - 2 * rate - 1, n)]
    runs = {pattern: _gather(pattern, x, rate, spans) for pattern in A.PATTERNS}
    first = runs["ones"]
    assert len(first) == 2
    for pattern, clips in runs.items():
        assert clips.keys() == first.keys()
        for length, (_, bits, _, _) in clips.items():
            assert torch.equal(bits, first[length][1]), (pattern, length)
    if rate == 16000:                                             # and they are the samples: (float)x * 2^-15
        f = x.astype(np.float32) / np.float32(32768)
        for length, (table, bits, _, _) in first.items():
            got = bits.numpy().view(np.float32).reshape(-1, length)
            for c, (a, _, at, _) in enumerate(table.tolist()):
                assert np.array_equal(got[c], f[a + at:a + at + length]), (length, c)


@pytest.mark.parametrize("rate", [16000, 44100])
def test_gather_writes_nothing_behind_the_clips_it_was_asked_for(rate):
    n = 3 * rate + 1
    x = _track(n)
    spans = [(0, n), (1, n), (7, n)]
    for pattern in A.PATTERNS:
        (length, (table, _, ar, clips)), = _gather(pattern, x, rate, spans, n_clips=4).items()
        assert table.shape[0] == 9 and ar.is_pattern(clips, start=4 * 4 * length), pattern


@pytest.mark.parametrize("rate", [16000, 44100])
def test_a_device_clip_table_that_disagrees_writes_less_never_elsewhere(rate):
    """The host copy is valid; rows of the device copy hold the poison itself, a start or a length past the track, a negative field.
    Those clips are unspecified (less of them is written); the rows that agree keep their bits, the guards hold."""
    n = 3 * rate + 1
    x = _track(n)
    spans = [(0, n), (1, n), (7, n)]
    (length, (_, want, _, _)), = _gather("zeros", x, rate, spans).items()
    want = want.view(9, length)
    for pattern, word in A.PATTERNS.items():
        poison = int(np.array([word | (word << 32)], dtype=np.uint64).view(np.int64)[0])
        bad = {0: (poison,) * 4, 2: (n + 5, 10, 0, 0), 4: (1, 2 ** 62, 2 ** 40, 0), 5: (-9, n, 0, 0), 7: (n - 3, 2 ** 40, 0, 0)}
        (_, (_, got, _, _)), = _gather(pattern, x, rate, spans, poison_rows={length: bad}).items()
        got = got.view(9, length)
        for c in (1, 3, 6, 8):
            assert torch.equal(got[c], want[c]), (pattern, c)


# ---- window sums -----------------------------------------------------------------------------------------------------------------
N = 20011


def _windows():
    return np.array([(0, N), (1, 8193), (3, 129), (N - 8200, 8200), (N - 1, 1), (7, 0), (N, 0), (5, 7), (2, 16389)], dtype=np.int64)


def _exact(x, table):
    sq = np.concatenate([[0], np.cumsum(np.square(x.astype(np.int64)))])
    return np.array([int(sq[a + m] - sq[a]) * 2.0 ** -30 for a, m in table.tolist()])


def _sums_arena(pattern, x, table_dev, out_elems):
    dev = _lib()[2]
    ar = A.GuardedArena(A.needed_bytes([x.nbytes, table_dev.nbytes, out_elems * 8]), dev, A.PATTERNS[pattern])
    return ar, ar.put(torch.from_numpy(x), "track"), ar.put(torch.from_numpy(table_dev), "windows"), ar.carve(out_elems * 8, "sums")


def _sums_call(ar, track, windows, sums, x, table_host, n_windows):
    lib, L, _ = _lib()
    status = lib.hmm_audio_pcm16_window_sums(ar.address(track), x.shape[0], table_host.ctypes.data, ar.address(windows), n_windows,
                                             ar.address(sums), L.stream_ptr())
    torch.cuda.synchronize()
    return status


def test_sums_guards_hold_and_sums_do_not_depend_on_the_poison():
    x, table = _track(N), _windows()
    want = _exact(x, table)
    for pattern in A.PATTERNS:
        ar, track, windows, sums = _sums_arena(pattern, x, table, len(table))
        assert _sums_call(ar, track, windows, sums, x, table, len(table)) == 0
        ar.check_guards()
        assert torch.equal(track.cpu(), torch.from_numpy(x).view(torch.uint8))                 # inputs are not written
        assert torch.equal(windows.cpu(), torch.from_numpy(table).view(torch.uint8).reshape(-1))
        assert np.array_equal(sums.cpu().numpy().view(np.uint64), want.view(np.uint64)), pattern


def test_nothing_is_written_outside_the_first_n_windows_sums():
    x, table = _track(N), _windows()
    want = _exact(x, table)
    for pattern in A.PATTERNS:
        ar, track, windows, sums = _sums_arena(pattern, x, table, len(table))
        assert _sums_call(ar, track, windows, sums, x, table, 4) == 0
        ar.check_guards()
        assert ar.is_pattern(sums, start=32), pattern
        assert np.array_equal(sums[:32].cpu().numpy().view(np.uint64), want[:4].view(np.uint64))
        assert _sums_call(ar, track, windows, sums, x, table, 0) == 0                          # and nothing at all for no windows
        assert ar.is_pattern(sums, start=32)


def test_a_device_window_table_poisoned_past_the_track_is_survived():
    x, table = _track(N), _windows()
    want = _exact(x, table)
    for pattern, word in A.PATTERNS.items():
        poison = np.array([word | (word << 32)], dtype=np.uint64).view(np.int64)[0]
        bad = table.copy()
        bad[0] = (poison, poison)
        bad[2] = (3, 2 ** 62)                                      # a length far past the track
        bad[4] = (N + 5, 10)                                       # a start past the track
        bad[5] = (-9, 100)                                         # a negative start
        bad[7] = (N - 3, 2 ** 40)
        ar, track, windows, sums = _sums_arena(pattern, x, bad, len(table))
        assert _sums_call(ar, track, windows, sums, x, table, len(table)) == 0
        ar.check_guards()
        assert torch.equal(track.cpu(), torch.from_numpy(x).view(torch.uint8))
        got = sums.cpu().numpy().view(np.float64)
        for k in (1, 3, 6, 8):
            assert got[k:k + 1].view(np.uint64).tolist() == want[k:k + 1].view(np.uint64).tolist(), (pattern, k)


def test_an_invalid_host_window_table_is_refused_with_nothing_written():
    lib = _lib()[0]
    x, table = _track(N), _windows()
    ar, track, windows, sums = _sums_arena("ones", x, table, len(table))
    for row in ((-1, 10), (0, N + 1), (N - 9, 10), (N + 1, 0), (5, -2), (2 ** 62, 2 ** 62)):
        bad = table.copy()
        bad[3] = row
        assert _sums_call(ar, track, windows, sums, x, bad, len(table)) == HMM_E_INVALID, row
        msg = lib.hmm_last_error()
        assert b"audio_pcm16_window_sums" in msg and b"outside the track" in msg, msg
        assert ar.is_pattern(sums), row
    ar.check_guards()
