"""GPU: the memory contract of hmm_audio_span_peaks / hmm_audio_gather_clips in the guarded arena (tests/arena.py).  The track, the
span and clip tables, the taps, the peaks and the clip batch are carved at exactly their size; after the calls every guard still
holds its pattern, and peaks and clips are the same bits under all three patterns -- a sample read before the track's first,
behind its last (spans that start at sample 0 and 1 and end at the last sample; a track of 3 s + 1 sample, so that no 16-byte
load ends on its last byte) or an output left unwritten would differ between two of them."""
import numpy as np
import pytest
import torch

import arena as A
import audio_track_oracle as ato

pytestmark = pytest.mark.gpu


def _run(pattern, x, rate):
    from hippomm_amd import _lib
    from hippomm_amd.audio_track import clip_spans, clip_tables, rate_ratio
    from hippomm_amd.preprocess import _resample_kernel
    lib = _lib.load()
    dev = _lib.require_gpu()
    n = x.shape[0]
    dtype_code = 1 if x.dtype == np.float64 else 0
    orig, new = rate_ratio(rate)
    spans = clip_spans([(0, n), (1, n), (n - 32001, n)], n)
    tables = clip_tables(spans, orig, new)
    taps_host, width = (None, 0) if orig == new else _resample_kernel(orig, new)
    sizes = [x.nbytes, spans.nbytes, 4 * len(spans)]
    for length, (_, t) in tables.items():
        sizes += [t.nbytes, 4 * t.shape[0] * length]
    if taps_host is not None:
        sizes.append(taps_host.numel() * 4)
    ar = A.GuardedArena(A.needed_bytes(sizes), dev, A.PATTERNS[pattern])
    track = ar.put(torch.from_numpy(x), "track")
    spans_dev = ar.put(torch.from_numpy(spans), "spans")
    taps = None if taps_host is None else ar.put(taps_host[:, 0].t().contiguous(), "taps")
    peaks = ar.carve(4 * len(spans), "peaks")
    stream = _lib.stream_ptr()
    _lib.check(lib.hmm_audio_span_peaks(ar.address(track), dtype_code, n, spans.ctypes.data, ar.address(spans_dev), len(spans),
                                        ar.address(peaks), stream), "hmm_audio_span_peaks")
    clips = {}
    for length, (positions, table) in tables.items():
        table_dev = ar.put(torch.from_numpy(table), f"clips table {length}")
        out = ar.carve(4 * table.shape[0] * length, f"clips {length}")
        _lib.check(lib.hmm_audio_gather_clips(ar.address(track), dtype_code, n, table.ctypes.data, ar.address(table_dev),
                                              table.shape[0], ar.address(peaks), len(spans), length, orig, new, width,
                                              None if taps is None else ar.address(taps), ar.address(out), stream),
                   "hmm_audio_gather_clips")
        clips[length] = (positions, out)
    torch.cuda.synchronize()
    ar.check_guards()
    assert torch.equal(track.cpu(), torch.from_numpy(x).view(-1).view(torch.uint8))          # inputs are not written
    return peaks.clone().view(torch.int32).cpu(), {k: (p, o.clone().view(torch.int32).cpu()) for k, (p, o) in clips.items()}


@pytest.mark.parametrize("rate", [16000, 44100])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_guards_hold_and_results_do_not_depend_on_the_poison(dtype, rate):
    n = 3 * rate + 1
    x = np.ascontiguousarray(ato.make_track("f64_n", n=n, rate=rate, quiet=(rate, 2 * rate), seed=11).astype(dtype))
    runs = {pattern: _run(pattern, x, rate) for pattern in A.PATTERNS}
    first_peaks, first_clips = runs["ones"]
    x32 = x.astype(np.float32)
    want = np.array([np.abs(x32[a:n]).max() for a in (0, 1, n - 32001)], dtype=np.float32)
    assert np.array_equal(first_peaks.numpy().view(np.float32), want)
    assert len(first_clips) == (1 if rate == 16000 else 2)
    for pattern, (peaks, clips) in runs.items():
        assert torch.equal(peaks, first_peaks), pattern
        assert clips.keys() == first_clips.keys()
        for length, (positions, bits) in clips.items():
            assert torch.equal(bits, first_clips[length][1]), (pattern, length)
    if rate == 16000:                                             # and they are the recipe's bits
        from hippomm_amd.preprocess import _audio_clip_bounds
        (positions, bits), = first_clips.values()
        got = bits.numpy().view(np.float32).reshape(9, 32000)
        for i, a in enumerate((0, 1, n - 32001)):
            seg, _, _ = ato.resident_segment(x32, a, n)
            for c, (f, e) in enumerate(_audio_clip_bounds(n - a, 16000)):
                assert np.array_equal(got[3 * i + c].view(np.uint32), seg[f:e].view(np.uint32))
