"""The audio track of a video on the device: upload the waveform once, embed any list of its spans in one call.

Replaces the audio block of the reference's ``process_sequence`` loop (hippomm/core/hippocampal_memory.py:1198-1251), which per
segment slices the waveform, mixes it to mono (:1206), casts it to float32 (:1212), peak-normalises it (:1215-1216), writes a
temporary wav (:1219) and calls ``extract_features({'audio': [path]}, ['audio'])`` on that one file.  Here the track is uploaded
as it is (fp64 or fp32), and per call two kernels (csrc/audio_track.hip) produce the clip batch ``hmm_audio_fbank`` consumes:

    hmm_audio_span_peaks     max |x| per span over the narrowed samples, NaN-propagating like ``np.abs(x).max()``
    hmm_audio_gather_clips   narrow, divide by the peak when it exceeds 1, and -- for a track that is not at 16 kHz -- resample the
                             span as a file of its own (torchaudio's polyphase windowed sinc), computing only the samples inside
                             the three clips of ``preprocess._audio_clip_bounds``

At 16 kHz the clips carry the bits of the reference's wav round trip; at another rate each sample lies within the error bound of
a T-term fp32 dot product of the exact filter output (tests/test_gpu_audio_track.py).  The host does what is left: the mix-down
of a multi-channel track (once, the reference's own expression) and the span / clip tables.

The same resident track serves the audio-level scan of ``_segment_sequence`` (hippocampal_memory.py:993-1000, :1061-1077), which
comes before the spans exist: ``AudioTrack.window_levels`` takes the 500 ms windows of a walk step, one launch of

    hmm_audio_window_sums    per window the sum of squares in the track's dtype, in the order of numpy's np.mean(np.square(x))

and one read-back, and forms the levels on the host with numpy scalars of that dtype (``levels_from_sums``): the bits of the
reference's expression on the host slices (tests/test_cpu_audio_levels_model.py, tests/test_gpu_audio_levels.py).
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, _pinned
from .preprocess import (AUDIO_CLIPS_PER_VIDEO, AUDIO_MEL_BINS, AUDIO_SAMPLE_RATE, AUDIO_TARGET_LENGTH, _audio_clip_bounds,
                         _resample_kernel, melspec_clips_device)

UPLOAD_CHUNK_BYTES = 16 << 20                       # two pinned buffers of this size per device carry a track of any length

_track_staging = {}                                 # (device, 0 | 1) -> PinnedStage of UPLOAD_CHUNK_BYTES bytes
_taps = {}                                          # (orig, new, device) -> tap-major (T, new) fp32 table on the device


def spans_of(segments, sample_rate: int) -> List[Tuple[int, int]]:
    """Objects with start_time / end_time (seconds) -> sample spans, as the reference forms them: int(t * sample_rate) (:1105-1107)."""
    return [(int(s.start_time * sample_rate), int(s.end_time * sample_rate)) for s in segments]


def rate_ratio(sample_rate: int) -> Tuple[int, int]:
    """(orig, new): the track's rate and 16 kHz, both divided by their gcd (torchaudio.functional.resample)."""
    sample_rate = int(sample_rate)
    if sample_rate < 1:
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    g = math.gcd(sample_rate, AUDIO_SAMPLE_RATE)
    return sample_rate // g, AUDIO_SAMPLE_RATE // g


def clip_spans(spans: Sequence[Tuple[int, int]], track_len: int) -> np.ndarray:
    """spans -> (S, 2) int64, each clipped to the track as the numpy slice audio_data[start:end] would.  Negative indices and a
    span that is empty after clipping raise ValueError (the reference raises on the empty one too: max() of an empty array)."""
    out = np.empty((len(spans), 2), dtype=np.int64)
    for i, (a, b) in enumerate(spans):
        a, b = int(a), int(b)
        if a < 0 or b < 0:
            raise ValueError(f"span {i} = ({a}, {b}): negative sample indices are not supported")
        a, b = min(a, track_len), min(b, track_len)
        if b <= a:
            raise ValueError(f"span {i} = ({int(spans[i][0])}, {int(spans[i][1])}) is empty on a track of {track_len} samples")
        out[i] = (a, b)
    return out


def resampled_length(n: int, orig: int, new: int) -> int:
    """Samples of an n-sample span at 16 kHz: ceil(new * n / orig), what resample_waveform returns."""
    return n if orig == new else -(-new * n // orig)


def clip_tables(spans: np.ndarray, orig: int, new: int) -> Dict[int, Tuple[List[int], np.ndarray]]:
    """Clipped spans (S, 2) -> {clip length: (span positions, table)}.  table: int64 (3 * len(positions), 4), row 3 * i + c =
    (span start, span length, first output sample of clip c, span index) for span positions[i], with the clips at
    _audio_clip_bounds(length at 16 kHz, 16000).  The three clips of a span are equally long (2 s, or the whole span when it is
    shorter), so spans group by clip length as the file route's clips do."""
    groups: Dict[int, Tuple[List[int], List[Tuple[int, int, int, int]]]] = {}
    for s, (a, b) in enumerate(spans.tolist()):
        bounds = _audio_clip_bounds(resampled_length(b - a, orig, new), AUDIO_SAMPLE_RATE)
        lengths = {e - f for f, e in bounds}
        if len(lengths) != 1:
            raise AssertionError(f"clips of unequal length {bounds}")
        positions, rows = groups.setdefault(lengths.pop(), ([], []))
        positions.append(s)
        rows += [(a, b - a, f, s) for f, _ in bounds]
    return {length: (positions, np.asarray(rows, dtype=np.int64).reshape(-1, 4)) for length, (positions, rows) in groups.items()}


def window_table(starts: Sequence[int], window: int, track_len: int) -> np.ndarray:
    """Window starts -> (W, 2) int64 (start, length), each clipped to the track as the numpy slice audio_data[lo:lo + window]
    would (a window past the track's end is empty).  Negative starts or a negative window raise ValueError."""
    window = int(window)
    if window < 0:
        raise ValueError(f"window must not be negative, got {window}")
    out = np.empty((len(starts), 2), dtype=np.int64)
    for i, lo in enumerate(starts):
        lo = int(lo)
        if lo < 0:
            raise ValueError(f"window {i} starts at {lo}: negative sample indices are not supported")
        a = min(lo, track_len)
        out[i] = (a, min(lo + window, track_len) - a)
    return out


def levels_from_sums(sums: np.ndarray, counts: Sequence[int]) -> list:
    """Sums of squares (dtype T) and sample counts -> the levels ``segmentation.audio_level`` returns for those windows, as it
    returns them: 20 * np.log10(rms), a scalar of dtype T, if rms > 0, else the int -100 -- with rms = np.sqrt(T(sum / n)),
    which is np.sqrt(np.mean(...)).  An all-zero window, one that holds a NaN and an empty one (0 / 0) have no rms > 0: -100,
    what the host expression gives (there with numpy's warnings for the empty one)."""
    out = []
    with np.errstate(all="ignore"):
        for s, n in zip(sums, counts):
            mean = s.dtype.type(s / np.intp(n))                               # np.mean's own expression; 0 / 0 = nan
            rms = np.sqrt(mean)
            out.append(20 * np.log10(rms) if rms > 0 else -100)
    return out


def _taps_device(orig: int, new: int, dev: torch.device) -> Tuple[torch.Tensor, int]:
    key = (orig, new, str(dev))
    if key not in _taps:
        kernels, width = _resample_kernel(orig, new)                          # (new, 1, T): phase-major
        _taps[key] = (kernels[:, 0].t().contiguous().to(dev), width)          # (T, new): a wave's lanes read consecutive floats
    return _taps[key]


class AudioTrack:
    """A video's waveform on the device.  audio_data: what np.load of the reference's audio.npy yields -- float64 (n, 1) -- or
    (n,) / (n, C), float32 or float64 (any other dtype is cast with astype(np.float32) first).  C > 1 is mixed down once on the
    host with the reference's own expression, audio_data.mean(axis=1) (:1206; row-wise, so the whole track at once equals segment
    by segment).  The track is uploaded in chunks through the package's pinned staging; the caller's array is not pinned."""

    def __init__(self, audio_data, sample_rate: int, device=None):
        if device is not None and torch.device(device).type != "cuda":
            raise ValueError(f"AudioTrack lives on a GPU, got device {device}")
        self.device = _lib.require_gpu()
        if device is not None and torch.device(device).index is not None:
            self.device = torch.device(device)
        self.sample_rate = int(sample_rate)
        self.orig, self.new = rate_ratio(self.sample_rate)
        if isinstance(audio_data, torch.Tensor):
            audio_data = audio_data.detach().cpu().numpy()
        x = np.asarray(audio_data)
        self.source_dtype = x.dtype                 # window_levels refuses a track that was not float32 / float64 at its source
        self.source_shape = tuple(x.shape)          # checkpoint.py writes a memory's waveform from the track only if this is (n,) / (n, 1)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float32)
        if x.ndim == 2:
            x = x.reshape(-1) if x.shape[1] == 1 else x.mean(axis=1)
        elif x.ndim != 1:
            raise ValueError(f"audio_data must be (n,) or (n, channels), got shape {x.shape}")
        self.n_samples = int(x.shape[0])
        self.dtype_code = 1 if x.dtype == np.float64 else 0
        self.samples = self._upload(np.ascontiguousarray(x))

    def _upload(self, x: np.ndarray) -> torch.Tensor:
        dev_track = torch.empty(x.shape[0], dtype=torch.float64 if self.dtype_code else torch.float32, device=self.device)
        src, dst = x.view(np.uint8), dev_track.view(torch.uint8)
        with torch.cuda.device(self.device):
            for k, lo in enumerate(range(0, src.shape[0], UPLOAD_CHUNK_BYTES)):
                hi = min(lo + UPLOAD_CHUNK_BYTES, src.shape[0])
                st = _pinned.stage(_track_staging, (str(self.device), k & 1), (UPLOAD_CHUNK_BYTES,))
                st.wait()                            # the copy issued from this buffer two chunks ago has left it
                st.host[:hi - lo] = src[lo:hi]
                dst[lo:hi].copy_(st.pinned[:hi - lo], non_blocking=True)
                st.mark()
        return dev_track

    # ---- levels -----------------------------------------------------------------------------------------------------------
    def window_sums(self, table: np.ndarray) -> np.ndarray:
        """Clipped windows (W, 2) int64 (start, length) -> (W,) sums of squares on the host, in the track's dtype and in numpy's
        summation order (hmm_audio_window_sums): one launch, one read-back."""
        lib = _lib.load()
        table = np.ascontiguousarray(table, dtype=np.int64)
        np_dtype = np.float64 if self.dtype_code else np.float32
        if table.shape[0] == 0:
            return np.empty(0, dtype=np_dtype)
        with torch.cuda.device(self.device):
            table_dev = torch.from_numpy(table).to(self.device)
            sums = torch.empty(table.shape[0], dtype=self.samples.dtype, device=self.device)
            _lib.check(lib.hmm_audio_window_sums(self.samples.data_ptr(), self.dtype_code, self.n_samples, table.ctypes.data,
                                                 table_dev.data_ptr(), table.shape[0], sums.data_ptr(), _lib.stream_ptr()),
                       "hmm_audio_window_sums")
            return sums.cpu().numpy()

    def window_level_values(self, starts: Sequence[int], window: int) -> list:
        """The level of audio_data[lo:lo + window] for every lo in starts, each the very object ``segmentation.audio_level``
        returns for that slice (a numpy scalar of the track's dtype, or the int -100)."""
        if self.source_dtype not in (np.float32, np.float64):
            raise TypeError(f"window_levels needs a track that was float32 or float64 at its source, got {self.source_dtype}: "
                            "the reference's level of such an array is a different computation (keep it on the host route)")
        table = window_table(starts, window, self.n_samples)
        return levels_from_sums(self.window_sums(table), table[:, 1].tolist())

    def window_levels(self, starts: Sequence[int], window: int) -> np.ndarray:
        """dB levels of the windows [lo, lo + window) for lo in starts, clipped to the track, in the track's dtype: bit for bit
        what ``segmentation.audio_level`` gives on the host slices of the array this track was made from."""
        return np.asarray(self.window_level_values(starts, window), dtype=np.float64 if self.dtype_code else np.float32)

    # ---- clips ------------------------------------------------------------------------------------------------------------
    def span_peaks(self, spans: np.ndarray) -> torch.Tensor:
        """Clipped spans (S, 2) int64 -> (S,) fp32 on the device: max |x| of each span's narrowed samples (NaN if it holds one)."""
        lib = _lib.load()
        spans = np.ascontiguousarray(spans, dtype=np.int64)
        with torch.cuda.device(self.device):
            spans_dev = torch.from_numpy(spans).to(self.device)
            peaks = torch.empty(spans.shape[0], dtype=torch.float32, device=self.device)
            _lib.check(lib.hmm_audio_span_peaks(self.samples.data_ptr(), self.dtype_code, self.n_samples, spans.ctypes.data,
                                                spans_dev.data_ptr(), spans.shape[0], peaks.data_ptr(), _lib.stream_ptr()),
                       "hmm_audio_span_peaks")
        return peaks

    def segment_clips(self, spans: Sequence[Tuple[int, int]]) -> List[Tuple[List[int], torch.Tensor]]:
        """spans [(start_sample, end_sample), ...] -> one (positions, clips) per clip length: clips (3 * len(positions), clip_len)
        fp32 on the device, mono at 16 kHz, rows 3 * i .. 3 * i + 2 the clips of span positions[i]."""
        lib = _lib.load()
        clipped = clip_spans(spans, self.n_samples)
        if clipped.shape[0] == 0:
            return []
        peaks = self.span_peaks(clipped)
        out = []
        with torch.cuda.device(self.device):
            taps, width = (None, 0) if self.orig == self.new else _taps_device(self.orig, self.new, self.device)
            for length, (positions, table) in clip_tables(clipped, self.orig, self.new).items():
                table_dev = torch.from_numpy(table).to(self.device)
                clips = torch.empty(table.shape[0], length, dtype=torch.float32, device=self.device)
                _lib.check(lib.hmm_audio_gather_clips(self.samples.data_ptr(), self.dtype_code, self.n_samples, table.ctypes.data,
                                                      table_dev.data_ptr(), table.shape[0], peaks.data_ptr(), clipped.shape[0],
                                                      length, self.orig, self.new, width,
                                                      None if taps is None else taps.data_ptr(), clips.data_ptr(),
                                                      _lib.stream_ptr()), "hmm_audio_gather_clips")
                out.append((positions, clips))
        return out

    def melspec(self, spans: Sequence[Tuple[int, int]]) -> torch.Tensor:
        """spans -> (S, 3, 1, 128, 204) fp32 on the device, in span order: what load_and_transform_audio_data_device returns for the
        wav files the reference would have written for these spans."""
        n = len(spans)
        out = torch.empty(n, AUDIO_CLIPS_PER_VIDEO, 1, AUDIO_MEL_BINS, AUDIO_TARGET_LENGTH, dtype=torch.float32, device=self.device)
        groups = self.segment_clips(spans)
        with torch.cuda.device(self.device):
            if len(groups) == 1:
                melspec_clips_device(groups[0][1], out=out)
                return out
            flat = out.view(n * AUDIO_CLIPS_PER_VIDEO, AUDIO_MEL_BINS, AUDIO_TARGET_LENGTH)
            for positions, clips in groups:
                rows = [AUDIO_CLIPS_PER_VIDEO * p + c for p in positions for c in range(AUDIO_CLIPS_PER_VIDEO)]
                flat[torch.tensor(rows, device=self.device)] = melspec_clips_device(clips)
        return out
