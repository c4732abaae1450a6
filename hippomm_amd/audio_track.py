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

``AudioTrack.from_wav`` / ``from_pcm16`` keep the 16-bit samples of the WAV the reference's extraction step wrote
(batch_process.py:280-339) resident as they are, 2 bytes per sample instead of the 8 of ``np.load(audio.npy)``, and give every
output above the bits of the float64 track ``x / 32768.0`` through three entry points of their own:

    hmm_audio_pcm16_gather_clips   the gather with the loader (float)x * 2^-15 and without peaks (|x / 32768| <= 1: never scaled)
    hmm_audio_pcm16_window_sums    the exact sum of (x / 32768)^2 of a window of at most 2^22 samples, which any order gives
    hmm_segment_walk_pcm16         the device walk of segmentation.py over such a track

(tests/test_cpu_audio_pcm.py, tests/test_gpu_audio_pcm.py).
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


PCM_WINDOW_MAX = 1 << 22                            # the longest window whose sum of squares is exact on a 16-bit track
_PCM_SUBFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")           # KSDATAFORMAT_SUBTYPE_*: the GUID behind the tag


def read_wav_pcm16(path) -> Tuple[int, np.ndarray]:
    """A 16-bit PCM WAV file -> (sample_rate, samples): an int16 ``np.memmap`` of shape (n_frames, channels) over the file's
    ``data`` chunk (a plain empty int16 array when it holds no frame: nothing can be mapped).  Pure host.

    Its own RIFF walker: chunks it does not need (ffmpeg writes a ``LIST`` chunk before ``data``) are skipped, with the pad byte
    after a chunk of odd size.  Format tag 1, or WAVE_FORMAT_EXTENSIBLE with the PCM sub-format, at 16 bits.  A ``data`` size of
    0xFFFFFFFF (a streamed file) or one that reaches past the end of the file means "to the end of the file", whole frames only.
    Everything else raises ``ValueError`` naming what was found: RF64, another sample width or format tag, a block align other
    than 2 * channels, ``data`` before ``fmt ``, a file without ``data``."""
    import struct
    path = str(path)
    with open(path, "rb") as f:
        head = f.read(12)
        size = f.seek(0, 2)
        if len(head) < 12 or head[:4] not in (b"RIFF", b"RF64") or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF/WAVE file (it starts with {head[:12]!r})")
        if head[:4] == b"RF64":
            raise ValueError(f"{path}: RF64 files are not supported")
        fmt, at = None, 12
        while at + 8 <= size:
            f.seek(at)
            tag, n = struct.unpack("<4sI", f.read(8))
            body = at + 8
            if tag == b"fmt ":
                raw = f.read(min(n, 40))
                if n < 16 or len(raw) < 16:
                    raise ValueError(f"{path}: a fmt chunk of {n} bytes")
                code, channels, rate, _, align, bits = struct.unpack("<HHIIHH", raw[:16])
                if code == 0xFFFE:                                            # WAVE_FORMAT_EXTENSIBLE: the tag is in the sub-format
                    if len(raw) < 40 or raw[26:40] != _PCM_SUBFORMAT_TAIL:
                        raise ValueError(f"{path}: WAVE_FORMAT_EXTENSIBLE with a fmt chunk of {n} bytes or an unknown sub-format")
                    code = struct.unpack("<H", raw[24:26])[0]
                fmt = (code, channels, rate, align, bits)
            elif tag == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: the data chunk comes before any fmt chunk")
                code, channels, rate, align, bits = fmt
                if code != 1:
                    raise ValueError(f"{path}: format tag {code}" + (" (IEEE float)" if code == 3 else "") + ", only PCM (1) is supported")
                if bits != 16:
                    raise ValueError(f"{path}: {bits}-bit samples, only 16-bit PCM is supported")
                if channels < 1 or align != 2 * channels:
                    raise ValueError(f"{path}: block align {align} with {channels} channels, 16-bit PCM has 2 * channels")
                if n == 0xFFFFFFFF or n > size - body:
                    n = size - body                                           # to the end of the file
                frames = n // align                                           # whole frames only
                if frames == 0:
                    return rate, np.empty((0, channels), dtype=np.int16)
                return rate, np.memmap(path, dtype="<i2", mode="r", offset=body, shape=(frames, channels))
            at = body + n + (n & 1)
    raise ValueError(f"{path}: no data chunk" + ("" if fmt else " and no fmt chunk"))


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
    by segment).  The track is uploaded in chunks through the package's pinned staging; the caller's array is not pinned.

    ``from_wav`` / ``from_pcm16`` build the track from the 16-bit samples of the extracted WAV instead and keep them resident as
    int16 (``pcm`` is True): every method then answers with the bits of the float64 track ``x / 32768.0``."""

    pcm = False                                     # True on a track of 16-bit samples (from_pcm16 / from_wav)

    def __init__(self, audio_data, sample_rate: int, device=None):
        self._open(sample_rate, device)
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
        self.samples = self._upload(np.ascontiguousarray(x), torch.float64 if self.dtype_code else torch.float32)

    def _open(self, sample_rate: int, device) -> None:
        if device is not None and torch.device(device).type != "cuda":
            raise ValueError(f"AudioTrack lives on a GPU, got device {device}")
        self.device = _lib.require_gpu()
        if device is not None and torch.device(device).index is not None:
            self.device = torch.device(device)
        self.sample_rate = int(sample_rate)
        self.orig, self.new = rate_ratio(self.sample_rate)

    @classmethod
    def from_pcm16(cls, samples, sample_rate: int, device=None) -> "AudioTrack":
        """The track of 16-bit PCM samples x -- int16 (n,) or (n, 1); any other dtype raises ``TypeError`` -- with the values
        sf.read gives them, x / 32768: in every output bit the track ``AudioTrack(x.astype(np.float64).reshape(-1, 1) / 32768.0,
        sample_rate)``, what the reference's extraction step makes of its 16-bit WAV (batch_process.py:280-339), but resident as
        int16: 2 bytes per sample read, staged and held instead of 8.  ``pcm`` is True, ``samples`` the int16 device tensor;
        ``source_dtype`` / ``source_shape`` / ``dtype_code`` are those of the float64 (n, 1) array it stands for, and
        ``as_float64`` returns slices of that array.  Why the bits agree: csrc/audio_track.hip, DESIGN.md section 14.

        (n, C > 1): ``samples.astype(np.float64) / 32768.0`` goes to the ordinary constructor, which mixes it down on the host --
        the same semantics without the compact layout (``pcm`` is False)."""
        x = np.asarray(samples.detach().cpu().numpy() if isinstance(samples, torch.Tensor) else samples)
        if x.dtype != np.int16:
            raise TypeError(f"from_pcm16 takes int16 samples, got {x.dtype} (a float array goes to AudioTrack(...))")
        if x.ndim not in (1, 2):
            raise ValueError(f"samples must be (n,) or (n, channels), got shape {x.shape}")
        if x.ndim == 2 and x.shape[1] != 1:
            return cls(x.astype(np.float64) / 32768.0, sample_rate, device)
        self = cls.__new__(cls)
        self._open(sample_rate, device)
        self.pcm = True
        self.n_samples = int(x.shape[0])
        self.source_dtype = np.dtype(np.float64)
        self.source_shape = (self.n_samples, 1)
        self.dtype_code = 1
        self.samples = self._upload(np.ascontiguousarray(x.reshape(-1)), torch.int16)    # a memmap stays one: chunks are read as they go up
        return self

    @classmethod
    def from_wav(cls, path, device=None) -> "AudioTrack":
        """``from_pcm16`` of a 16-bit PCM WAV file (``read_wav_pcm16``) at the file's own rate: the file is mapped and goes up chunk
        by chunk, without a full copy on the host."""
        rate, samples = read_wav_pcm16(path)
        return cls.from_pcm16(samples, rate, device)

    def as_float64(self, start: int = 0, stop=None) -> np.ndarray:
        """The host slice [start:stop] of the float64 (n, 1) array a PCM track stands for (a read-back and numpy's x / 32768.0),
        for callers that still need a segment's ``audio_data``."""
        if not self.pcm:
            raise TypeError("as_float64 is for a track of 16-bit samples (from_pcm16 / from_wav)")
        return self.samples[start:stop].cpu().numpy().astype(np.float64).reshape(-1, 1) / 32768.0

    def _upload(self, x: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
        dev_track = torch.empty(x.shape[0], dtype=dtype, device=self.device)
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
            if self.pcm:                             # fp64 sums of (x / 32768)^2, exact: the float64 track's bits (a window above 2^22 is refused)
                sums = torch.empty(table.shape[0], dtype=torch.float64, device=self.device)
                _lib.check(lib.hmm_audio_pcm16_window_sums(self.samples.data_ptr(), self.n_samples, table.ctypes.data,
                                                           table_dev.data_ptr(), table.shape[0], sums.data_ptr(), _lib.stream_ptr()),
                           "hmm_audio_pcm16_window_sums")
                return sums.cpu().numpy()
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
        """Clipped spans (S, 2) int64 -> (S,) fp32 on the device: max |x| of each span's narrowed samples (NaN if it holds one).
        On a 16-bit track: max |x / 32768|, at most 1.0."""
        lib = _lib.load()
        spans = np.ascontiguousarray(spans, dtype=np.int64)
        if self.pcm:                                 # never above 1.0, so no clip needs it: plain torch on the slices, off every hot path
            with torch.cuda.device(self.device):
                peaks = [self.samples[a:b].to(torch.int32).abs().max().to(torch.float32) * 2.0 ** -15 if b > a
                         else torch.zeros((), dtype=torch.float32, device=self.device) for a, b in spans.tolist()]
                return torch.stack(peaks) if peaks else torch.empty(0, dtype=torch.float32, device=self.device)
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
        peaks = None if self.pcm else self.span_peaks(clipped)                # a 16-bit track is never scaled: no peak pass
        out = []
        with torch.cuda.device(self.device):
            taps, width = (None, 0) if self.orig == self.new else _taps_device(self.orig, self.new, self.device)
            for length, (positions, table) in clip_tables(clipped, self.orig, self.new).items():
                table_dev = torch.from_numpy(table).to(self.device)
                clips = torch.empty(table.shape[0], length, dtype=torch.float32, device=self.device)
                if self.pcm:
                    _lib.check(lib.hmm_audio_pcm16_gather_clips(self.samples.data_ptr(), self.n_samples, table.ctypes.data,
                                                                table_dev.data_ptr(), table.shape[0], length, self.orig, self.new,
                                                                width, None if taps is None else taps.data_ptr(), clips.data_ptr(),
                                                                _lib.stream_ptr()), "hmm_audio_pcm16_gather_clips")
                    out.append((positions, clips))
                    continue
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
