"""Sequence segmentation on MI355X -- drop-ins for

    _compute_frame_similarity     <- hippomm/core/hippocampal_memory.py:980-991
    _segment_sequence             <- hippomm/core/hippocampal_memory.py:1002-1114 (segment_sequence: the same as a function)

The other stages of the formation frame path have modules of their own -- ``ssim``, ``resize``, ``frame_cache``, ``frame_extraction``,
and ``retrieval`` for the recall dedup walk -- and their public names still import from here (the block at the end of this file).

The window walk of ``_segment_sequence`` is a pure host function of the scores (``walk_segments``); the GPU scorer behind it is
``frame_cache.PathScorer``, which raises a pair's error only when the walk consults that pair, where the reference raises it.

The audio-level scan of the walk (500 ms windows from the end of a step backwards) has two routes, chosen by the caller.  Given
only the ndarray, it is the reference's numpy expression on the host (``audio_level``), and an audio-only call needs no GPU.
Given ``audio_track=``, the video's ``AudioTrack``, the levels of all windows of a step come from one ``AudioTrack.window_levels``
call (``hmm_audio_window_sums``), bit for bit the levels of the host route, so the segment list is the same.

``segment_sequence(..., walk="device")``, opt-in, takes the walk itself to the device (``hmm_segment_walk``, csrc/segment_walk.hip):
every adjacent pair is scored into one device array (``PathScorer.score_adjacent``) and the segment list is the one read-back.

Deliberate deviations from the reference, documented on the functions: ``_segment_sequence`` raises ``ValueError`` where the
reference would loop forever; an unreadable image raises ``OSError`` naming the path where the reference raises ``cv2.error``.
There is no CPU fallback for the SSIM: without a GPU these calls raise ``HippoMMHipError``.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Callable, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .frame_cache import PathScorer

# the reference's __init__ defaults (hippocampal_memory.py:263-266)
MAX_SEGMENT_DURATION, MIN_SEGMENT_DURATION = 10.0, 5.0
FRAME_SIMILARITY_THRESHOLD, AUDIO_SILENCE_THRESHOLD = 0.95, -40


@dataclass
class SequenceSegment:
    """The fields of the reference's SequenceSegment (hippocampal_memory.py:36-42)."""
    start_time: float
    end_time: float
    frames: Optional[List[str]] = None
    audio_data: Optional[np.ndarray] = None
    frame_times: Optional[List[float]] = None


def _compute_frame_similarity(self, frame1_path: str, frame2_path: str) -> float:
    """Drop-in for ``HippocampalMemory._compute_frame_similarity`` (assign it on the class; ``self`` is unused): SSIM of the two
    files' gray frames with data_range = max - min of the first.  Pillow decodes (the reference uses cv2.imread); an unreadable
    file raises ``OSError`` naming its path, frames of different shapes or under 7x7 raise ``ValueError`` as skimage does."""
    return next(iter(PathScorer().score([(frame1_path, frame2_path)])))


def audio_level(audio_data: np.ndarray, sample_rate: int):
    """RMS level in dB with the reference's numpy expression (hippocampal_memory.py:993-1000), so levels are bit-identical."""
    if len(audio_data.shape) > 1:
        audio_data = audio_data.mean(axis=1)
    rms = np.sqrt(np.mean(np.square(audio_data)))
    return 20 * np.log10(rms) if rms > 0 else -100


def walk_segments(video_frames, frame_times, audio_data, audio_sample_rate,
                  score_window: Callable[[List[Tuple[int, int]]], Iterable[float]],
                  max_segment_duration: float = MAX_SEGMENT_DURATION, min_segment_duration: float = MIN_SEGMENT_DURATION,
                  frame_similarity_threshold: float = FRAME_SIMILARITY_THRESHOLD,
                  audio_silence_threshold: float = AUDIO_SILENCE_THRESHOLD, *, audio_track=None) -> List[SequenceSegment]:
    """The window walk of ``_segment_sequence`` as a host function of the scores.  ``score_window(pairs)`` gets one window's pairs
    of frame indices (later, earlier) -- adjacent entries of the window's frame list, scanned from the end -- and yields their
    similarities in that order; the walk stops reading at the first score below the threshold (NaN never breaks).

    Behaviour of the reference kept: the walk starts at 0.0 whatever frame_times[0] is; a frame is in a window when
    start <= t <= end; the audio scan (500 ms windows, from the end backwards, excluding offset 0) runs after the video scan and
    overrides it; then the minimum-duration clamp; segment contents take inclusive time bounds and audio samples
    int(start * sr):int(end * sr).  One deviation: where the reference would loop forever (a start it has already been at, which
    only happens with min_segment_duration <= 0), this raises ValueError.

    ``audio_track`` (an ``audio_track.AudioTrack`` of the same waveform): the levels of a step's windows come from one
    ``window_level_values`` call over all of the step's window starts instead of one host expression per window -- the same
    objects, so the same segments; the level is a pure function of the window, and the first window from the end below the
    threshold still decides.  Its rate must be ``audio_sample_rate`` (ValueError).  ``audio_data`` may then be None: the track's
    length stands in for ``len(audio_data)`` and ``seg.audio_data`` is None (form spans with ``audio_track.spans_of``)."""
    segments: List[SequenceSegment] = []
    if audio_track is not None:
        if audio_track.sample_rate != audio_sample_rate:
            raise ValueError(f"audio_track is at {audio_track.sample_rate} Hz, audio_sample_rate is {audio_sample_rate}")
        if audio_data is not None and len(audio_data) != audio_track.n_samples:
            raise ValueError(f"audio_track holds {audio_track.n_samples} samples, audio_data {len(audio_data)}")
    if video_frames is None and audio_data is None and audio_track is None:
        return segments
    has_video = bool(video_frames and frame_times)
    has_audio = (audio_data is not None or audio_track is not None) and bool(audio_sample_rate)
    if has_video:
        total_duration = frame_times[-1] - frame_times[0]
    elif has_audio:
        total_duration = (len(audio_data) if audio_data is not None else audio_track.n_samples) / audio_sample_rate
    else:
        return segments

    current_start = 0.0
    seen = set()
    while current_start < total_duration:
        if current_start in seen:
            raise ValueError(f"segmentation makes no progress at t = {current_start} (min_segment_duration = "
                             f"{min_segment_duration}); the reference would loop forever here")
        seen.add(current_start)
        current_end = min(current_start + max_segment_duration, total_duration)
        optimal_end = current_end

        if has_video:
            inside = [i for i, t in enumerate(frame_times) if current_start <= t <= current_end]
            if len(inside) > 1:
                pairs = [(inside[k], inside[k - 1]) for k in range(len(inside) - 1, 0, -1)]
                for (later, _), similarity in zip(pairs, score_window(pairs)):
                    if similarity < frame_similarity_threshold:
                        optimal_end = frame_times[later]
                        break

        if has_audio:
            start_sample = int(current_start * audio_sample_rate)
            end_sample = int(current_end * audio_sample_rate)
            window = int(0.5 * audio_sample_rate)
            if audio_track is not None:                      # every window of this step in one launch
                starts = [start_sample + off for off in range(end_sample - start_sample - window, 0, -window)]
                resident = dict(zip(starts, audio_track.window_level_values(starts, window)))
            for off in range(end_sample - start_sample - window, 0, -window):
                lo = start_sample + off
                level = resident[lo] if audio_track is not None else audio_level(audio_data[lo:lo + window], audio_sample_rate)
                if level < audio_silence_threshold:
                    optimal_end = lo / audio_sample_rate
                    break

        if optimal_end - current_start < min_segment_duration:
            optimal_end = min(current_start + min_segment_duration, total_duration)

        seg = SequenceSegment(start_time=current_start, end_time=optimal_end)
        if has_video:
            seg.frames = [f for f, t in zip(video_frames, frame_times) if current_start <= t <= optimal_end]
            seg.frame_times = [t for t in frame_times if current_start <= t <= optimal_end]
        if has_audio and audio_data is not None:
            seg.audio_data = audio_data[int(current_start * audio_sample_rate):int(optimal_end * audio_sample_rate)]
        segments.append(seg)
        current_start = optimal_end
    return segments


def _window_scorer(video_frames, scorer: PathScorer):
    """score_window for walk_segments on the GPU: the window's last pair alone first (at threshold 0.95 it usually breaks), then,
    if it did not, the rest of the window in one launch."""
    def score_window(pairs):
        paths = [(video_frames[a], video_frames[b]) for a, b in pairs]
        yield from scorer.score(paths[:1])
        if len(paths) > 1:
            yield from scorer.score(paths[1:])
    return score_window


# hmm_segment_record and hmm_segment_walk_state of include/hippomm_hip.h
SEGMENT_RECORD = np.dtype([("start_time", "<f8"), ("end_time", "<f8"), ("first_frame", "<i4"), ("last_frame", "<i4"),
                           ("cut_pair", "<i4"), ("cut_window", "<i4"), ("pairs_consulted", "<i4"), ("windows_consulted", "<i4")])
SEGMENT_STATE = np.dtype([("n_segments", "<i4"), ("status", "<i4"), ("flagged_pair", "<i4"), ("steps", "<i4"),
                          ("current_start", "<f8")])
WALK_DONE, WALK_FLAGGED, WALK_BOUND = 1, 2, 3       # HMM_SEGMENT_WALK_*
MAX_DEVICE_STEPS = 4096                             # two launches per step with audio: beyond this the host walks
MAX_DEVICE_WINDOWS = 65535                          # windows of one step (one workgroup each)


def _silent_on_host(rms, threshold) -> bool:
    """The host route's decision for a window whose rms is the numpy scalar `rms`: ``audio_level``'s last line, then the walk's
    comparison, with the very objects the host route compares."""
    with np.errstate(all="ignore"):
        return bool((20 * np.log10(rms) if rms > 0 else -100) < threshold)


@lru_cache(maxsize=64)
def _silence_cut(dtype_name: str, threshold, _threshold_type) -> Tuple[float, bool]:
    T = np.dtype(dtype_name).type
    U = np.uint32 if T is np.float32 else np.uint64
    value = lambda bits: U(bits).view(T)                                      # noqa: E731
    lo, hi = 1, int(T(np.inf).view(U))                                        # positive floats in the order of their bit patterns
    if _silent_on_host(value(hi), threshold):
        raise AssertionError(f"silence_cut: an infinite rms is silent under threshold {threshold!r}")
    while lo < hi:                                                            # the least pattern that is not silent
        mid = (lo + hi) // 2
        if _silent_on_host(value(mid), threshold):
            lo = mid + 1
        else:
            hi = mid
    cut = value(lo)
    if _silent_on_host(cut, threshold) or (lo > 1 and not _silent_on_host(value(lo - 1), threshold)):
        raise AssertionError(f"silence_cut: the level is not monotonic around rms = {cut!r} for threshold {threshold!r}")
    return float(cut), bool(-100 < threshold)


def silence_cut(dtype, threshold) -> Tuple[float, bool]:
    """The silence rule of the walk without a logarithm: -> (rms_cut, silent_without_rms) such that, for an rms of `dtype`
    (float32 or float64), ``(20 * np.log10(rms) if rms > 0 else -100) < threshold`` is ``rms < rms_cut if rms > 0 else
    silent_without_rms``.  rms_cut is found by bisection over the bit patterns of the positive floats with this host's own scalar
    expression, and checked: the float below it is silent, it is not (``AssertionError`` otherwise -- a log10 that is not
    monotonic there).  Cached per (dtype, threshold)."""
    return _silence_cut(np.dtype(dtype).name, threshold, type(threshold))


def _device_walk(video_frames, frame_times, audio_data, audio_sample_rate, max_segment_duration, min_segment_duration,
                 frame_similarity_threshold, audio_silence_threshold, scorer, audio_track, stats: dict):
    """The walk by ``hmm_segment_walk`` -> the segments, or a str: why this call stays on the host route."""
    has_video = bool(video_frames and frame_times)
    has_audio = (audio_data is not None or audio_track is not None) and bool(audio_sample_rate)
    if not has_video and not has_audio:
        return "nothing to segment"
    if has_audio and audio_track is None:
        raise ValueError("walk='device' needs the video's AudioTrack (audio_track=) when there is audio")
    params = (max_segment_duration, min_segment_duration, frame_similarity_threshold, audio_silence_threshold)
    if any(p != p for p in params) or not all(np.isfinite(p) for p in params[:2]):
        return "NaN parameters"
    if not min_segment_duration > 0:
        return "min_segment_duration <= 0"
    times = np.empty(0)
    if has_video:
        if len(video_frames) != len(frame_times) or not all(isinstance(t, float) for t in frame_times):
            return "frame_times are not one float per frame"
        times = np.asarray(frame_times, dtype=np.float64)
        if not np.all(np.isfinite(times)) or np.any(times[1:] < times[:-1]):
            return "unsorted frame_times"
        total = frame_times[-1] - frame_times[0]
    rate = 0
    if has_audio:
        if audio_track.sample_rate != audio_sample_rate or (audio_data is not None and len(audio_data) != audio_track.n_samples):
            return "audio_track does not match the call"                       # the host route raises the ValueError
        if audio_track.source_dtype not in (np.float32, np.float64):
            return "track not float32 / float64 at its source"
        rate = int(audio_sample_rate)
        if rate != audio_sample_rate or rate < 2:
            return "sample rate not an integer >= 2"
        if not has_video:
            total = audio_track.n_samples / audio_sample_rate
    if not np.isfinite(total) or (has_audio and not total * rate < 2.0 ** 52):
        return "duration out of range"
    span = min(max_segment_duration, max(total, 0.0))                          # no step is longer, up to rounding
    window = int(0.5 * rate)
    if has_audio and getattr(audio_track, "pcm", False) and window > (1 << 22):
        return "a window above 2^22 samples on a 16-bit track"
    if not total / min_segment_duration < MAX_DEVICE_STEPS or (has_audio and not span * rate / window < MAX_DEVICE_WINDOWS):
        return "more steps or windows than the device route launches"
    max_steps = max(int(np.ceil(total / min_segment_duration)), 0) + 2         # a clamped step advances by min, or reaches the end
    max_windows = int((span * rate + 2) // window) + 1 if has_audio else 0

    lib = _lib.load()
    dev = audio_track.device if has_audio else scorer.dev
    rms_cut, silent_without_rms = silence_cut(np.float64 if audio_track.dtype_code else np.float32,
                                              audio_silence_threshold) if has_audio else (0.0, False)
    problems: List[Optional[Exception]] = []
    scores = flags = times_dev = None
    with torch.cuda.device(dev):
        if has_video:
            scores, problems = scorer.score_adjacent(video_frames)
            scores = scores.to(dev)
            flags = torch.tensor([p is not None for p in problems], dtype=torch.int32).to(dev)
            times_dev = torch.from_numpy(times).to(dev)
        ws = torch.empty(max(lib.hmm_segment_walk_workspace_bytes(max_windows, max_steps), 256), dtype=torch.uint8, device=dev)
        out = torch.empty(max_steps * SEGMENT_RECORD.itemsize + SEGMENT_STATE.itemsize, dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
        head = (ptr(scores), ptr(flags), ptr(times_dev), times.ctypes.data if has_video else None, len(times),
                audio_track.samples.data_ptr() if has_audio else None)
        rest = (audio_track.n_samples if has_audio else 0, rate, float(total), float(max_segment_duration), float(min_segment_duration),
                float(frame_similarity_threshold), rms_cut, int(silent_without_rms), max_windows, max_steps, out.data_ptr(),
                out.data_ptr() + max_steps * SEGMENT_RECORD.itemsize, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        if has_audio and getattr(audio_track, "pcm", False):                   # int16 samples: the entry point without a track_dtype
            _lib.check(lib.hmm_segment_walk_pcm16(*head, *rest), "hmm_segment_walk_pcm16")
        else:
            _lib.check(lib.hmm_segment_walk(*head, audio_track.dtype_code if has_audio else 0, *rest), "hmm_segment_walk")
        host = out.cpu().numpy()                                               # the one read-back
    state = host[max_steps * SEGMENT_RECORD.itemsize:].view(SEGMENT_STATE)[0]
    records = host[:int(state["n_segments"]) * SEGMENT_RECORD.itemsize].view(SEGMENT_RECORD)
    stats.update(steps=int(state["steps"]), launches=2 * max_steps + 1 if has_audio else 1, read_backs=1,
                 pairs_scored=len(problems) - sum(p is not None for p in problems),
                 pairs_consulted=int(records["pairs_consulted"].sum()), windows_consulted=int(records["windows_consulted"].sum()))
    if state["status"] == WALK_FLAGGED:
        raise problems[int(state["flagged_pair"])]
    if state["status"] != WALK_DONE:
        return "step bound exhausted"
    segments = []
    for rec in records:
        start, end = float(rec["start_time"]), float(rec["end_time"])
        seg = SequenceSegment(start_time=start, end_time=end)
        if has_video:                                                          # the frames with start <= t <= end: one index range
            inside = slice(int(rec["first_frame"]), int(rec["last_frame"]) + 1)
            seg.frames = list(video_frames[inside])
            seg.frame_times = list(frame_times[inside])
        if has_audio and audio_data is not None:
            seg.audio_data = audio_data[int(start * audio_sample_rate):int(end * audio_sample_rate)]
        segments.append(seg)
    return segments


def segment_sequence(video_frames: Optional[List[str]] = None, frame_times: Optional[List[float]] = None,
                     audio_data: Optional[np.ndarray] = None, audio_sample_rate: Optional[int] = None, *,
                     max_segment_duration: float = MAX_SEGMENT_DURATION, min_segment_duration: float = MIN_SEGMENT_DURATION,
                     frame_similarity_threshold: float = FRAME_SIMILARITY_THRESHOLD,
                     audio_silence_threshold: float = AUDIO_SILENCE_THRESHOLD,
                     scorer: Optional[PathScorer] = None, audio_track=None, walk: str = "host",
                     stats: Optional[dict] = None) -> List[SequenceSegment]:
    """``_segment_sequence`` as a function; the four parameters default to the reference's __init__ defaults.  Frame similarities
    come from the GPU (``PathScorer``).  Without ``audio_track`` an audio-only call needs no GPU (the audio scan is host numpy,
    as in the reference); with the video's ``AudioTrack`` the scan reads the resident track (see ``walk_segments``).

    ``walk="device"`` (opt-in; "host" is the default and is the route above, untouched) takes the control loop to the device as
    well: every adjacent pair is scored into one device array (``PathScorer.score_adjacent``), ``hmm_segment_walk`` walks it and
    the resident track, and the segment list is the one read-back -- the same segments: times equal as floats, the same frame
    lists, the same audio slices (times come back as Python floats; the frames of a segment are taken as one index range, which
    is what the reference's comprehension selects when the times are sorted).  It needs the video's ``audio_track`` when there
    is audio (``ValueError``).  It scores every pair, the host route only the consulted ones: with frames that are not in the
    cache yet it decodes them all.  A pair that cannot be scored raises its error only if the walk consults it, as on the host
    route.  Calls it does not take go the host route and say why in ``stats["reason"]``: unsorted or non-float frame_times, NaN
    parameters, min_segment_duration <= 0, a track that was not float32 / float64 at its source (a 16-bit track of
    ``AudioTrack.from_wav`` / ``from_pcm16`` stands for a float64 array and is walked by ``hmm_segment_walk_pcm16``), more steps than
    MAX_DEVICE_STEPS, a walk that did not finish within its step bound.  Measured on one MI355X with every input resident (600
    cached 1080p frames, a 600 s float64 track at 16 kHz, 80 segments; profiles/segment_walk.json): 9.4 ms
    against 31.3 ms for the host walk, 1 read-back against 226; uncached frames and other inputs were not measured.

    ``stats``: a dict that receives ``route`` ("host" / "device") and, from the device walk, ``steps``, ``launches``,
    ``read_backs``, ``pairs_scored``, ``pairs_consulted``, ``windows_consulted``; ``reason`` when a device call went to the host."""
    if walk not in ("host", "device"):
        raise ValueError(f"walk must be 'host' or 'device', got {walk!r}")
    stats = {} if stats is None else stats
    if video_frames and frame_times and scorer is None:
        scorer = PathScorer()
    if walk == "device":
        done = _device_walk(video_frames, frame_times, audio_data, audio_sample_rate, max_segment_duration, min_segment_duration,
                            frame_similarity_threshold, audio_silence_threshold, scorer, audio_track, stats)
        if not isinstance(done, str):
            stats["route"] = "device"
            return done
        stats["reason"] = done
    stats["route"] = "host"
    score_window = _window_scorer(video_frames, scorer) if scorer is not None else None
    return walk_segments(video_frames, frame_times, audio_data, audio_sample_rate, score_window,
                         max_segment_duration, min_segment_duration, frame_similarity_threshold, audio_silence_threshold,
                         audio_track=audio_track)


def _segment_sequence(self, video_frames: Optional[List[str]] = None, frame_times: Optional[List[float]] = None,
                      audio_data: Optional[np.ndarray] = None, audio_sample_rate: Optional[int] = None,
                      audio_track=None) -> List[SequenceSegment]:
    """Drop-in for ``HippocampalMemory._segment_sequence`` (assign it on the class): reads self.max_segment_duration,
    self.min_segment_duration, self.frame_similarity_threshold and self.audio_silence_threshold.  The video's ``AudioTrack``,
    given as the ``audio_track`` argument or set as ``self.audio_track``, moves the audio-level scan to the device;
    ``self.segment_walk = "device"`` moves the walk itself there (``segment_sequence``'s ``walk``; "host" when not set)."""
    if audio_track is None:
        audio_track = getattr(self, "audio_track", None)
    return segment_sequence(video_frames, frame_times, audio_data, audio_sample_rate,
                            max_segment_duration=self.max_segment_duration, min_segment_duration=self.min_segment_duration,
                            frame_similarity_threshold=self.frame_similarity_threshold,
                            audio_silence_threshold=self.audio_silence_threshold, audio_track=audio_track,
                            walk=getattr(self, "segment_walk", "host"))


# the public names of the other stages, importable from here as before
from .ssim import WIN, compute_frame_difference, gray_frames, ssim_pairs  # noqa: E402,F401
from .resize import RESIZE_AREA2X, RESIZE_COEF_SCALE, RESIZE_LINEAR, resize_frames, resize_linear_tables, resize_mode  # noqa: E402,F401
from .frame_cache import ADJACENT_CHUNK, CACHE_BYTES, UPLOAD_FRAMES, FrameCache, default_cache  # noqa: E402,F401
from .frame_extraction import (CHECK_INTERVAL, EXTRACT_BATCH, EXTRACT_RECORD, EXTRACT_STATE, MAX_DIFF_THRESHOLD,  # noqa: E402,F401
                               MIN_SAVE_GAP, SAVE_QUALITY, SAVE_SUBSAMPLING, ExtractionState, FrameExtractor, extract_frames,
                               extraction_records, save_frame, save_frames)
from .retrieval import RECALL_SIMILARITY_CUT, RECALL_SIZE, walk_recall_window  # noqa: E402,F401
