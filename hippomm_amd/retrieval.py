"""The callers' retrieval step -- QARecallSystem._find_relevant_video_segments / _find_relevant_audio_segments
(hippomm/core/hippocampal_memory.py:3127-3279, :3281-3383) -- on a resident EventStore.

The reference loops over the events, scans each one (k = 5), and per event either turns the hits whose row is a KEPT row
(``idx < len(event.frame_times)`` / ``idx < len(event.feature_times['audio_times'])``) into +-1 s segments or, when the best
similarity is below 0.4 and the event has captions / a transcription, asks the LLM (entries at similarity 0.6, or the event's own
hits on an error).  All entries are then sorted by similarity (Python's stable sort) and the best 5 kept.

Here one ``EventStore.relevant_hits`` call applies both rules and the ranking on the device and returns the best ``keep`` feature
hits plus the deferred events with their own hits.  The LLM block stays the integrator's Python: ``deferred(event, idx, sims)``
returns that event's ``[(similarity, [segments])]`` entries.  The merge runs on the host over at most ``keep`` device hits and the
callables' entries; a feature hit among the final ``keep`` is among the best ``keep`` feature hits, so nothing is lost.

Limits: where NaN similarities sort is this library's rule (first), not Python's.  By default the similarities are fp32 results,
so on a store converted from float64 a 0.4 decision within 2e-6 of the threshold, and the order of hits whose cosines differ by
less than fp32 accumulation noise, can differ from the reference, which computes them in float64.  ``exact64=True`` takes the
float64 route for a store whose float64 source held fp32 values (a reloaded event does): similarities within 2^-42 of the exact
quotient in a fixed, documented summation order, the query's norm numpy's own, the two rules and the stable sort on doubles on the
host.  What stays this library's then: the order inside exact ties, and the last fp32 bit of the norm of a query that lives on the
device (include/hippomm_hip.h).  The default is unchanged.

``recall_window_frames`` is the step the reference takes next (:2210-2251 in ``_process_video_query``, :2773-2815 in
``_process_multimodal_query``, the same text): the frames of a +-1 s window around every frame_time of the segments found are
shrunk with ``cv2.resize(frame, (320, 180))``, written as JPEG and dropped when their SSIM with the last kept file of the window
is above 0.3.  Here the shrink, the files, their decoded pixels, the gray frames and the scores of all windows of a question are
made on the device in one pass; the walk is a host function of the scores.  A question's wall time is the caller's video seeks
and the captioner, not this arithmetic: the point is that no numeric step of the retrieval path is left on the host.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, jpeg
from .frame_cache import FrameCache
from .frame_extraction import SAVE_QUALITY, SAVE_SUBSAMPLING
from .resize import resize_frames, resize_mode
from .segmentation import SequenceSegment
from .ssim import WIN, gray_frames, ssim_launch, upload_frames
from .vector_ops import FEATURE_DIM, EventStore

logger = logging.getLogger(__name__)

_MODALITIES = {"vision": "frame_captions", "audio": "holistic_audio_transcription"}
_warned_no_callable = False


def _kept_times(event, modality: str):
    """The kept rows' times: the list whose length is the reference's row limit."""
    return event.frame_times if modality == "vision" else event.feature_times["audio_times"]


def _segment(event, row: int, modality: str) -> SequenceSegment:
    """The +-1 s segment the reference builds around kept row ``row`` (:3263-3271, :3371-3375)."""
    if modality == "vision":
        t = event.frame_times[row]
        return SequenceSegment(start_time=max(0, t - 1), end_time=t + 1,
                               frames=[event.frames[i] for i in range(len(event.frames))
                                       if event.frame_times[i] >= t - 1 and event.frame_times[i] <= t + 1],
                               frame_times=[u for u in event.frame_times if u >= t - 1 and u <= t + 1])
    times = event.feature_times["audio_times"]
    return SequenceSegment(start_time=max(0, times[row] - 1), end_time=times[row] + 1, audio_data=None)


def feature_entries(event, idx, sims, modality: str) -> List[Tuple[float, List[SequenceSegment]]]:
    """The ``(similarity, [segment])`` entries the reference builds from an event's own hits (:3261-3272, :3369-3376): the row rule,
    then the +-1 s segment.  What the error branch of the LLM block falls back to."""
    if modality not in _MODALITIES:
        raise ValueError(f"feature_entries: modality must be 'vision' or 'audio', got {modality!r}")
    limit = len(_kept_times(event, modality))
    return [(similarity, [_segment(event, int(row), modality)]) for row, similarity in zip(idx, sims) if row < limit]


def merge_entries(entries, keep: int) -> List[SequenceSegment]:
    """entries: [(similarity, event position, order inside the event, [segments])] -> the segments of the best ``keep`` entries.
    Similarity descending; equal similarities in event order, then in-event order -- what a stable sort of the reference's
    event-ordered list gives.  NaN first."""
    ordered = sorted(entries, key=lambda entry: (entry[1], entry[2]))
    ordered.sort(key=lambda entry: (0, 0.0) if entry[0] != entry[0] else (1, -float(entry[0])))
    out = []
    for entry in ordered[:keep]:
        out.extend(entry[3])
    return out


def _find(modality: str, events: Sequence, query_features, store: Optional[EventStore], deferred: Optional[Callable], k: int,
          keep: int, min_similarity: float, prefilter: bool, exact64: bool = False) -> List[SequenceSegment]:
    global _warned_no_callable
    what = f"find_relevant_{'video' if modality == 'vision' else 'audio'}_segments"
    query = query_features.detach().cpu().numpy() if isinstance(query_features, torch.Tensor) else np.asarray(query_features)
    query = query.reshape(-1)
    if modality == "vision" and query.shape[0] != FEATURE_DIM:
        logger.warning("Unexpected query feature dimension: %d, expected %d", query.shape[0], FEATURE_DIM)
        return []
    having = [event for event in events if modality in event.features]
    if not having:
        return []
    if store is None:
        store = EventStore([f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else f
                            for f in (event.features[modality] for event in having)])
    elif len(store.lengths) != len(having):
        raise ValueError(f"{what}: the store holds {len(store.lengths)} events, {len(having)} events have {modality} features")
    row_limits = [len(_kept_times(event, modality)) for event in having]
    defer = [bool(getattr(event, _MODALITIES[modality], None)) for event in having]
    hits, handed_back = store.relevant_hits(query, k, keep, row_limits=row_limits, defer=defer, min_similarity=min_similarity,
                                            prefilter=prefilter, exact64=exact64)
    entries = [(similarity, e, order, [_segment(having[e], row, modality)]) for order, (e, row, similarity) in enumerate(hits)]
    for e, idx, sims in handed_back:
        if deferred is None:
            if not _warned_no_callable:
                logger.warning("%s: no `deferred` callable was given; events below the similarity threshold are answered from "
                               "their own hits", what)
                _warned_no_callable = True
            answered = feature_entries(having[e], idx, sims, modality)
        else:
            answered = deferred(having[e], idx, sims)
        entries.extend((similarity, e, order, segments) for order, (similarity, segments) in enumerate(answered))
    return merge_entries(entries, keep)


def find_relevant_video_segments(events, query_features, *, store: Optional[EventStore] = None, deferred: Optional[Callable] = None,
                                 k: int = 5, keep: int = 5, min_similarity: float = 0.4, prefilter: bool = False,
                                 exact64: bool = False) -> List[SequenceSegment]:
    """``_find_relevant_video_segments`` (:3127-3279) over ``events`` (the long-term store).  ``store``: an ``EventStore`` over the
    vision matrices of the events that have one, in order (built once when not given -- keep it between questions).
    ``deferred(event, idx, sims)``: the LLM block for an event below the threshold that has captions; it returns the event's
    ``[(similarity, [segments])]`` entries (``feature_entries`` is what its error branch returns, and what stands in when no
    callable is given).  A query whose size is not 1024 returns [] (:3135-3137).  ``exact64=True``: similarities, the threshold
    decision and the ranking in float64 (``EventStore.relevant_hits``); ValueError with ``prefilter`` or on a store that is not
    eligible."""
    return _find("vision", events, query_features, store, deferred, k, keep, min_similarity, prefilter, exact64)


def find_relevant_audio_segments(events, query_features, *, store: Optional[EventStore] = None, deferred: Optional[Callable] = None,
                                 k: int = 5, keep: int = 5, min_similarity: float = 0.4, prefilter: bool = False,
                                 exact64: bool = False) -> List[SequenceSegment]:
    """``_find_relevant_audio_segments`` (:3281-3383); see ``find_relevant_video_segments`` (the store holds the audio matrices,
    the row limit is ``len(event.feature_times['audio_times'])``, the flag is ``holistic_audio_transcription``)."""
    return _find("audio", events, query_features, store, deferred, k, keep, min_similarity, prefilter, exact64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the recall frame windows: shrink, JPEG and SSIM dedup of the frames read around every frame_time of the relevant segments
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_WINDOW_FRAMES = 8                      # the reference's +-1 s windows at 1 fps hold at most 3
RECALL_SIZE = (320, 180)                   # (width, height) of cv2.resize at hippocampal_memory.py:2232, :2795
RECALL_SIMILARITY_CUT = 0.3                # :2238, :2801


def walk_recall_window(scores, similarity_cut: float = RECALL_SIMILARITY_CUT) -> List[int]:
    """The dedup walk of one recall window (hippocampal_memory.py:2223-2249, :2786-2812) as a host function of the scores:
    ``scores[i][j]``, i < j, is the SSIM of frames i and j of the window with i in the im1 role; only those entries are read, and
    only the ones the walk consults.  -> the kept indices.  Frame 0 is kept; frame j is dropped iff
    ``scores[last kept][j] > similarity_cut`` -- a NaN score (a flat earlier frame) keeps the frame, as Python's comparison does
    -- and a dropped frame does not become the comparison base."""
    m = len(scores)
    kept = [0] if m else []
    for j in range(1, m):
        if not scores[kept[-1]][j] > similarity_cut:
            kept.append(j)
    return kept


@dataclass
class RecallWindowFrames:
    """What ``recall_window_frames`` returns.  Per window, in the order given: ``kept`` the indices of the frames that survive
    the dedup walk, ``times`` their times, ``files`` their JPEG files (bytes).  Flat, window after window -- the order in which the
    reference appends to all_segment_frames / all_segment_times: ``all_segment_times``, ``all_segment_files`` and, when ``paths``
    were given, ``all_segment_frames`` (the paths the kept files were written to; else None)."""
    kept: List[List[int]]
    times: List[List[float]]
    files: List[List[bytes]]
    all_segment_times: List[float]
    all_segment_files: List[bytes]
    all_segment_frames: Optional[List[str]] = None


def recall_window_frames(windows, size: Tuple[int, int] = RECALL_SIZE, similarity_cut: float = RECALL_SIMILARITY_CUT,
                         quality: int = SAVE_QUALITY, paths=None, cache: Optional[FrameCache] = None) -> RecallWindowFrames:
    """The numeric work of the frame loop that follows retrieval in ``_process_video_query`` / ``_process_multimodal_query``
    (:2226-2249, :2789-2812) for all windows of a question in one pass.  ``windows``: one list per (segment, frame_time) of
    ``(time, frame)`` in read order, the frames BGR uint8 (H, W, 3) arrays as ``cap.read()`` returns them; video decoding stays
    with the caller.  At most ``MAX_WINDOW_FRAMES`` frames per window (``ValueError``).

    Per call: one pinned upload and one resize launch per source geometry (``cv2.resize(frame, size)``, ``size`` = (width,
    height): ``resize.resize_frames``); one ``encode_jpeg(..., "BGR", return_decoded=True)`` at ``quality`` and 4:2:0 (the
    files of ``cv2.imwrite``'s defaults, and their decoded pixels without a file round-trip); one gray pass with min / max; one
    ``hmm_ssim_pairs`` over all (i < j) pairs inside each window, the earlier frame in the im1 role (data_range = max - min of
    it, as ``_compute_frame_similarity`` passes); one read-back of the scores; then ``walk_recall_window`` per window
    on the host: frame 0 is kept, a frame is dropped iff its SSIM with the last kept frame is ``> similarity_cut``.

    ``paths``: one path per frame, nested as ``windows``; the kept frames' files are written there (parents are created), dropped
    frames write nothing.  The reference's ``/tmp/frame_<ms>.jpg`` names collide across segments, so naming stays with the
    caller.  ``cache``: a ``FrameCache`` that receives the gray frame of every file written (needs ``paths``).

    The source may not be smaller than ``size`` on either axis, and ``size`` not under 7 x 7 (``ValueError``).  The file bytes are
    Pillow's for the shrunk frame (``encode_jpeg``); they are not claimed to equal OpenCV's file."""
    windows = [list(w) for w in windows]
    for w, window in enumerate(windows):
        if len(window) > MAX_WINDOW_FRAMES:
            raise ValueError(f"recall_window_frames: window {w} holds {len(window)} frames; at most {MAX_WINDOW_FRAMES} are taken")
        for _, frame in window:
            if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
                raise TypeError(f"recall_window_frames: window {w} holds a frame that is not a uint8 (H, W, 3) BGR array")
    if paths is not None:
        paths = [[str(p) for p in ps] for ps in paths]
        if [len(ps) for ps in paths] != [len(w) for w in windows]:
            raise ValueError("recall_window_frames: paths must hold one path per frame, nested as windows")
    elif cache is not None:
        raise ValueError("recall_window_frames: cache= keys frames by the path of their file; give paths= too")
    dw, dh = (int(v) for v in size)
    if dw < WIN or dh < WIN:
        raise ValueError(f"recall_window_frames: size {dw} x {dh} is under the {WIN} x {WIN} SSIM window")
    flat = [frame for window in windows for _, frame in window]
    base = np.cumsum([0] + [len(window) for window in windows])
    groups = {}
    for i, frame in enumerate(flat):
        resize_mode(frame.shape[:2], (dh, dw))                            # an enlargement raises before anything is uploaded
        groups.setdefault(frame.shape[:2], []).append(i)
    scores = np.empty(0)
    files: List[bytes] = []
    pairs = [(int(base[w]) + i, int(base[w]) + j) for w, window in enumerate(windows)
             for i in range(len(window)) for j in range(i + 1, len(window))]
    if flat:
        dev = _lib.require_gpu()
        small = None
        for members in groups.values():
            shrunk = resize_frames(upload_frames([flat[i] for i in members], dev), (dw, dh))
            if len(groups) == 1:
                small = shrunk
            else:
                if small is None:
                    small = torch.empty((len(flat), dh, dw, 3), dtype=torch.uint8, device=dev)
                small.index_copy_(0, torch.tensor(members, dtype=torch.int64).to(dev), shrunk)
        files, decoded = jpeg.encode_jpeg(small, quality=quality, subsampling=SAVE_SUBSAMPLING, channel_order="BGR",
                                          return_decoded=True)
        if pairs:
            gray, minmax = gray_frames(decoded, "RGB", return_minmax=True)
            scores = ssim_launch(gray, np.array(pairs, dtype=np.int32), -1.0, minmax).cpu().numpy()
    out = RecallWindowFrames([], [], [], [], [], None if paths is None else [])
    at = 0
    for w, window in enumerate(windows):
        m = len(window)
        table = np.full((m, m), np.nan)
        for i in range(m):
            for j in range(i + 1, m):
                table[i, j] = scores[at]
                at += 1
        kept = walk_recall_window(table, similarity_cut)
        out.kept.append(kept)
        out.times.append([window[i][0] for i in kept])
        out.files.append([files[int(base[w]) + i] for i in kept])
        out.all_segment_times.extend(out.times[-1])
        out.all_segment_files.extend(out.files[-1])
        if paths is not None:
            out.all_segment_frames.extend(paths[w][i] for i in kept)
    if paths is not None:
        written = []
        for w, kept in enumerate(out.kept):
            for i, data in zip(kept, out.files[w]):
                Path(paths[w][i]).parent.mkdir(parents=True, exist_ok=True)
                Path(paths[w][i]).write_bytes(data)
                written.append((paths[w][i], int(base[w]) + i))
        if cache is not None and written:
            last = {p: k for p, k in written}                             # a path written twice holds its last frame
            cache.put(list(last), decoded[torch.tensor(list(last.values()), dtype=torch.int64).to(decoded.device)])
    return out
