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

Limits: where NaN similarities sort is this library's rule (first), not Python's; a store converted from fp64 holds fp32
similarities widened, so a 0.4 decision within 2e-6 of the threshold can differ from the reference.
"""
from __future__ import annotations

import logging
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .segmentation import SequenceSegment
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
          keep: int, min_similarity: float, prefilter: bool) -> List[SequenceSegment]:
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
                                            prefilter=prefilter)
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
                                 k: int = 5, keep: int = 5, min_similarity: float = 0.4, prefilter: bool = False
                                 ) -> List[SequenceSegment]:
    """``_find_relevant_video_segments`` (:3127-3279) over ``events`` (the long-term store).  ``store``: an ``EventStore`` over the
    vision matrices of the events that have one, in order (built once when not given -- keep it between questions).
    ``deferred(event, idx, sims)``: the LLM block for an event below the threshold that has captions; it returns the event's
    ``[(similarity, [segments])]`` entries (``feature_entries`` is what its error branch returns, and what stands in when no
    callable is given).  A query whose size is not 1024 returns [] (:3135-3137)."""
    return _find("vision", events, query_features, store, deferred, k, keep, min_similarity, prefilter)


def find_relevant_audio_segments(events, query_features, *, store: Optional[EventStore] = None, deferred: Optional[Callable] = None,
                                 k: int = 5, keep: int = 5, min_similarity: float = 0.4, prefilter: bool = False
                                 ) -> List[SequenceSegment]:
    """``_find_relevant_audio_segments`` (:3281-3383); see ``find_relevant_video_segments`` (the store holds the audio matrices,
    the row limit is ``len(event.feature_times['audio_times'])``, the flag is ``holistic_audio_transcription``)."""
    return _find("audio", events, query_features, store, deferred, k, keep, min_similarity, prefilter)
