"""A numpy / plain-Python model of the reference's retrieval step after the per-event scan (hippocampal_memory.py:3143-3277,
:3294-3381): the fallback rule, the row rule, the global stable ranking and the host merge.  It is written from the reference's
statements, independently of hippomm_amd: the tests compare the kernels, the store methods and hippomm_amd.retrieval with it, and
test_cpu_relevant_hits_model.py pins the model itself to the reference's recorded answers.

Order: similarity descending, NaN first (the library's rule, include/hippomm_hip.h), equal similarities by position -- event, then
slot inside the event -- which is what Python's stable ``sort(reverse=True)`` leaves of a list built event by event."""
import numpy as np


def _rank_key(sim):
    """Ascending sort key of 'similarity descending, NaN first'; -0.0 and 0.0 are equal, as the device's order bits make them."""
    return (0, 0.0) if sim != sim else (1, -float(sim))


def is_deferred(defer, e, count, best, min_similarity):
    """Rule 2 for one event: flagged, has a hit, and its best similarity (slot 0) is below the threshold as fp32.  A NaN best
    similarity compares False, as ``max(similarities) < 0.4`` does."""
    return bool(defer is not None and defer[e] and count > 0 and np.float32(best) < np.float32(min_similarity))


def rank_filtered(idx, sims, counts, keep, row_limits=None, defer=None, min_similarity=0.4):
    """The C contract of hmm_rank_segment_hits_filtered on (E, k) arrays -> dict of
    event / row / sim (padded to keep with -1 / -1 / 0), n, deferred_event (padded to E with -1), n_deferred, and the compacted
    deferred_idx / deferred_sim (n_deferred, k) / deferred_count (n_deferred,)."""
    idx, sims, counts = np.asarray(idx), np.asarray(sims, np.float32), np.asarray(counts)
    E, k = idx.shape
    deferred = [e for e in range(E) if is_deferred(defer, e, counts[e], sims[e, 0], min_similarity)]
    gone = set(deferred)
    cand = [(e, s) for e in range(E) if e not in gone for s in range(min(int(counts[e]), k))
            if row_limits is None or int(idx[e, s]) < int(row_limits[e])]
    cand.sort(key=lambda es: _rank_key(sims[es]))                       # stable: ties stay in (event, slot) order
    best = cand[:keep]
    out = {"event": np.full(keep, -1, np.int64), "row": np.full(keep, -1, np.int64), "sim": np.zeros(keep, np.float32),
           "n": len(best), "deferred_event": np.full(E, -1, np.int32), "n_deferred": len(deferred)}
    for t, (e, s) in enumerate(best):
        out["event"][t], out["row"][t], out["sim"][t] = e, idx[e, s], sims[e, s]
    out["deferred_event"][:len(deferred)] = deferred
    out["deferred_idx"] = idx[deferred].reshape(len(deferred), k).astype(np.int64)
    out["deferred_sim"] = sims[deferred].reshape(len(deferred), k)
    out["deferred_count"] = counts[deferred].astype(np.int32)
    return out


def relevant_hits(per_event, keep=5, row_limits=None, defer=None, min_similarity=0.4):
    """EventStore.relevant_hits from the per-event hits [(idx, sims)] (what top_k_per_event returns) -> (hits, deferred)."""
    E = len(per_event)
    deferred = [e for e in range(E)
                if is_deferred(defer, e, len(per_event[e][0]), per_event[e][1][0] if len(per_event[e][1]) else 0.0, min_similarity)]
    gone = set(deferred)
    cand = [(e, int(row), sim) for e in range(E) if e not in gone for row, sim in zip(*per_event[e])
            if row_limits is None or row < row_limits[e]]
    cand.sort(key=lambda hit: _rank_key(hit[2]))
    return ([(e, row, float(sim)) for e, row, sim in cand[:keep]],
            [(e, np.asarray(per_event[e][0], np.int64), np.asarray(per_event[e][1], np.float32)) for e in deferred])


def kept_times(event, modality):
    return event.frame_times if modality == "vision" else event.feature_times["audio_times"]


def segment_fields(event, row, modality):
    """The fields of the +-1 s segment around kept row ``row`` (:3263-3271, :3371-3375) as a dict."""
    if modality == "vision":
        t = event.frame_times[row]
        return {"start_time": max(0, t - 1), "end_time": t + 1,
                "frames": [f for f, u in zip(event.frames, event.frame_times) if t - 1 <= u <= t + 1],
                "frame_times": [u for u in event.frame_times if t - 1 <= u <= t + 1], "audio_data": None}
    times = event.feature_times["audio_times"]
    return {"start_time": max(0, times[row] - 1), "end_time": times[row] + 1, "frames": None, "frame_times": None, "audio_data": None}


def find_segments(events, per_event, modality, answers, keep=5, min_similarity=0.4):
    """The whole step -> the returned segments' fields.  events: those that HAVE the modality, per_event their scan hits,
    answers[e]: the [(similarity, segment fields)] entries of deferred event e (the LLM block's, recorded from the reference)."""
    flag = "frame_captions" if modality == "vision" else "holistic_audio_transcription"
    entries = []                                                          # (similarity, fields) in the reference's list order
    for e, (event, (idx, sims)) in enumerate(zip(events, per_event)):
        if is_deferred([bool(getattr(event, flag, None))], 0, len(idx), sims[0] if len(sims) else 0.0, min_similarity):
            entries.extend((sim, fields) for sim, fields in answers[e])
        else:
            limit = len(kept_times(event, modality))
            entries.extend((sim, segment_fields(event, int(row), modality)) for row, sim in zip(idx, sims) if row < limit)
    entries.sort(key=lambda entry: _rank_key(entry[0]))
    return [fields for _, fields in entries[:keep]]
