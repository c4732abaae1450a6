"""Input recipes of tests/golden/retrieval_segments_golden.json: hand-built long-term stores for the reference's
_find_relevant_video_segments / _find_relevant_audio_segments (hippocampal_memory.py:3127-3383), rebuilt from seeds by the
generator (make_retrieval_golden.py) and by the tests.

Every row of an event is  t * u + sqrt(1 - t^2) * v  scaled by a positive factor, with u the unit query and v a unit vector
orthogonal to it, so its cosine similarity with the query is the chosen t up to fp32 rounding.  The t of one case are drawn
without replacement from the grid 0.0007 + 0.002 i: any two differ by at least 2e-3, and none is within 7e-4 of the 0.4
threshold or of the LLM entries' 0.6.

An event spec: (rows, kept, lo, hi, flagged, answer)
  rows, kept    rows of the feature matrix, and how many of them are kept rows (len(frame_times) / len(audio_times));
  lo, hi        the similarities of its rows lie in [lo, hi);
  flagged       the event has captions (vision) / a transcription (audio);
  answer        what the fake LLM answers for this event (None where it is never asked).
"""
from types import SimpleNamespace

import numpy as np

DIM = 1024

# An event named "other" has no matrix of the case's modality and is skipped (:3144, :3295).
CASES = {
    # events of 1, 4, 9 and 30 rows; every row kept: the row rule drops nothing
    "sizes_all_kept": {"seed": 11, "events": [(1, 1, 0.45, 0.9, False, None), (4, 4, 0.45, 0.9, False, None),
                                             (9, 9, 0.45, 0.9, False, None), (30, 30, 0.45, 0.9, False, None)]},
    # kept lists from 1 to n rows: the rule drops all, most, some and none of an event's five hits
    "kept_1_to_n": {"seed": 12, "events": [(30, 1, 0.45, 0.9, False, None), (30, 5, 0.45, 0.9, False, None), "other",
                                          (30, 15, 0.45, 0.9, False, None), (30, 29, 0.45, 0.9, False, None),
                                          (30, 30, 0.45, 0.9, False, None), (9, 1, 0.45, 0.9, False, None),
                                          (9, 8, 0.45, 0.9, False, None), (4, 2, 0.45, 0.9, False, None), (1, 1, 0.45, 0.9, False, None)]},
    # flagged, but its best similarity is above 0.4: not deferred; and one below 0.4 without the flag: not deferred either
    "not_deferred": {"seed": 13, "events": [(9, 9, 0.05, 0.55, True, None), (9, 9, 0.05, 0.38, False, None),
                                           (4, 3, 0.05, 0.38, "absent", None)]},
    # deferred, the LLM's answer parses: one entry at 0.6 between the feature hits
    "deferred_parsable": {"seed": 14, "events": [(9, 9, 0.45, 0.9, False, None), (30, 12, 0.05, 0.38, True, "parsable"),
                                                (4, 4, 0.3, 0.58, False, None)]},
    # deferred, the answer does not parse: the error branch answers from the event's own hits, under the row rule
    "deferred_error": {"seed": 15, "events": [(9, 4, 0.05, 0.38, True, "unparsable"), (4, 4, 0.05, 0.3, False, None),
                                             (30, 30, 0.05, 0.25, True, "unparsable")]},
    # fewer than five entries survive the row rule
    "fewer_than_five": {"seed": 16, "events": [(30, 2, 0.45, 0.9, False, None), (9, 1, 0.45, 0.9, False, None),
                                              (4, 1, 0.45, 0.9, False, None)]},
}
ANSWERS = {("vision", "parsable"): "2", ("vision", "unparsable"): "frames: 1 and 2",
           ("audio", "parsable"): '{"start": 3.25, "end": 5.5}', ("audio", "unparsable"): "[1, 2]"}
MODALITIES = ("vision", "audio")


def _unit(v):
    return v / np.linalg.norm(v)


def build(name, modality):
    """-> (events, query float32[1024], answers {event tag: the fake LLM's reply}).  events: SimpleNamespace objects with the
    attributes the reference reads; ``name`` is the tag the fake client finds in the prompt."""
    spec = CASES[name]
    rng = np.random.default_rng(spec["seed"] * 2 + MODALITIES.index(modality))
    query = rng.standard_normal(DIM)
    u = _unit(query)
    n_rows = sum(e[0] for e in spec["events"] if e != "other")
    grid = 0.0007 + 0.002 * np.arange(500)
    events, answers, taken = [], {}, set()
    for pos, e in enumerate(spec["events"]):
        tag = f"EVENT-{pos}-TAG"
        if e == "other":
            other = "audio" if modality == "vision" else "vision"
            events.append(SimpleNamespace(name=tag, features={other: np.zeros((2, DIM), np.float32)}, frame_times=[0.0], frames=["x.jpg"],
                                          feature_times={"audio_times": [0.0]}))
            continue
        rows, kept, lo, hi, flagged, answer = e
        free = [i for i in np.flatnonzero((grid >= lo) & (grid < hi)) if i not in taken]
        pick = rng.choice(free, size=rows, replace=False)
        taken.update(int(i) for i in pick)
        mat = np.empty((rows, DIM))
        for r, t in enumerate(grid[pick]):
            v = rng.standard_normal(DIM)
            v = _unit(v - (v @ u) * u)
            mat[r] = (t * u + np.sqrt(1.0 - t * t) * v) * rng.uniform(0.5, 3.0)
        times = [round(0.4 + 0.7 * j + 0.05 * pos, 3) for j in range(kept)]
        event = SimpleNamespace(name=tag, features={modality: mat.astype(np.float32)})
        if modality == "vision":
            event.frame_times, event.frames = times, [f"{tag}/frame_{j:03d}.jpg" for j in range(kept)]
            if flagged != "absent":
                event.frame_captions = [f"{tag} caption {j}" for j in range(kept)] if flagged else []
        else:
            event.feature_times = {"audio_times": times}
            if flagged != "absent":
                event.holistic_audio_transcription = [{"start": 0.0, "end": 4.0, "text": f"{tag} somebody speaks"}] if flagged else []
        if answer is not None:
            answers[tag] = ANSWERS[modality, answer]
        events.append(event)
    assert n_rows == sum(len(ev.features[modality]) for ev in events if modality in ev.features)
    return events, query.astype(np.float32), answers
