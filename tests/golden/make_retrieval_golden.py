#!/usr/bin/env python3
"""Generate tests/golden/retrieval_segments_golden.json by running the UNMODIFIED reference methods
QARecallSystem._find_relevant_video_segments / _find_relevant_audio_segments (hippomm/core/hippocampal_memory.py:3127-3383).

Run where the reference tree is available (make_golden.py names the place):

    python tests/golden/make_retrieval_golden.py

The methods are imported behind the stub modules of ``make_golden.import_reference()`` and called on an instance made with
``QARecallSystem.__new__`` that carries only what they read: a ``SimpleNamespace`` memory whose ``long_term_store`` is the hand-built
events of retrieval_recipes.py, a token counter, and a fake ``thinking_client`` that answers each prompt with the reply the recipe
gives for the event whose tag the prompt contains.

Written: the recipe names (the inputs are rebuilt from seeds), the returned segments' fields, and -- for every event the
reference handed to the LLM block -- the ``(similarity, segment)`` entries that block produced.  Those are read off the method's own
``similarity_segments`` list when the method returns (a profile hook; the method runs unmodified), with the store reduced to
that one event, so the entries are the event's alone.  The tests' callable replays them: nothing of the LLM block is restated.

Two margins are ASSERTED here, both >= 1e-4 (50 x the scan's stated 2e-6), so that no decision can flip on a summation order:
  * every flagged event's best similarity is at least 1e-4 away from 0.4;
  * adjacent similarities among the best keep + 1 entries differ by at least 1e-4.
"""
from __future__ import annotations

import json
import platform
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden  # noqa: E402
import retrieval_recipes as R  # noqa: E402

KEEP, MARGIN = 5, 1e-4
METHODS = {"vision": "_find_relevant_video_segments", "audio": "_find_relevant_audio_segments"}
FLAG = {"vision": "frame_captions", "audio": "holistic_audio_transcription"}


class FakeClient:
    """thinking_client.chat.completions.create(...): the recipe's reply for the event whose tag is in the prompt."""

    def __init__(self, answers):
        self.answers, self.asked = answers, []
        self.chat = SimpleNamespace(completions=SimpleNamespace(create=self.create))

    def create(self, model, messages, **_):
        prompt = messages[0]["content"]
        tags = [tag for tag in self.answers if tag in prompt]
        assert len(tags) == 1, tags
        self.asked.append(tags[0])
        return SimpleNamespace(choices=[SimpleNamespace(message=SimpleNamespace(content=self.answers[tags[0]]))])


def segment_fields(seg):
    return {"start_time": seg.start_time, "end_time": seg.end_time, "frames": seg.frames, "frame_times": seg.frame_times,
            "audio_data": seg.audio_data}


def run_reference(QARecallSystem, modality, events, query, answers):
    """-> (returned segments, the method's similarity_segments list at its return, the events the LLM was asked about)."""
    qa = QARecallSystem.__new__(QARecallSystem)
    qa.memory = SimpleNamespace(long_term_store=events)
    qa.tc = SimpleNamespace(num_tokens_from_string=lambda s: len(s.split()))
    qa.context_length, qa.reasoning_model, qa._current_question = 100000, "fake", "what happens?"
    qa.thinking_client = FakeClient(answers)
    seen = {}

    def hook(frame, event, arg):
        if event == "return" and frame.f_code.co_name == METHODS[modality]:
            seen["entries"] = list(frame.f_locals["similarity_segments"])

    sys.setprofile(hook)
    try:
        args = (torch.from_numpy(query), "an element") if modality == "vision" else (torch.from_numpy(query),)
        segments = getattr(qa, METHODS[modality])(*args)
    finally:
        sys.setprofile(None)
    return segments, seen["entries"], qa.thinking_client.asked


def main():
    topk_ref, _ = make_golden.import_reference()
    from hippomm.core.hippocampal_memory import QARecallSystem
    out = {"_generated_by": "tests/golden/make_retrieval_golden.py",
           "_env": {"numpy": np.__version__, "python": platform.python_version(), "machine": platform.processor() or platform.machine()},
           "_reference": "hippomm/core/hippocampal_memory.py:3127-3279, :3281-3383", "keep": KEEP, "cases": {}}
    for modality in R.MODALITIES:
        for name in R.CASES:
            events, query, answers = R.build(name, modality)
            segments, entries, asked = run_reference(QARecallSystem, modality, events, query, answers)
            # margin 1: flagged events against the threshold
            threshold_margin = np.inf
            for event in events:
                if modality in event.features and getattr(event, FLAG[modality], None):
                    best = float(np.max(topk_ref(query, event.features[modality], 5)[1]))
                    threshold_margin = min(threshold_margin, abs(best - 0.4))
            assert threshold_margin >= MARGIN, (modality, name, threshold_margin)
            # margin 2: adjacent entries among the best keep + 1 (the list is sorted when the method returns)
            top = [float(sim) for sim, _ in entries[:KEEP + 1]]
            gaps = [a - b for a, b in zip(top, top[1:])]
            assert all(g >= MARGIN for g in gaps), (modality, name, top)
            # the LLM block's entries, event by event: the store reduced to that event
            deferred = {}
            for tag in asked:
                alone = [event for event in events if event.name == tag]
                _, own, asked_again = run_reference(QARecallSystem, modality, alone, query, answers)
                assert asked_again == [tag]
                deferred[tag] = [[float(sim), segment_fields(segs[0])] for sim, segs in own]
                assert all(len(segs) == 1 for _, segs in own)
            out["cases"][f"{modality}/{name}"] = {
                "modality": modality, "recipe": name, "n_entries": len(entries), "asked": asked,
                "threshold_margin": None if not np.isfinite(threshold_margin) else threshold_margin,
                "min_gap_top": min(gaps) if gaps else None,
                "segments": [segment_fields(s) for s in segments], "deferred_entries": deferred}
            print(f"{modality}/{name}: {len(entries)} entries, {len(segments)} segments, asked {asked}")
    (HERE / "retrieval_segments_golden.json").write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
