#!/usr/bin/env python3
"""Generate tests/golden/consolidation_caller_golden.json by running the UNMODIFIED reference's consolidation caller.

Run in the build container only (it needs the reference checkout, which does not exist on the GPU box):

    python tests/golden/make_consolidation_caller_golden.py [--reference DIR] [--check]

HippocampalMemory._process_vision_features (hippomm/core/hippocampal_memory.py:815-867), _process_audio_features (:869-927) and
consolidate_short_term_memory (:754-813) are imported behind the stub modules of make_golden.py and called unchanged on a
``HippocampalMemory.__new__`` object, with the reference's own ShortTermMemory / SequenceSegment objects built from the recipe of
tests/consolidation_cases.py.  The object's ``_select_key_frames`` is the reference's own, wrapped only to note what it returned.
Written: the recipe, the kept frames, the times, shapes / dtypes / SHA-256 of the stacked matrices, the order of their rows (found by
looking every stacked row's bytes up among the recipe's rows), the scalar fields of the consolidated memory, the number of rows the
reference's warning reports as skipped, and the smallest |S - 0.9| over the comparisons the selection made.  No feature value and
no reference source.  A case whose margin is under 1e-3 is refused.  --check compares with the committed file instead of writing.
"""
from __future__ import annotations

import argparse
import json
import logging
import platform
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import consolidation_cases as K  # noqa: E402

THRESHOLD = 0.9


class _Warnings(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


def _margin(features: np.ndarray, kept) -> float:
    """The smallest |S - 0.9| over the comparisons of :958-965, with S as :951-952 computes it and the kept list as it stood at
    each step (rebuilt from the reference's answer).  None: no comparison was made (:947-948)."""
    if len(features) <= 2:
        return None
    fn = features / np.linalg.norm(features, axis=1, keepdims=True)
    S = np.dot(fn, fn.T)
    kept, so_far, low = set(int(i) for i in kept), [0], np.inf
    for i in range(1, len(features)):
        low = min(low, float(np.abs(S[i, so_far].astype(np.float64) - THRESHOLD).min()))
        if i in kept:
            so_far.append(i)
    return min(low, float(np.abs(S[-1, so_far].astype(np.float64) - THRESHOLD).min()))


def _matrix_entry(ci, which, features) -> dict:
    table = K.rows_by_bytes(ci, which)
    return {"order": [table[row.tobytes()] for row in features], "shape": list(features.shape), "dtype": str(features.dtype),
            "sha256": K.digest(features)}


def generate(hm) -> dict:
    watch = _Warnings()
    hm.logger.addHandler(watch)
    cases = []
    try:
        for ci, case in enumerate(K.RECIPE["cases"]):
            make = lambda: K.case_memories(ci, memory=hm.ShortTermMemory, segment=hm.SequenceSegment)   # noqa: E731
            self = hm.HippocampalMemory.__new__(hm.HippocampalMemory)
            selections = []

            def noting(features, times, *a, **k):
                kept = hm.HippocampalMemory._select_key_frames(self, features, times, *a, **k)
                selections.append((features, kept))
                return kept
            self._select_key_frames = noting

            def skipped(call, memories, what):
                before = len(watch.messages)
                result = call(self, memories, None)
                return result, sum(what in m for m in watch.messages[before:])

            def vision_entry(features, content, n_skipped):
                if "vision" not in features:
                    return {"empty": True, "skipped": n_skipped}
                f, kept = selections[-1]
                assert f is features["vision"]
                margin = _margin(f, kept)
                if margin is not None and margin < K.MIN_MARGIN:
                    raise SystemExit(f"case {case['name']}: a compared similarity lies {margin:.2e} from the threshold")
                return dict(_matrix_entry(ci, 0, f), times=features["vision_times"].tolist(), times_dtype=str(features["vision_times"].dtype),
                            skipped=n_skipped, kept=[int(i) for i in kept], frames=content["frames"], frame_times=content["frame_times"],
                            margin=margin)

            def audio_entry(features, content, n_skipped):
                if "audio" not in features:
                    return {"empty": True, "skipped": n_skipped}
                return dict(_matrix_entry(ci, 1, features["audio"]), times=features["audio_times"].tolist(),
                            times_dtype=str(features["audio_times"].dtype), skipped=n_skipped, audio_times=content["audio_times"],
                            transcription=content["transcription"])

            # the two helpers on the list as the caller holds it ...
            entry = {"name": case["name"]}
            v, v_skipped = skipped(hm.HippocampalMemory._process_vision_features, make(), "Skipping frame feature")
            assert v["features"] or v == {"features": {}, "content": {}}
            entry["vision"] = vision_entry(v["features"], v["content"], v_skipped)
            a, a_skipped = skipped(hm.HippocampalMemory._process_audio_features, make(), "Skipping audio feature")
            assert a["features"] or a == {"features": {}, "content": {}}
            entry["audio"] = audio_entry(a["features"], a["content"], a_skipped)
            # ... and the whole call, which sorts the list by start_time first: tied frame times can fall differently
            memories = make()
            ids = {id(m): spec["id"] for m, spec in zip(memories, case["memories"])}
            before = len(watch.messages)
            c = hm.HippocampalMemory.consolidate_short_term_memory(self, memories)
            said = watch.messages[before:]
            entry["consolidated"] = {"timestamp": c.timestamp, "source_time": c.source_time,
                                     "segment_info": {"start_time": c.segment_info.start_time, "end_time": c.segment_info.end_time},
                                     "modalities": sorted(c.modalities), "transcription": c.transcription,
                                     "feature_keys": list(c.features), "content_keys": list(c.content),
                                     "memory_order": [ids[id(m)] for m in memories],
                                     "vision": vision_entry(c.features, c.content, sum("Skipping frame feature" in m for m in said)),
                                     "audio": audio_entry(c.features, c.content, sum("Skipping audio feature" in m for m in said))}
            cases.append(entry)
    finally:
        hm.logger.removeHandler(watch)
    return {"_generated_by": "tests/golden/make_consolidation_caller_golden.py",
            "_env": {"numpy": np.__version__, "python": platform.python_version()},
            "_reference": {"consolidate": "hippomm/core/hippocampal_memory.py:754-813", "vision": "hippomm/core/hippocampal_memory.py:815-867",
                           "audio": "hippomm/core/hippocampal_memory.py:869-927", "select": "hippomm/core/hippocampal_memory.py:944-967"},
            "threshold": THRESHOLD, "min_margin": K.MIN_MARGIN, "recipe": K.RECIPE, "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="the reference checkout (default: where make_golden.py looks)")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture; write nothing")
    a = ap.parse_args()
    import make_golden
    if a.reference:
        make_golden.REF = a.reference
    make_golden.import_reference()
    import hippomm.core.hippocampal_memory as hm
    out = json.loads(json.dumps(generate(hm)))                       # as the file will read back
    margins = [v["margin"] for c in out["cases"] for v in (c["vision"], c["consolidated"]["vision"]) if v.get("margin") is not None]
    if a.check:
        have = K.golden()
        differ = [k for k in out if not k.startswith("_env") and out[k] != have.get(k)]
        if differ:
            raise SystemExit(f"{K.GOLDEN} differs from what the reference gives now in: {differ}")
        print(f"{K.GOLDEN}: reproduced ({len(out['cases'])} cases, smallest margin {min(margins):.4f})")
        return
    K.GOLDEN.write_text(json.dumps(out, indent=1) + "\n")
    print(f"{K.GOLDEN}: {K.GOLDEN.stat().st_size} bytes, {len(out['cases'])} cases, smallest margin {min(margins):.4f}")


if __name__ == "__main__":
    main()
