#!/usr/bin/env python3
"""Record what the UNMODIFIED reference returns on the float64 route's near-tie and threshold inputs.

Run next to a checkout of the reference (make_golden.REF); it imports hippomm/utils/vector_ops.py:151-188 as it is and calls it
the way _find_relevant_video_segments does: the store as the float64 matrix load_theta_event builds (here: the float64 copy of
the fp32 rows of tests/exact64_cases.py), the query as the fp32 vector `.cpu().numpy().flatten()` leaves.

    python tests/golden/make_exact64_golden.py            writes tests/golden/exact64_golden.json
    python tests/golden/make_exact64_golden.py --stdout   prints the same JSON (tests/test_cpu_exact64.py compares it live)

The file holds data only: per ladder seed the reference's index list and similarities (k = 20: the twelve rungs and the eight
rows behind them), per threshold seed the same for each of the three events (k = 5)."""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

LADDER_K, EVENT_K = 20, 5


def record():
    from make_golden import import_reference
    topk_ref = import_reference()[0]
    import exact64_cases as cases

    def call(store, query, k):
        idx, sims = topk_ref(query, np.asarray(store, dtype=np.float64), k)
        assert sims.dtype == np.float64
        return {"idx": [int(i) for i in idx], "sims": [float(s) for s in sims]}

    out = {"ladder_k": LADDER_K, "event_k": EVENT_K, "ladder": {}, "threshold": {}}
    for seed in cases.LADDER_SEEDS:
        store, query = cases.ladder_case(seed)[:2]
        out["ladder"][str(seed)] = call(store, query, LADDER_K)
    for seed in cases.THRESHOLD_SEEDS:
        events, query = cases.threshold_case(seed)[:2]
        out["threshold"][str(seed)] = [call(ev, query, EVENT_K) for ev in events]
    return out


if __name__ == "__main__":
    text = json.dumps(record(), indent=1)
    if "--stdout" in sys.argv[1:]:
        print(text)
    else:
        (HERE / "exact64_golden.json").write_text(text + "\n")
