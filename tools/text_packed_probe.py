"""Text tower, padded rows against packed rows, on one MI355X: what a batch of questions costs by each route, in one process.

    python tools/text_packed_probe.py        # -> profiles/text_packed.json

Workload: the full-depth text tower (24 blocks, seeded random-init weights), Q in {1, 9, 16, 64, 256} questions whose lengths
(SOT + tokens + EOS) are drawn uniformly from 4 .. 12.  That is the ASSUMED shape of the reference's "2-5-word" queries
(hippocampal_memory.py:2173-2176, :2445-2448) under the CLIP BPE; it is not measured on real questions.
The sides, alternating in one session:
  (padded) ImageBind.forward({"text": ids}) as it stands: 77 rows per question;
  (packed) the same call with pack_text = True: sum of the lengths rows, the last block on the EOS rows only.
The ids start on the host, as a tokenizer returns them; each call is timed on the wall clock around the forward AND the .cpu()
of its embeddings (upload of the ids, table upload, tower, read-back).  Steady state: ROUNDS alternating groups; in each group
and for each side WARM_MS of the same calls, then ITERS timed calls; the median group of each side.  The padded route of the
same build is the baseline (the packed route does not touch it).  Not part of bench.py; no threshold and no default depends on it.
"""
from __future__ import annotations

import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
QS = (1, 9, 16, 64, 256)
LEN_LO, LEN_HI = 4, 12
WARM_MS, ROUNDS, ITERS = 60.0, 5, 20
SOT, EOS = 49406, 49407


def questions(q, seed):
    """(q,77) int64 host ids with lengths uniform in LEN_LO .. LEN_HI, and the lengths."""
    import torch
    rng = np.random.default_rng(seed)
    lengths = rng.integers(LEN_LO, LEN_HI + 1, size=q)
    ids = np.zeros((q, 77), dtype=np.int64)
    for b, n in enumerate(lengths):
        ids[b, 0] = SOT
        ids[b, 1:n - 1] = rng.integers(1, 49000, size=n - 2)
        ids[b, n - 1] = EOS
    return torch.from_numpy(ids), lengths


def _warm(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < WARM_MS:
        fn()


def _alternate(sides):
    import torch
    got = {name: [] for name in sides}
    for _ in range(ROUNDS):
        for name, fn in sides.items():
            _warm(fn)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ITERS):
                fn()                                             # ends in .cpu(): the call is complete when it returns
            got[name].append((time.perf_counter() - t0) * 1e3 / ITERS)
    return got


def main():
    import torch
    from hippomm_amd.encoder import ImageBind, synthetic_state_dict
    torch.cuda.set_device(0)
    model = ImageBind(state_dict=synthetic_state_dict(("text",), seed=5), towers=("text",))
    result = {"workload": f"text tower, full depth; lengths uniform {LEN_LO}..{LEN_HI} (assumed shape of 2-5-word queries, not measured)",
              "timing": f"wall clock around forward + .cpu(); {ROUNDS} alternating groups of {ITERS} calls after {WARM_MS:g} ms warm-up; "
                        "median group, ms per call", "by_questions": {}}
    for q in QS:
        ids, lengths = questions(q, seed=100 + q)

        def run(pack):
            model.pack_text = pack
            return model.forward({"text": ids})["text"].cpu()

        padded, packed = run(False), run(True)
        stats = dict(model.text_stats)
        cos = torch.nn.functional.cosine_similarity(padded, packed, dim=1)
        groups = _alternate({"padded": lambda: run(False), "packed": lambda: run(True)})
        ms = {k: statistics.median(v) for k, v in groups.items()}
        entry = {"rows_padded": stats["rows_padded"], "rows_packed": stats["rows_packed"],
                 "padded_ms": round(ms["padded"], 4), "packed_ms": round(ms["packed"], 4),
                 "packed_over_padded": round(ms["packed"] / ms["padded"], 4),
                 "groups_ms": {k: [round(x, 4) for x in v] for k, v in groups.items()},
                 "min_cos_packed_vs_padded": float(cos.min())}
        result["by_questions"][str(q)] = entry
        print(json.dumps({"questions": q, **{k: entry[k] for k in ("rows_padded", "rows_packed", "padded_ms", "packed_ms",
                                                                     "packed_over_padded", "min_cos_packed_vs_padded")}}), flush=True)
    model.pack_text = False
    out = ROOT / "profiles" / "text_packed.json"
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
