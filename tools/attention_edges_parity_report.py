"""Writes profiles/attention_edges_parity.json: for every value and route case of tests/test_gpu_attention_edges.py the kernel's
worst error as a fraction of the tolerance the test applies (2^-8 |want| + 2^-8 softmax @ |v| + 1e-4 per element, against the
float64 reference of tests/attention_cases.py), and whether every one-hot case returned exactly its V rows.  A record of one
run; no threshold is taken from it.  Run on an MI355X after the library is built:
python tools/attention_edges_parity_report.py [--out PATH]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch                                       # noqa: E402

import attention_cases as A                        # noqa: E402
import test_gpu_attention_edges as T               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attention_edges_parity.json"))
    args = ap.parse_args()
    rows = []
    for group in ("value", "route"):
        for s in A.specs(group):
            c = A.case(s)
            r = A.ratio(c, T.run(c))
            rows.append({"group": group, "case": c.label, "worst_error_over_tolerance": r, "within_tolerance": r <= 1.0})
    exact = [{"case": s.label, "exact": bool(torch.equal(T.run(A.case(s)), A.case(s).picked))} for s in A.specs("onehot")]
    worst = {g: max(r["worst_error_over_tolerance"] for r in rows if r["group"] == g) for g in ("value", "route")}
    worst_case = max(rows, key=lambda r: r["worst_error_over_tolerance"])["case"]
    Path(args.out).write_text(json.dumps({"tolerance": "2^-8 |want| + 2^-8 softmax @ |v| + 1e-4", "worst_ratio": worst, "worst_case": worst_case,
                                          "one_hot_cases": len(exact), "one_hot_exact": sum(e["exact"] for e in exact),
                                          "cases": rows, "one_hot": exact}, indent=1) + "\n")
    print(f"{len(rows)} value and route cases, worst error / tolerance: {worst} ({worst_case}); "
          f"{sum(e['exact'] for e in exact)} / {len(exact)} one-hot cases exact -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
