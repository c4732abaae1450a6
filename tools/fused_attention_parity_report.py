"""Writes profiles/fused_attention_parity.json: for every value and deal case of tests/test_gpu_fused_attention_edges.py the fused
in_proj + attention kernel's worst error as a fraction of the tolerance the test applies (2^-8 |want| + 2^-8 softmax @ |v| + 1e-4
per element, against the float64 reference of tests/fused_attention_cases.py on exactly known q / k / v images), next to the
figure of that reference itself rounded to bf16, and whether every one-hot case returned exactly its V rows.  A record of one
run; no threshold is taken from it.  Run on an MI355X after the library is built:
python tools/fused_attention_parity_report.py [--out PATH]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch                                       # noqa: E402

import attention_cases as A                        # noqa: E402
import fused_attention_cases as F                  # noqa: E402
import test_gpu_fused_attention_edges as T         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fused_attention_parity.json"))
    args = ap.parse_args()
    cus = T._cus()
    rows = []
    for group in ("value", "deal"):
        for s in F.specs(group, cus):
            c = F.case(s)
            r, ref = A.ratio(c, T.run(c)), A.ratio(c, A.to_bf16(c.want))
            rows.append({"group": group, "case": c.label, "worst_error_over_tolerance": r, "rounded_reference_over_tolerance": ref,
                         "within_tolerance": r <= 1.0})
    exact = [{"case": s.label, "exact": bool(torch.equal(T.run(F.case(s)), F.case(s).picked))} for s in F.specs("onehot")]
    worst = {g: max(r["worst_error_over_tolerance"] for r in rows if r["group"] == g) for g in ("value", "deal")}
    worst_ref = {g: max(r["rounded_reference_over_tolerance"] for r in rows if r["group"] == g) for g in ("value", "deal")}
    worst_case = max(rows, key=lambda r: r["worst_error_over_tolerance"])["case"]
    Path(args.out).write_text(json.dumps({"tolerance": "2^-8 |want| + 2^-8 softmax @ |v| + 1e-4", "compute_units": cus, "worst_ratio": worst,
                                          "worst_ratio_of_the_rounded_reference": worst_ref, "worst_case": worst_case,
                                          "one_hot_cases": len(exact), "one_hot_exact": sum(e["exact"] for e in exact),
                                          "cases": rows, "one_hot": exact}, indent=1) + "\n")
    print(f"{len(rows)} value and deal cases, worst error / tolerance: {worst} ({worst_case}), rounded reference {worst_ref}; "
          f"{sum(e['exact'] for e in exact)} / {len(exact)} one-hot cases exact -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
