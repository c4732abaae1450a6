"""Writes profiles/stage_ops_parity.json: for every fp32 value case of tests/test_gpu_stage_ops.py (token assembly, L2 normalise)
the kernel's worst error against the float64 reference, the float32-torch yardstick of the same case, their ratio and the
tolerance the test applies (4 x the yardstick, floored at 8 * 2^-24 of the row's largest magnitude).  Run on an MI355X after the
library is built:  python tools/stage_ops_parity_report.py [--out PATH]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests"):
    sys.path.insert(0, str(p))

import stage_cases as S                            # noqa: E402
import test_gpu_stage_ops as T                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stage_ops_parity.json"))
    args = ap.parse_args()
    rows = []
    for stage in ("assemble_tokens", "l2norm_rows"):
        for c in S.cases(stage):
            got = T.run(stage, c)
            err, _ = S.f32_error(got, c.want)
            try:
                S.check(stage, c, got)
                within = True
            except AssertionError:
                within = False
            rows.append({"stage": stage, "case": c.label, "kernel_max_error": float(err.max()), "float32_torch_yardstick": c.yardstick,
                         "ratio": float(err.max()) / c.yardstick if c.yardstick > 0 else None,
                         "allowed_factor": S.F32_FACTOR, "within_tolerance": within})
    worst = {s: max((r["ratio"] or 0.0) for r in rows if r["stage"] == s) for s in ("assemble_tokens", "l2norm_rows")}
    Path(args.out).write_text(json.dumps({"floor": "8 * 2^-24 * max|row|", "worst_ratio": worst, "cases": rows}, indent=1) + "\n")
    print(f"{len(rows)} cases, worst kernel error / float32-torch error: {worst} -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
