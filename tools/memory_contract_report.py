"""Writes profiles/memory_contract.json: per entry point and case family of tests/test_gpu_memory_contract.py the declared
workspace bytes, the highest workspace offset any poison pattern shows as written, the guard result and the poison-independence
result.  Run on an MI355X after the library is built:  python tools/memory_contract_report.py [--out PATH] [--markdown]"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "tests" / "golden"):
    sys.path.insert(0, str(p))

import arena as A                                  # noqa: E402
import test_gpu_memory_contract as T               # noqa: E402


def measure(case):
    row = {"entry": case.entry, "family": case.family, "case": case.label, "workspace_bytes": case.need, "high_water": None,
           "guards": "intact", "poison_independent": True}
    base, high = None, -1
    for pattern in A.PATTERNS:
        try:
            got, hw = T.fresh(case, pattern)
        except A.GuardViolation as exc:
            row["guards"] = str(exc)
            return row
        high = max(high, hw)
        if base is None:
            base = got
        else:
            try:
                T._same(base, got, pattern)
            except AssertionError as exc:
                row["poison_independent"] = str(exc)
    if case.need is not None:
        row["high_water"] = high
        row["untouched_tail_bytes"] = case.need - 1 - high
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "memory_contract.json"))
    ap.add_argument("--markdown", action="store_true", help="also print the per-family table")
    args = ap.parse_args()
    cases = [c for make in T.CASES.values() for c in make()]
    cases += [T.Encoder(name, b, s, f) for name, bs in T.ENCODER_BATCHES.items() for b in bs for s, f in ((2, 1), (1, 0))]
    rows = [measure(c) for c in cases]
    families = {}
    for r in rows:                                   # one line per entry point and family: the case with the least untouched tail
        f = families.setdefault((r["entry"], r["family"]), {"entry": r["entry"], "family": r["family"], "cases": 0,
                                                             "workspace_bytes": [], "min_untouched_tail_bytes": None,
                                                             "tightest_case": None, "guards": "intact", "poison_independent": True})
        f["cases"] += 1
        if r["workspace_bytes"] is not None:
            f["workspace_bytes"].append(r["workspace_bytes"])
            tail = r.get("untouched_tail_bytes")
            if tail is not None and (f["min_untouched_tail_bytes"] is None or tail < f["min_untouched_tail_bytes"]):
                f["min_untouched_tail_bytes"], f["tightest_case"] = tail, {k: r[k] for k in ("case", "workspace_bytes", "high_water")}
        if r["guards"] != "intact":
            f["guards"] = r["guards"]
        if r["poison_independent"] is not True:
            f["poison_independent"] = r["poison_independent"]
    fam = list(families.values())
    for f in fam:
        w = f.pop("workspace_bytes")
        f["workspace_bytes_range"] = [min(w), max(w)] if w else None
    Path(args.out).write_text(json.dumps({"guard_bytes": A.GUARD_BYTES, "patterns": {k: f"0x{v:08X}" for k, v in A.PATTERNS.items()},
                                          "families": fam, "cases": rows}, indent=1) + "\n")
    if args.markdown:
        print("| entry point | family | cases | workspace bytes | tightest: high water / declared | guards | poison-independent |")
        print("|---|---|---|---|---|---|---|")
        for f in fam:
            t = f["tightest_case"]
            print(f"| {f['entry']} | {f['family']} | {f['cases']} | {f['workspace_bytes_range'] or '-'} | "
                  f"{(str(t['high_water']) + ' / ' + str(t['workspace_bytes']) + ' (' + t['case'] + ')') if t else '-'} | "
                  f"{'intact' if f['guards'] == 'intact' else 'HIT'} | {'yes' if f['poison_independent'] is True else 'NO'} |")
    bad = [r for r in rows if r["guards"] != "intact" or r["poison_independent"] is not True]
    print(f"{len(rows)} cases, {len(bad)} with a guard hit or a poison dependence -> {args.out}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
