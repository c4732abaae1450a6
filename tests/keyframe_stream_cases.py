"""Shared by the key-frame stream tests (plain helper module, not a fixture plugin): the batch partitions, the golden lists, the
prefix rule a growing selection must satisfy after every batch, and a numpy model of hmm_keyframe_extend's five steps."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np


_DOC = json.loads((Path(__file__).resolve().parent / "golden" / "select_golden.json").read_text())
GOLD = {name: case["kept"] for name, case in _DOC["cases"].items()}
GOLD.update({name: case["kept_exact_definition"] for name, case in _DOC["inband_cases"].items()})
SHA = {name: case["input_sha256"] for part in ("cases", "inband_cases") for name, case in _DOC[part].items()}

CYCLE = (1, 2, 3, 63, 64, 65)


def batches(n: int, sizes) -> list:
    """[(start, stop)] covering range(n) with batch sizes taken from `sizes` in turn (cycling)."""
    out, at, i = [], 0, 0
    while at < n:
        step = min(int(sizes[i % len(sizes)]), n - at)
        out.append((at, at + step))
        at += step
        i += 1
    return out


def partitions(name: str, n: int) -> dict:
    """The partitions of the issue: everything at once, row by row (small inputs), the cycle 1,2,3,63,64,65, 33s and 32s."""
    if name == "n3600_clusters600":
        return {"450": batches(n, [450]), "32": batches(n, [32])}
    parts = {"all": batches(n, [n]), "cycle": batches(n, CYCLE), "33": batches(n, [33]), "32": batches(n, [32])}
    if n <= 300:
        parts["1"] = batches(n, [1])
    return parts


def expected_after(final_kept, n_seen: int) -> list:
    """What kept() must list once n_seen rows have arrived, given the one-shot list of the whole input: the list restricted to the
    rows seen (the greedy rule is causal), or every row while n_seen <= 2 (hippocampal_memory.py:947-948)."""
    if n_seen <= 2:
        return list(range(n_seen))
    return [i for i in final_kept if i < n_seen]


# ---- numpy model of the five steps -------------------------------------------------------------------------------------------
def _unit(f32: np.ndarray) -> np.ndarray:
    """normalize_rows_kernel: fp64 sum of squares, fp32 norm, one fp32 division."""
    norm = np.sqrt(np.sum(f32.astype(np.float64) ** 2, axis=1)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (f32 / norm[:, None]).astype(np.float32)


def _hits(a: np.ndarray, b: np.ndarray, thr: np.float32) -> np.ndarray:
    """not (S < thr) with S = every dot accumulated in fp64 and rounded to fp32 once; a NaN similarity blocks."""
    with np.errstate(invalid="ignore"):
        s = (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)
        return ~(s < thr)


class ModelSelector:
    """State: the normalised kept rows, their global indices, the rows seen."""

    def __init__(self, similarity_threshold: float = 0.9):
        self.thr = np.float32(similarity_threshold)
        self.kept_rows = np.zeros((0, 1024), np.float32)
        self.kept_idx = []
        self.n_seen = 0

    def extend(self, rows: np.ndarray):
        fn = _unit(np.ascontiguousarray(rows, dtype=np.float32))                       # 1 normalise
        m = fn.shape[0]
        blocked = _hits(fn, self.kept_rows, self.thr).any(axis=1) if len(self.kept_idx) else np.zeros(m, bool)   # 2 new x kept
        adj = _hits(fn, fn, self.thr)                                                  # 3 new x new
        adj = np.triu(adj) | np.triu(adj).T                                            #   (each unordered pair evaluated once)
        new_rows = []
        for i in range(m):                                                             # 4 greedy, seeded
            if self.n_seen + i == 0 or not blocked[i]:
                self.kept_idx.append(self.n_seen + i)
                new_rows.append(i)
                blocked |= adj[i]
        self.kept_rows = np.concatenate([self.kept_rows, fn[new_rows]])                # 5 append the kept rows
        self.n_seen += m

    def kept(self) -> list:
        return list(range(self.n_seen)) if self.n_seen <= 2 else list(self.kept_idx)
