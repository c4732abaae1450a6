"""The memory contract of the batched scans through the bf16 shadow (hmm_cosine_topk_multi_prefilter,
hmm_cosine_topk_segmented_multi_prefilter), through the guarded, poisoned arena of tests/arena.py and the checks of
tests/test_gpu_memory_contract.py: guards intact, outputs bitwise equal under the three poison patterns and both workspace
alignments, nothing written past the documented extents, the same result after another shape used the workspace, and a workspace
one byte short refused before any launch -- at one shape on each side of the dispatch limit and one that takes the fallback."""
import numpy as np
import pytest
import torch

import arena as A  # noqa: F401  (the instrument; used through the helpers below)
from test_gpu_memory_contract import DEV, Case, _fs, _L, _rand, _store, check_case, check_reuse

pytestmark = pytest.mark.gpu


class MultiPrefilter(Case):
    entry = "hmm_cosine_topk_multi_prefilter"

    def __init__(self, n, nq, k, kind, route):
        super().__init__()
        _, lib = _L()
        self.n, self.nq, self.k, self.kk, self.route = n, nq, k, min(k, n), route      # route: "prefilter" | "fallback" | "exact"
        self.family, self.label = f"multi prefilter ({route})", f"n={n},q={nq},k={k},{kind}"
        store = _store(n, kind)
        self.fs = _fs(store).build_shadow()
        self.inputs = {"store": store, "shadow": self.fs._shadow, "queries": _rand((nq, 1024), 50 + nq)}
        self.outs = {"idx": 8 * nq * k, "sims": 4 * nq * k, "n_out": 4 * nq, "stats": 8 * nq}
        self.need = lib.hmm_cosine_topk_multi_prefilter_workspace_bytes(n, nq, k)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_cosine_topk_multi_prefilter(p["store"], p["shadow"], self.n, 1024, p["queries"], self.nq, self.k, p["idx"],
                                                   p["sims"], p["n_out"], p["stats"], ws, ws_bytes, None)

    def compare(self, raw):                                      # rows of stride k; the first min(k, n_rows) entries of a row are valid
        stats = raw["stats"].view(torch.int32).view(self.nq, 2)
        if self.route == "exact":
            assert (stats == -1).all(), stats.tolist()
        elif self.route == "fallback":                           # the conditional exact pass answered, inside the same call
            assert ((stats[:, 1] > 0) | (stats[:, 0] > 1024)).any(), stats.tolist()
        else:
            assert (stats[:, 1] == 0).all() and (stats[:, 0] >= self.k).all() and (stats[:, 0] <= 1024).all(), stats.tolist()
        return {"idx": raw["idx"].view(torch.int64).view(self.nq, self.k)[:, : self.kk].contiguous(),
                "sims": raw["sims"].view(torch.float32).view(self.nq, self.k)[:, : self.kk].contiguous(), "n_out": raw["n_out"],
                "stats": raw["stats"]}

    def shim(self):                                              # the EXACT function through the Python layer: the same bytes
        idx, sims = _fs(self.inputs["store"]).search_multi_device(self.inputs["queries"], self.k, prefilter=False)
        return {"idx": idx, "sims": sims, "n_out": torch.full((self.nq,), self.kk, dtype=torch.int32)}


class SegMultiPrefilter(Case):
    entry = "hmm_cosine_topk_segmented_multi_prefilter"

    def __init__(self, sizes, nq, k, kind, route):
        super().__init__()
        _, lib = _L()
        self.n, self.E, self.nq, self.k, self.route = sum(sizes), len(sizes), nq, k, route   # route: "prefilter" | "whole" | "exact"
        self.family, self.label = f"segmented multi prefilter ({route})", f"sizes={sizes},q={nq},k={k},{kind}"
        if kind == "scene":                                      # near-identical rows: every row of an event is a candidate
            store = (_rand((1, 1024), 5) + 1e-3 * _rand((self.n, 1024), 6)).contiguous()
        else:
            store = _store(self.n, kind)
        self.fs = _fs(store).build_shadow()
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)
        self.inputs = {"store": store, "shadow": self.fs._shadow, "queries": _rand((nq, 1024), 60 + nq), "offsets": self.offsets}
        self.outs = {"idx": 8 * nq * self.E * k, "sims": 4 * nq * self.E * k, "n_out": 4 * nq * self.E, "stats": 8}
        self.need = lib.hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes(self.n, self.E, nq, k)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_cosine_topk_segmented_multi_prefilter(p["store"], p["shadow"], self.n, 1024, p["queries"], self.nq, p["offsets"],
                                                             self.E, self.k, p["idx"], p["sims"], p["n_out"], p["stats"], ws,
                                                             ws_bytes, None)

    def compare(self, raw):
        got = super().compare(raw)
        whole, cand = got["stats"].view(torch.int32).tolist()
        if self.route == "exact":
            assert (whole, cand) == (-1, -1)
        elif self.route == "whole":                              # events whose candidates do not fit: every row re-scored
            assert whole > 0 and cand > 1024, (whole, cand)
        else:
            assert whole == 0 and cand > 0, (whole, cand)
        return got

    def shim(self):                                              # the EXACT function through the Python layer: the same bytes
        idx, sims, counts = _fs(self.inputs["store"]).search_segments_multi_device(self.inputs["queries"], self.offsets, self.k)
        return {"idx": idx, "sims": sims, "n_out": counts}


RAGGED = [1, 3, 7, 64, 65, 200, 1, 1023, 2, 300]                  # 1666 rows in 10 events: at least 128 per event on average
RAGGED_TINY = [1, 2, 3, 50, 0, 7]                                 # below it: the call IS the exact function
SCENE = [2000, 300, 1700]                                         # near-identical rows: two events with more candidates than the buffer holds

CASES = {
    "flat": lambda: [MultiPrefilter(20000, 5, 5, "random", "prefilter"), MultiPrefilter(16383, 5, 5, "random", "exact"),
                     MultiPrefilter(20000, 17, 5, "ties", "fallback")],
    "per event": lambda: [SegMultiPrefilter(RAGGED, 5, 5, "zero_rows", "prefilter"), SegMultiPrefilter(RAGGED_TINY, 5, 5, "random", "exact"),
                          SegMultiPrefilter(SCENE, 17, 5, "scene", "whole")],
}


@pytest.mark.parametrize("group", list(CASES))
def test_guards_poison_independence_extent_refusal(group):
    for case in CASES[group]():
        check_case(case)


@pytest.mark.parametrize("group", list(CASES))
def test_reuse_of_one_workspace_across_shapes(group):
    cases = CASES[group]()
    check_reuse(cases[2], cases[0])
    check_reuse(cases[0], cases[2])
    check_reuse(cases[0], cases[1])
