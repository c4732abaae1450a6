"""GPU: the memory contract of the batched per-event calls, with the instrument and the six assertions of
tests/test_gpu_memory_contract.py: every device buffer carved from a poisoned, guarded arena (tests/arena.py) at its exact
documented size; guards intact, outputs bitwise equal under the three poison patterns and both workspace alignments, bitwise
what the Python shim returns, nothing written past the documented extent, the same result after another shape used the
workspace, and refusal at need - 1 with workspace and outputs still pure pattern.

hmm_cosine_topk_segmented_multi: cases on its branch points -- 1, 16 and 17 questions (one pass, a full pass, a second pass);
the small-event and the large-event selection shape; k = 64 (the last matrix-core k) and k = 65 (one single-question scan per
question); an empty event first, in the middle and last; row counts that are not a multiple of the 16-row tile.
hmm_rank_segment_hits_multi takes no workspace: guards and poison on its inputs and outputs.
"""
import numpy as np
import pytest
import torch

import test_gpu_memory_contract as M

pytestmark = pytest.mark.gpu
DEV = M.DEV

SMALL = [0, 1, 3, 7, 0, 64, 65, 200, 1, 1023, 2, 300, 0]          # 1666 rows (16 x 104 + 2) in 13 events: the 1024-key selection
LARGE = [0, 1, 5000, 4097, 0, 12000, 2, 0]                          # 21100 rows (16 x 1318 + 12): events beyond one 4096-key piece


class SegmentedMulti(M.Case):
    entry = "hmm_cosine_topk_segmented_multi"

    def __init__(self, lengths, nq, k):
        super().__init__()
        _, lib = M._L()
        self.lengths, self.nq, self.k, self.E, self.n = lengths, nq, k, len(lengths), sum(lengths)
        self.family = "segments multi " + ("small" if self.n <= 1024 * self.E and k <= 64 else "large") + (", k>64" if k > 64 else "")
        self.label = f"E={self.E},n={self.n},q={nq},k={k}"
        store = M._store(self.n)
        self.fs = M._fs(store)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=DEV)
        self.inputs = {"store": store, "queries": M._rand((nq, 1024), 90 + nq + k), "offsets": offs}
        slots = nq * self.E
        self.outs = {"idx": 8 * slots * k, "sims": 4 * slots * k, "counts": 4 * slots}        # -1 / 0 padded: all of it is written
        self.need = lib.hmm_cosine_topk_segmented_multi_workspace_bytes(self.n, self.E, nq, k)
        assert self.need == lib.hmm_cosine_topk_segmented_multi_workspace_bytes(self.n, self.E, 16, k)

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_cosine_topk_segmented_multi(p["store"], self.n, 1024, p["queries"], self.nq, p["offsets"], self.E, self.k,
                                                   p["idx"], p["sims"], p["counts"], ws, ws_bytes, None)

    def compare(self, raw):
        got = super().compare(raw)
        idx = got["idx"].view(torch.int64).view(self.nq, self.E, self.k)
        sims = got["sims"].view(torch.int32).view(self.nq, self.E, self.k)
        counts = got["counts"].view(torch.int32).view(self.nq, self.E)
        for e, n in enumerate(self.lengths):                     # the documented padding and no more: -1 / 0 behind min(k, n_e) entries
            kk = min(self.k, n)
            assert counts[:, e].eq(kk).all(), (e, counts[:, e])
            assert idx[:, e, kk:].eq(-1).all() and sims[:, e, kk:].eq(0).all(), e
            assert idx[:, e, :kk].ge(0).all() and idx[:, e, :kk].lt(max(n, 1)).all(), e
        return got

    def shim(self):
        idx, sims, counts = self.fs.search_segments_multi_device(self.inputs["queries"], self.inputs["offsets"], self.k)
        return {"idx": idx, "sims": sims, "counts": counts}


class RankHitsMulti(M.Case):
    entry, family = "hmm_rank_segment_hits_multi", "rank segment hits multi"

    def __init__(self, lengths, nq, k, keep):
        super().__init__()
        from hippomm_amd.vector_ops import EventStore
        self.nq, self.k, self.keep, self.E = nq, k, keep, len(lengths)
        self.label = f"E={self.E},q={nq},k={k},keep={keep}"
        self.es = EventStore.from_device_rows(M._store(sum(lengths)), lengths)
        self.q = M._rand((nq, 1024), 17 + nq)
        idx, sims, counts = self.es.search_segments_multi_device(self.q, self.es.offsets, k)
        self.inputs = {"idx": idx.clone(), "sims": sims.clone(), "counts": counts.clone()}
        self.outs = {"event": 8 * nq * keep, "row": 8 * nq * keep, "sim": 4 * nq * keep, "n_out": 4 * nq}   # -1 / -1 / 0 padded to `keep`

    def call(self, lib, p, ws, ws_bytes):
        return lib.hmm_rank_segment_hits_multi(p["idx"], p["sims"], p["counts"], self.nq, self.E, self.k, self.keep, p["event"],
                                               p["row"], p["sim"], p["n_out"], None)

    def compare(self, raw):
        n = raw["n_out"].view(torch.int32)
        ev = raw["event"].view(torch.int64).view(self.nq, self.keep)
        row = raw["row"].view(torch.int64).view(self.nq, self.keep)
        sim = raw["sim"].view(torch.float32).view(self.nq, self.keep)
        out = {"n_out": n.clone()}
        for q in range(self.nq):
            m = int(n[q])
            assert 0 <= m <= self.keep
            assert ev[q, m:].eq(-1).all() and row[q, m:].eq(-1).all() and sim[q, m:].view(torch.int32).eq(0).all(), q
            out.update({f"event{q}": ev[q, :m].contiguous(), f"row{q}": row[q, :m].contiguous(), f"sim{q}": sim[q, :m].contiguous()})
        return out

    def shim(self):
        hits = self.es.top_hits_multi(self.q, self.k, self.keep)
        out = {"n_out": torch.tensor([len(h) for h in hits], dtype=torch.int32)}
        for q, h in enumerate(hits):
            out.update({f"event{q}": torch.tensor([x[0] for x in h], dtype=torch.int64),
                        f"row{q}": torch.tensor([x[1] for x in h], dtype=torch.int64),
                        f"sim{q}": torch.tensor([x[2] for x in h], dtype=torch.float64).float()})
        return out


CASES = {
    "segmented_multi_small": lambda: [SegmentedMulti(SMALL, nq, 5) for nq in (1, 16, 17)] +
                                     [SegmentedMulti(SMALL, 3, 64), SegmentedMulti(SMALL, 3, 65), SegmentedMulti([1], 1, 5),
                                      SegmentedMulti([0, 17, 0], 2, 5)],
    "segmented_multi_large": lambda: [SegmentedMulti(LARGE, 1, 5), SegmentedMulti(LARGE, 16, 5), SegmentedMulti(LARGE, 17, 64),
                                      SegmentedMulti(LARGE, 3, 65)],
    "rank_hits_multi": lambda: [RankHitsMulti([1, 3, 7, 64], 1, 5, 5), RankHitsMulti([2, 1], 17, 5, 64),
                                RankHitsMulti([30] * 900, 3, 5, 5), RankHitsMulti([0, 2, 0], 4, 5, 7)],
}
REUSE = [lambda: (SegmentedMulti(LARGE, 17, 64), SegmentedMulti(SMALL, 1, 5)),
         lambda: (SegmentedMulti(LARGE, 3, 65), SegmentedMulti(SMALL, 16, 5)),
         lambda: (SegmentedMulti(SMALL, 17, 5), SegmentedMulti(LARGE, 3, 65)),
         lambda: (SegmentedMulti(SMALL, 3, 65), SegmentedMulti(LARGE, 16, 5))]


@pytest.mark.parametrize("group", list(CASES))
def test_guards_poison_independence_shim_extent_refusal(group):
    failures = []
    for case in CASES[group]():
        try:
            M.check_case(case)
        except AssertionError as exc:                             # every case of the group reports, not only the first
            failures.append(f"{case}: {exc}")
    assert not failures, "\n".join(failures)


def test_reuse_of_one_workspace_across_shapes():
    failures = []
    for make in REUSE:
        x, y = make()
        try:
            M.check_reuse(x, y)
        except AssertionError as exc:
            failures.append(f"{x} then {y}: {exc}")
    assert not failures, "\n".join(failures)
