"""GPU: the memory contract of hmm_rank_segment_hits_filtered[_multi] (include/hippomm_hip.h), with the instrument of
tests/test_gpu_memory_contract.py: every device buffer -- the three inputs, row_limits, defer and the nine outputs -- is carved
from a poisoned, guarded arena (tests/arena.py) at exactly its documented size.  Under each of the three poison patterns:

  * the guards on both sides of every buffer are intact and the inputs are unchanged;
  * every DECLARED output byte is written: hits, counts and the deferred events' list are full arrays (-1 / -1 / 0 / -1 padding
    included), the compacted deferred slices reach n_deferred * k entries (their counts n_deferred) -- all of them equal to the
    model's values (tests/relevant_hits_model.py), so none can be a leftover pattern byte;
  * the compacted arrays are still pure pattern from n_deferred * k (counts: n_deferred) on, per question: the header documents
    them as NOT written.

The calls take no workspace.  Every byte written or inspected lies inside the arena's own allocation; nothing here provokes a
fault."""
import numpy as np
import pytest
import torch

import arena as A
import relevant_hits_model as model
from test_gpu_relevant_hits import hits

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = np.float32(0.4)

# (Q or None for the single form, E, k, keep, with row_limits, defer pattern)
CASES = [(None, 1, 5, 5, True, "all"), (None, 7, 5, 5, False, None), (None, 1025, 5, 64, True, "some"), (None, 2049, 3, 130, True, "all"),
         (None, 13108, 5, 70, True, "some"), (None, 300, 5, 1024, True, "none"),
         (1, 9, 5, 5, True, "all"), (17, 1030, 5, 70, True, "some"), (3, 13108, 5, 5, False, "all"), (4, 40, 8, 1024, True, None)]


def _pattern_bytes(pattern, nbytes):
    return np.tile(np.frombuffer(int(pattern).to_bytes(4, "little"), np.uint8), nbytes // 4 + 1)[:nbytes]


def _inputs(Q, E, k, with_limits, defer):
    parts = [hits(E, k, seed=7 * E + q, lo=0.1, hi=0.45) for q in range(Q or 1)]
    idx, sims, counts = (np.stack([p[i] for p in parts]) for i in range(3))
    rng = np.random.default_rng(E)
    limits = rng.integers(0, 41, E).astype(np.int64) if with_limits else None
    flags = {None: None, "none": np.zeros(E, np.uint8), "all": np.ones(E, np.uint8), "some": (rng.random(E) < 0.5).astype(np.uint8)}[defer]
    return idx, sims, counts.astype(np.int32), limits, flags


@pytest.mark.parametrize("Q,E,k,keep,with_limits,defer", CASES)
def test_guards_inputs_declared_bytes_and_the_unwritten_tails(Q, E, k, keep, with_limits, defer):
    from hippomm_amd import _lib
    _lib.require_gpu()
    lib = _lib.load()
    nq = Q or 1
    idx, sims, counts, limits, flags = _inputs(Q, E, k, with_limits, defer)
    want = [model.rank_filtered(idx[q], sims[q], counts[q], keep, limits, flags, T) for q in range(nq)]
    inputs = {"idx": idx, "sims": sims, "counts": counts}
    if limits is not None:
        inputs["row_limits"] = limits
    if flags is not None:
        inputs["defer"] = flags
    outs = {"event": (np.int64, keep), "row": (np.int64, keep), "sim": (np.float32, keep), "n": (np.int32, 1), "deferred_event": (np.int32, E),
            "n_deferred": (np.int32, 1), "deferred_idx": (np.int64, E * k), "deferred_sim": (np.float32, E * k), "deferred_count": (np.int32, E)}
    sizes = [a.nbytes for a in inputs.values()] + [nq * n * np.dtype(t).itemsize for t, n in outs.values()]
    for pattern in A.PATTERNS.values():
        ar = A.GuardedArena(A.needed_bytes(sizes), DEV, pattern)
        ptr, views = {}, {}
        for name, a in inputs.items():
            views[name] = ar.put(torch.from_numpy(a), name)
            ptr[name] = ar.address(views[name])
        for name, (t, n) in outs.items():
            views[name] = ar.carve(nq * n * np.dtype(t).itemsize, "out:" + name)
            ptr[name] = ar.address(views[name])
        fn = lib.hmm_rank_segment_hits_filtered_multi if Q is not None else lib.hmm_rank_segment_hits_filtered
        rc = fn(ptr["idx"], ptr["sims"], ptr["counts"], *((Q,) if Q is not None else ()), E, k, keep, ptr.get("row_limits"), ptr.get("defer"),
                float(T), *[ptr[name] for name in outs], None)
        torch.cuda.synchronize()
        assert rc == 0, lib.hmm_last_error()
        ar.check_guards()
        for name, a in inputs.items():
            assert views[name].cpu().numpy().tobytes() == a.tobytes(), f"input '{name}' was modified"
        got = {name: views[name].cpu().numpy().view(t).reshape(nq, n) for name, (t, n) in outs.items()}
        for q in range(nq):
            w, m = want[q], want[q]["n_deferred"]
            assert int(got["n"][q, 0]) == w["n"] and int(got["n_deferred"][q, 0]) == m, (q, hex(pattern))
            for name in ("event", "row", "sim", "deferred_event"):          # whole arrays, padding included
                assert got[name][q].tobytes() == w[name].tobytes(), (q, name, hex(pattern))
            for name, front in (("deferred_idx", m * k), ("deferred_sim", m * k), ("deferred_count", m)):
                t, n = outs[name]
                assert got[name][q, :front].tobytes() == np.ascontiguousarray(w[name]).astype(t).tobytes(), (q, name, hex(pattern))
                tail = got[name][q, front:].view(np.uint8)
                # the arena's pattern is phase-locked to 4 bytes and every carve and every entry here starts on a multiple of 4
                at = (q * n + front) * np.dtype(t).itemsize
                assert at % 4 == 0 and tail.tobytes() == _pattern_bytes(pattern, tail.size).tobytes(), \
                    f"question {q}: '{name}' was written past its {front} compacted entries (pattern {pattern:#x})"
    if defer in ("all", "some") and E >= 7:                                 # the cases do defer events
        assert any(w["n_deferred"] > 0 for w in want)
