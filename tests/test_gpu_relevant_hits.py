"""GPU: hmm_rank_segment_hits_filtered[_multi] on hand-made (E, k) arrays against tests/relevant_hits_model.py (no scan is
involved), then EventStore.relevant_hits[_multi] and hippomm_amd.retrieval end to end on small stores.

The kernel's answer is exact: a selection and a copy, no arithmetic.  Every comparison here is bitwise."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import relevant_hits_model as model
import retrieval_recipes as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = Path(__file__).resolve().parent.parent
T = np.float32(0.4)
BELOW, ABOVE = np.nextafter(T, np.float32(0)), np.nextafter(T, np.float32(1))
SENTINEL = 0x5A


def _L():
    from hippomm_amd import _lib
    _lib.require_gpu()
    return _lib, _lib.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(idx, sims, counts, keep, row_limits=None, defer=None, min_similarity=T):
    """The C entry point on (E, k) arrays (single form) or (Q, E, k) arrays (multi form) -> a list of per-question dicts shaped like
    model.rank_filtered's, the deferred arrays cut to the written front; what lies behind it must still be the sentinel."""
    _lib, lib = _L()
    idx, sims, counts = np.asarray(idx, np.int64), np.asarray(sims, np.float32), np.asarray(counts, np.int32)
    multi = idx.ndim == 3
    Q, (E, k) = (idx.shape[0] if multi else 1), idx.shape[-2:]
    d_in = [_dev(idx), _dev(sims), _dev(counts)]
    lim = _dev(np.asarray(row_limits, np.int64)) if row_limits is not None else None
    dfr = _dev(np.asarray(defer, np.uint8)) if defer is not None else None
    shapes = [((Q, keep), torch.int64), ((Q, keep), torch.int64), ((Q, keep), torch.float32), ((Q,), torch.int32),
              ((Q, E), torch.int32), ((Q,), torch.int32), ((Q, E * k), torch.int64), ((Q, E * k), torch.float32), ((Q, E), torch.int32)]
    outs = [torch.full((int(np.prod(s)) * torch.empty(0, dtype=t).element_size(),), SENTINEL, dtype=torch.uint8, device=DEV)
            for s, t in shapes]
    ptrs = [o.data_ptr() for o in outs]
    lead = (Q,) if multi else ()
    fn = lib.hmm_rank_segment_hits_filtered_multi if multi else lib.hmm_rank_segment_hits_filtered
    rc = fn(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), *lead, E, k, keep, lim.data_ptr() if lim is not None else None,
            dfr.data_ptr() if dfr is not None else None, float(min_similarity), *ptrs, _lib.stream_ptr())
    assert rc == 0, lib.hmm_last_error()
    torch.cuda.synchronize()
    for t, a in zip(d_in, (idx, sims, counts)):
        assert t.cpu().numpy().tobytes() == a.tobytes(), "an input was modified"
    ev, row, val, n, d_ev, n_d, d_idx, d_sim, d_cnt = [o.view(t).view(s).cpu().numpy() for o, (s, t) in zip(outs, shapes)]
    sent64, sent32 = np.frombuffer(bytes([SENTINEL]) * 8, np.int64)[0], np.frombuffer(bytes([SENTINEL]) * 4, np.int32)[0]
    res = []
    for q in range(Q):
        m = int(n_d[q])
        assert 0 <= m <= E
        assert (d_idx[q, m * k:] == sent64).all() and (d_sim[q, m * k:].view(np.int32) == sent32).all() and (d_cnt[q, m:] == sent32).all(), \
            "the deferred arrays were written past n_deferred"
        res.append({"event": ev[q], "row": row[q], "sim": val[q], "n": int(n[q]), "deferred_event": d_ev[q], "n_deferred": m,
                    "deferred_idx": d_idx[q, :m * k].reshape(m, k), "deferred_sim": d_sim[q, :m * k].reshape(m, k),
                    "deferred_count": d_cnt[q, :m]})
    return res


def same(got, want, what=""):
    assert got["n"] == want["n"] and got["n_deferred"] == want["n_deferred"], (what, got["n"], want["n"], got["n_deferred"], want["n_deferred"])
    for name in ("event", "row", "deferred_event", "deferred_idx", "deferred_count"):
        assert np.array_equal(got[name], want[name]), (what, name, got[name][:8], want[name][:8])
    for name in ("sim", "deferred_sim"):                          # bits, NaN payloads included
        assert got[name].shape == want[name].shape and got[name].tobytes() == np.asarray(want[name], np.float32).tobytes(), (what, name)


def check(idx, sims, counts, keep, row_limits=None, defer=None, min_similarity=T, what=""):
    got = run(idx, sims, counts, keep, row_limits, defer, min_similarity)[0]
    same(got, model.rank_filtered(idx, sims, counts, keep, row_limits, defer, min_similarity), what)
    return got


def hits(E, k, seed, rows=40, lo=0.0, hi=1.0, ties=True):
    """Per-event hits as a scan leaves them: sorted descending inside an event, -1 / 0 behind the count; counts from 0 to k; with
    ``ties`` the similarities come from 200 values, so equal ones occur across and inside events."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, k + 1, E).astype(np.int32)
    counts[rng.random(E) < 0.6] = k
    sims = (rng.integers(0, 200, (E, k)) / 200.0 * (hi - lo) + lo if ties else rng.uniform(lo, hi, (E, k))).astype(np.float32)
    sims = -np.sort(-sims, axis=1)
    idx = rng.integers(0, rows, (E, k)).astype(np.int64)
    slot = np.arange(k)[None, :]
    idx[slot >= counts[:, None]] = -1
    sims[slot >= counts[:, None]] = 0.0
    return idx, sims, counts


@pytest.mark.parametrize("E,k", [(13107, 5), (8192, 8), (13108, 5)])        # 65 535 and 65 536 slots: quick route; 65 540: windowed
@pytest.mark.parametrize("keep", [5, 64, 130])
def test_both_routes_at_their_edge(E, k, keep):
    idx, sims, counts = hits(E, k, seed=E + keep)
    rng = np.random.default_rng(1)
    limits, defer = rng.integers(0, 41, E), rng.random(E) < 0.3
    check(idx, sims, counts, keep, limits, defer, what="limits+defer")
    check(idx, sims, counts, keep, limits, None, what="limits")
    sparse = np.where(rng.random(E) < 0.999, 0, limits)                     # nearly everything filtered: fewer than keep per round
    check(idx, sims, counts, keep, sparse, None, what="sparse")


@pytest.mark.parametrize("E", [1, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("pattern", ["none", "all", "alternating"])
def test_ordered_compaction_and_padding(E, pattern):
    idx, sims, counts = hits(E, 5, seed=E, lo=0.2, hi=0.6)
    counts[:] = np.maximum(counts, 1)
    idx, sims = np.where(idx < 0, 0, idx), sims
    sims[:, 0] = np.where(np.arange(E) % 3 == 0, np.float32(0.7), np.float32(0.1))      # a third of the events stay above the threshold
    sims = -np.sort(-sims, axis=1)
    defer = {"none": np.zeros(E, bool), "all": np.ones(E, bool), "alternating": np.arange(E) % 2 == 1}[pattern]
    got = check(idx, sims, counts, 64, np.full(E, 40), defer)
    want = [e for e in range(E) if defer[e] and sims[e, 0] < T]
    assert got["deferred_event"][:len(want)].tolist() == want and (got["deferred_event"][len(want):] == -1).all()
    if pattern == "none":
        assert got["n_deferred"] == 0
        same(run(idx, sims, counts, 64, np.full(E, 40), None)[0], got)      # a null defer is an all-zero defer


def test_counts_of_zero_and_partial_counts():
    idx, sims, counts = hits(300, 5, seed=3, lo=0.0, hi=0.39)
    counts[::2], counts[1::2] = 0, np.maximum(counts[1::2], 1)
    idx[::2], sims[::2] = -1, 0.0
    got = check(idx, sims, counts, 64, None, np.ones(300, bool))
    assert got["n"] == 0 and got["n_deferred"] == 150                        # an event without a hit is never deferred (nor ranked)
    check(idx, sims, counts, 64, None, None)
    check(idx, sims, counts, 7, np.full(300, 20), np.arange(300) % 3 == 0)
    zero = np.zeros(300, np.int32)
    got = check(np.full((300, 5), -1), np.zeros((300, 5), np.float32), zero, 5, None, np.ones(300, bool))
    assert got["n"] == 0 and got["n_deferred"] == 0


def test_row_limits_from_zero_to_beyond_every_row():
    n, k = 30, 5
    rows = np.array([[n - 1, 0, 1, n - 2, 2]] * 5, np.int64)
    sims = np.linspace(0.9, 0.5, 25, dtype=np.float32).reshape(5, k)
    limits = np.array([0, 1, n - 1, n, 1 << 40], np.int64)
    got = check(rows, sims, np.full(5, k, np.int32), 64, limits)
    survivors = [(e, r) for e in range(5) for r in rows[e] if r < limits[e]]
    assert got["n"] == len(survivors) == 0 + 1 + 4 + 5 + 5
    assert sorted(zip(got["event"][:got["n"]].tolist(), got["row"][:got["n"]].tolist())) == sorted(survivors)


def test_threshold_at_float32_0_4_and_both_neighbours():
    # np.float32(x) < 0.4 is x < float32(0.4) under either numpy promotion rule: no fp32 lies strictly between 0.4 and float32(0.4)
    assert float(BELOW) < 0.4 < float(T) < float(ABOVE)
    sims = np.array([[BELOW, 0.1], [T, 0.1], [ABOVE, 0.1], [BELOW, 0.1]], np.float32)
    idx = np.zeros((4, 2), np.int64)
    got = check(idx, sims, np.full(4, 2, np.int32), 8, None, [1, 1, 1, 0])
    assert got["deferred_event"].tolist() == [0, -1, -1, -1] and got["n"] == 6
    assert [bool(np.float32(x) < 0.4) for x in (BELOW, T, ABOVE)] == [True, False, False]


def test_a_nan_best_similarity_never_defers_and_ranks_first():
    nan = np.float32("nan")
    sims = np.array([[0.3, 0.2, 0.1], [nan, 0.3, 0.1], [nan, nan, 0.2], [0.39, 0.1, 0.0]], np.float32)
    got = check(np.arange(12).reshape(4, 3), sims, np.full(4, 3, np.int32), 12, None, np.ones(4, bool))
    assert got["deferred_event"].tolist() == [0, 3, -1, -1]
    assert got["event"][:6].tolist() == [1, 2, 2, 1, 2, 1] and np.isnan(got["sim"][:3]).all() and got["n"] == 6


@pytest.mark.parametrize("threshold,deferred", [(np.inf, [0, 1, 3]), (-np.inf, []), (np.nan, [])])
def test_min_similarity_of_infinities_and_nan(threshold, deferred):
    sims = np.array([[0.9, 0.1], [-np.inf, -np.inf], [np.inf, 0.0], [-0.5, -0.6], [np.nan, 0.1]], np.float32)
    got = check(np.zeros((5, 2), np.int64), sims, np.full(5, 2, np.int32), 10, None, np.ones(5, bool), np.float32(threshold))
    assert got["deferred_event"][:got["n_deferred"]].tolist() == deferred


def test_equal_similarities_keep_event_then_slot_order():
    E, k = 700, 5
    sims = np.full((E, k), 0.5, np.float32)
    sims[::7] = 0.75
    idx = np.arange(E * k, dtype=np.int64).reshape(E, k)
    for keep in (5, 64, 200, 1024):
        got = check(idx, sims, np.full(E, k, np.int32), keep)
        assert (np.diff(got["row"][:100]) > 0).all()                         # rows number the positions: the order IS position order
    limits = np.where(np.arange(E) % 2 == 0, 1 << 40, 0)
    check(idx, sims, np.full(E, k, np.int32), 300, limits)


def test_everything_filtered_out():
    idx, sims, counts = hits(500, 5, seed=9)
    for keep in (1, 64, 65, 1024):
        got = check(idx, sims, counts, keep, np.zeros(500, np.int64))
        assert got["n"] == 0 and (got["event"] == -1).all() and (got["row"] == -1).all() and not got["sim"].view(np.int32).any()
    got = check(idx, np.where(sims > 0, sims * 0.3, sims).astype(np.float32), counts, 5, None, np.ones(500, bool))
    assert got["n"] == 0 and got["n_deferred"] == int((counts > 0).sum())


@pytest.mark.parametrize("keep", [1, 5, 64, 65, 128, 1024])
def test_keep_up_to_1024_in_rounds_of_64(keep):
    idx, sims, counts = hits(900, 5, seed=keep, ties=False)
    got = check(idx, sims, counts, keep, np.full(900, 30), np.arange(900) % 5 == 0)
    assert got["n"] == keep                                                  # thousands of candidates: every round is full
    idx, sims, counts = hits(900, 5, seed=keep + 1)                          # with ties across the rounds' boundaries
    check(idx, sims, counts, keep, np.full(900, 30))
    if keep == 128:                                                          # 100 survivors: the second round runs out
        limits = np.zeros(900, np.int64)
        limits[:20] = 1 << 40
        counts[:20], idx[:20] = 5, np.abs(idx[:20])
        got = check(idx, sims, counts, keep, limits)
        assert got["n"] == 100 and (got["event"][100:] == -1).all()
    if keep == 1024:                                                         # the windowed route, sixteen rounds
        idx, sims, counts = hits(13108, 5, seed=5)
        check(idx, sims, counts, keep, np.full(13108, 20), np.arange(13108) % 4 == 0)


def test_multi_slice_q_equals_the_single_call():
    Q, E, k = 19, 1030, 5
    parts = [hits(E, k, seed=100 + q, lo=0.2, hi=0.7) for q in range(Q)]
    idx, sims = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    counts = np.stack([p[2] for p in parts])
    rng = np.random.default_rng(4)
    limits, defer = rng.integers(0, 41, E), rng.random(E) < 0.5
    for keep in (5, 70):
        got = run(idx, sims, counts, keep, limits, defer)
        for q in range(Q):
            same(got[q], run(idx[q], sims[q], counts[q], keep, limits, defer)[0], f"question {q}")
        same(got[7], model.rank_filtered(idx[7], sims[7], counts[7], keep, limits, defer, T))
    assert len({g["n_deferred"] for g in got}) > 1                           # the questions do defer different events


@pytest.mark.parametrize("E,k,keep", [(2000, 5, 5), (13107, 5, 64), (13108, 5, 64), (3, 5, 64), (1, 1, 1)])
def test_without_rules_it_is_hmm_rank_segment_hits_bit_for_bit(E, k, keep):
    _lib, lib = _L()
    idx, sims, counts = hits(E, k, seed=E)
    sims[::11, 0] = np.nan
    got = run(idx, sims, counts, keep)[0]
    d = [_dev(idx), _dev(sims), _dev(counts)]
    ev, row = torch.empty(keep, dtype=torch.int64, device=DEV), torch.empty(keep, dtype=torch.int64, device=DEV)
    val, n = torch.empty(keep, dtype=torch.float32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    assert lib.hmm_rank_segment_hits(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), E, k, keep, ev.data_ptr(), row.data_ptr(),
                                     val.data_ptr(), n.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert got["n"] == int(n) and got["n_deferred"] == 0 and (got["deferred_event"] == -1).all()
    assert got["event"].tobytes() == ev.cpu().numpy().tobytes() and got["row"].tobytes() == row.cpu().numpy().tobytes()
    assert got["sim"].tobytes() == val.cpu().numpy().tobytes()


# ---- end to end: the store methods on small stores ---------------------------------------------------------------------------------
LENGTHS = [1, 4, 9, 17, 25, 33, 40]


def _events(seed=21):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(1024).astype(np.float32)
    mats = []
    for n in LENGTHS:                                                        # rows leaning towards the query by different amounts
        lean = rng.uniform(-0.2, 1.2, (n, 1)).astype(np.float32)
        mats.append((rng.standard_normal((n, 1024)) + lean * q * 0.6).astype(np.float32))
    return mats, q


def _hits_equal(got, want):
    (g_hits, g_def), (w_hits, w_def) = got, want
    assert [(e, r) for e, r, _ in g_hits] == [(e, r) for e, r, _ in w_hits]
    assert np.array([s for _, _, s in g_hits], np.float32).tobytes() == np.array([s for _, _, s in w_hits], np.float32).tobytes()
    assert [e for e, _, _ in g_def] == [e for e, _, _ in w_def]
    for (_, gi, gs), (_, wi, ws) in zip(g_def, w_def):
        assert gi.dtype == np.int64 and gs.dtype == np.float32 and gi.tolist() == wi.tolist() and gs.tobytes() == ws.tobytes()


@pytest.mark.parametrize("prefilter", [False, True])
def test_relevant_hits_is_the_model_on_top_k_per_event(prefilter):
    from hippomm_amd.vector_ops import EventStore
    mats, q = _events()
    rng = np.random.default_rng(2)
    pad_front, pad_back = rng.standard_normal((100, 1024)).astype(np.float32), rng.standard_normal((33, 1024)).astype(np.float32)
    small, large = EventStore(mats), EventStore([pad_front] + mats + [pad_back])
    limits = [max(1, n // 3) for n in LENGTHS]
    seen = {}
    for name, store, lim in (("small", small, limits), ("large", large, [0] + limits + [0])):
        per_event = store.top_k_per_event(q, 5, prefilter)
        best = sorted(float(s[0]) for _, s in per_event)
        for threshold in (0.4, best[len(best) // 2] + 1e-3):                 # the second defers about half of the flagged events
            for defer in (None, [True] * len(lim), [e % 2 == 0 for e in range(len(lim))]):
                for keep in (5, 70):
                    got = store.relevant_hits(q, 5, keep, row_limits=lim, defer=defer, min_similarity=threshold, prefilter=prefilter)
                    _hits_equal(got, model.relevant_hits(per_event, keep, lim, defer, threshold))
        seen[name] = store.relevant_hits(q, 5, 70, row_limits=lim, prefilter=prefilter)[0]
        assert store.relevant_hits(q, 5, 5) == (store.top_hits(q, 5, 5), [])   # without rules: top_hits
    # the same rows at another offset, behind an event whose hits are all dropped: the same hits, one event further on
    assert seen["large"] == [(e + 1, r, s) for e, r, s in seen["small"]] and seen["small"]


@pytest.mark.parametrize("prefilter", [False, True])
def test_relevant_hits_multi_is_the_model_on_top_k_per_event_multi(prefilter):
    from hippomm_amd.vector_ops import EventStore
    mats, q = _events()
    rng = np.random.default_rng(5)
    queries = np.concatenate([q[None], rng.standard_normal((17, 1024)).astype(np.float32) + 0.5 * q[None]])     # 18: a second pass
    store = EventStore([rng.standard_normal((50, 1024)).astype(np.float32)] + mats)
    limits = [10] + [max(1, n // 2) for n in LENGTHS]
    defer = [True, False, True, True, False, True, True, True]
    per_query = store.top_k_per_event_multi(queries, 5, prefilter)
    threshold = float(np.median([s[0] for hits_q in per_query for _, s in hits_q]))
    for keep in (5, 70):
        got = store.relevant_hits_multi(queries, 5, keep, row_limits=limits, defer=defer, min_similarity=threshold, prefilter=prefilter)
        assert len(got) == len(queries)
        for qi in range(len(queries)):
            _hits_equal(got[qi], model.relevant_hits(per_query[qi], keep, limits, defer, threshold))
    assert any(d for _, d in got)                                            # the median threshold does defer events
    none = store.relevant_hits_multi(queries, 5, 5)
    assert [h for h, _ in none] == store.top_hits_multi(queries, 5, 5) and all(d == [] for _, d in none)


GOLDEN = json.loads((ROOT / "tests" / "golden" / "retrieval_segments_golden.json").read_text())


@pytest.mark.parametrize("case_id", sorted(GOLDEN["cases"]))
def test_find_relevant_segments_equal_the_reference(case_id):
    from hippomm_amd import find_relevant_audio_segments, find_relevant_video_segments
    from hippomm_amd.segmentation import SequenceSegment
    g = GOLDEN["cases"][case_id]
    events, query, _ = R.build(g["recipe"], g["modality"])
    asked = []

    def deferred(event, idx, sims):
        asked.append(event.name)
        return [(sim, [SequenceSegment(**fields)]) for sim, fields in g["deferred_entries"][event.name]]

    find = find_relevant_video_segments if g["modality"] == "vision" else find_relevant_audio_segments
    segments = find(events, torch.from_numpy(query), deferred=deferred)
    got = [{"start_time": s.start_time, "end_time": s.end_time, "frames": s.frames, "frame_times": s.frame_times,
            "audio_data": s.audio_data} for s in segments]
    assert got == g["segments"] and asked == g["asked"]
