"""The selection layer of the retrieval kernels (topk_select.h and the routes built on it) under adversarial row layouts.

Every other scan test feeds standard-normal rows: the winners scatter uniformly over the workgroups, the thresholds settle after the
first round and no candidate list comes near its capacity.  Here the similarities are PLANTED (tests/scan_layout_cases.py): all
winners in one workgroup's list, in the last workgroups, on both sides of a compaction, behind a list full of decoys, in ascending
order so that every row beats the threshold, NaN rows and bit-identical rows in one workgroup -- on every route.

What is compared with what.  The exact one-question routes must return, at EVERY rank, top_k_documented_order of hmm_op_scan_sims'
values on the same store -- indices equal, similarities bit-equal (cosine_topk_shared.h: all streaming kernels produce the same
bits per row; NaN is compared as NaN) -- and hmm_op_scan_sims must lie within SIM_ATOL of the fp64 similarity of the fp32 rows,
once per store.  The batched routes compute on the MFMA and have bits of their own: their reference is the fp64 similarity, indices
equal at all k ranks (no rank is exempt: tests/test_cpu_scan_layouts.py proves the winners more than 5e-4 apart and 5e-2 above the
rest, and the condition is asserted again here on the fp64 values), similarities within SIM_ATOL.  Every shape above a compaction
or dispatch boundary is computed from constants read out of the sources."""
import numpy as np
import pytest
import torch

import scan_layout_cases as S
from oracle.vector_ops_oracle import scan_order_key, top_k_documented_order

pytestmark = pytest.mark.gpu

C = S.source_constants()
D = S.dealings()
SIM_ATOL = S.SIM_ATOL


@pytest.fixture(scope="module")
def buffer():
    """The one store buffer of the module, refilled per layout (3.1 GB: the store above the shadow route's compaction)."""
    buf = torch.empty(S.max_flat_rows(), 1024, dtype=torch.float32, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def bases():
    made = {}

    def get(n_questions):
        if n_questions not in made:
            U, v = S.basis(n_questions, "cuda")
            made[n_questions] = (U, v, S.queries_of(U))
        return made[n_questions]
    return get


def kernel_sims(rows, q) -> np.ndarray:
    from hippomm_amd import _lib as L
    sims = torch.full((rows.shape[0],), -7.0, device="cuda")
    L.check(L.load().hmm_op_scan_sims(rows.data_ptr(), rows.shape[0], q.data_ptr(), sims.data_ptr(), L.stream_ptr()), "hmm_op_scan_sims")
    return sims.cpu().numpy()


def canonical_bits(x) -> np.ndarray:
    x = np.array(x, dtype=np.float32)
    x[np.isnan(x)] = np.float32("nan")                                  # the keys carry one NaN
    return x.view(np.int32)


def single_store(buffer, bases, n, c, zero=(), ties=()):
    """(rows, query, hmm_op_scan_sims' values) of a one-question store; the values are checked against the fp64 reference here."""
    U, v, queries = bases(1)
    rows = S.fill_rows(buffer[:n], c[None, :], U, v, zero=zero, ties=ties)
    sk = kernel_sims(rows, queries[0])
    ref = S.reference_sims(rows, queries)[0]
    assert np.array_equal(np.isnan(sk), np.isnan(ref)) and int(np.isnan(ref).sum()) == len(zero)
    err = float(np.nanmax(np.abs(sk.astype(np.float64) - ref)))
    print(f"hmm_op_scan_sims vs fp64: max |err| = {err:.3g} over {n} rows")
    assert err <= SIM_ATOL
    return rows, queries[0], sk


def assert_documented_order(idx, sims, sk, k):
    """The route's answer is the documented order of the kernel's own similarities: every rank, every bit."""
    want_idx, want_sims = top_k_documented_order(sk, k)
    idx, sims = idx.cpu().numpy(), sims.cpu().numpy()
    assert idx.dtype == np.int64 and idx.tolist() == want_idx.tolist()
    assert canonical_bits(sims).tolist() == canonical_bits(want_sims).tolist()
    return want_idx


def assert_planted_answer(want_idx, p: S.Plant, k):
    """... and that order is the planted one: the expectation does not rest on the kernels alone."""
    if len(p.zero):
        assert want_idx.tolist() == np.sort(p.zero)[::-1][:k].tolist()
    elif len(p.ties):
        assert want_idx.tolist() == np.sort(p.ties)[::-1][:k].tolist()
    else:
        assert want_idx.tolist() == p.winners[:k].tolist()


# ---- (a) the dealing restatement is the kernel's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ascending", "decoys_then_winners@mid"])
@pytest.mark.parametrize("n", [S.rows_for(D["ScanDealing"], 5), 1003], ids=["full_grid", "grid_below_cap"])
def test_block_lists_are_the_best_keys_of_the_rows_the_restatement_deals(buffer, bases, layout, n):
    from hippomm_amd import _lib as L
    d = D["ScanDealing"]
    nb = d.grid(n)
    assert (nb == d.cap) == (n > 1003)
    p = S.make_plant(layout, d, n, nb, 4)
    rows, q, sk = single_store(buffer, bases, n, S.planted_vector(p, n, 4))
    keys = scan_order_key(sk)
    for k in (1, 8, C["kFusedK"]):
        cand = torch.zeros(2048 * k, dtype=torch.int64, device="cuda")
        L.check(L.load().hmm_op_scan_topk_only(rows.data_ptr(), n, q.data_ptr(), k, cand.data_ptr(), L.stream_ptr()), "hmm_op_scan_topk_only")
        lists = cand.cpu().numpy().view(np.uint64)[:nb * k].reshape(nb, k)
        named = lists[lists != 0] & np.uint64(0xFFFFFFFF)
        assert np.array_equal(d.block_of_row(named.astype(np.int64), nb), np.nonzero(lists)[0])
        for b in range(nb):
            want = np.zeros(k, np.uint64)
            best = np.sort(keys[d.rows_of_block(b, n, nb)])[::-1][:k]
            want[:len(best)] = best
            assert np.array_equal(lists[b], want), (k, b)


# ---- (b) exact single-question routes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.exact_cases(), ids=lambda c: c.id)
def test_exact_routes_return_the_documented_order_bit_for_bit(buffer, bases, case):
    from hippomm_amd.vector_ops import FeatureStore
    p = case.plant()
    rows, q, sk = single_store(buffer, bases, case.n, S.planted_vector(p, case.n, case.k), p.zero, p.ties)
    # the route the case is named after is the one hmm_cosine_topk takes at this shape (run_scan)
    full_sort = case.n > C["kChunk"] and min(case.k, case.n) > C["kFastK"]
    fused = not full_sort and case.n > C["kChunk"] and case.k <= C["kFusedK"]
    one_kernel = fused and case.k * case.k <= C["kChunk"]
    assert {"chunk": not fused and not full_sort and case.n <= C["kChunk"], "fused_final": one_kernel, "fused_chunks": fused and not one_kernel,
            "fused_compact": fused and D["ScanDealing"].iterations(case.n, D["ScanDealing"].cap) > S.compact_every(D["ScanDealing"], case.k),
            "sims_buffer": not fused and not full_sort and case.n > C["kChunk"], "full_sort": full_sort}[case.route]
    idx, sims = FeatureStore(rows).search_device(q, case.k)
    want_idx = assert_documented_order(idx, sims, sk, case.k)
    assert_planted_answer(want_idx, p, case.k)


@pytest.mark.parametrize("where", ["one_shard", "one_per_shard"])
def test_shard_keys_and_their_merge_return_the_documented_order(buffer, bases, where):
    """hmm_cosine_topk_keys on three ragged shards (sims-and-chunk route, fused route, a shard of k + 1 rows) and hmm_topk_merge_keys."""
    from hippomm_amd.vector_ops import FeatureStore, merge_keys_device
    k = 32
    bounds = [0, C["kChunk"] - 95, C["kChunk"] - 95 + k + 1, 3 * C["kChunk"] + 7]
    n = bounds[-1]
    rng = np.random.default_rng(3)
    if where == "one_shard":
        winners = rng.permutation(np.arange(bounds[2], n))[:k]
    else:
        winners = np.array([bounds[j % 3] + (97 * j) % (bounds[j % 3 + 1] - bounds[j % 3]) for j in range(k)])
    assert len(set(winners.tolist())) == k
    p = S.Plant(where, winners=winners.astype(np.int64))
    rows, q, sk = single_store(buffer, bases, n, S.planted_vector(p, n, k))
    keys = torch.stack([FeatureStore(rows[a:b]).search_keys_device(q, k) for a, b in zip(bounds[:-1], bounds[1:])])
    idx, sims = merge_keys_device(keys, torch.tensor(bounds[:-1], dtype=torch.int64, device="cuda"), k)
    assert_planted_answer(assert_documented_order(idx, sims, sk, k), p, k)


# ---- (c) the shadow route and its conditional exact scan ---------------------------------------------------------------------------
def _in_one_workgroup(case):
    """Rows of the layout that one workgroup of the shadow pass holds above the threshold."""
    kind = S.layout_kind(case.layout)
    if kind in ("tie_block", "nan_block"):
        return case.k + (5 if kind == "tie_block" else 3)
    return case.k if kind.startswith("one_workgroup") or kind in ("decoys_then_winners", "winners_then_decoys") else 1


@pytest.mark.parametrize("case", S.shadow_cases() + S.fallback_cases(), ids=lambda c: c.id)
def test_shadow_route_returns_the_documented_order_bit_for_bit(buffer, bases, case):
    from hippomm_amd.vector_ops import FeatureStore
    assert case.n >= C["kPrefilterMinRows"] and case.k <= C["kListMaxK"]
    p = case.plant()
    c = S.planted_vector(p, case.n, case.k)
    if case.route == "shadow_fallback":
        sat_rows, sat_values = S.saturators(case, p)
        c[sat_rows] = sat_values
        expect_fallback = True
    else:
        expect_fallback = _in_one_workgroup(case) >= case.list_len            # a list full of rows above the threshold: saturated
    rows, q, sk = single_store(buffer, bases, case.n, c, p.zero, p.ties)
    stats = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    idx, sims = FeatureStore(rows).search_prefiltered_device(q, case.k, stats)
    want_idx = assert_documented_order(idx, sims, sk, case.k)
    assert_planted_answer(want_idx, p, case.k)
    candidates, saturated = stats.cpu().tolist()
    print(f"stats: {candidates} candidates, {saturated} saturated lists")
    if expect_fallback:                                                       # exact_scan_fallback_kernel answered
        assert saturated > 0 or candidates > C["kCandCap"], (candidates, saturated)
    else:                                                                     # the shadow pass and its re-score answered
        assert saturated == 0 and case.k <= candidates <= C["kCandCap"], (candidates, saturated)


# ---- (d) batched routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.batch_cases(), ids=lambda c: c.id)
def test_batched_routes_return_the_planted_winners_at_every_rank(buffer, bases, case):
    from hippomm_amd.vector_ops import FeatureStore
    Q, k, n = case.n_questions, case.k, case.n
    plants, c = case.plant()
    U, v, queries = bases(Q)
    rows = S.fill_rows(buffer[:n], c, U, v)
    ref = S.reference_sims(rows, queries)
    for qi in range(Q):                                                       # the condition, on the reference itself
        inner, outer = S.separation(ref[qi], k)
        assert inner > S.MIN_WINNER_GAP and outer > S.MIN_WINNER_MARGIN, (qi, inner, outer)
    prefilter = case.route == "multi_prefilter"
    stats = torch.full((Q, 2), -7, dtype=torch.int32, device="cuda")
    idx, sims = FeatureStore(rows).search_multi_device(queries, k, prefilter=prefilter, stats=stats if prefilter else None)
    idx, sims = idx.cpu().numpy(), sims.cpu().numpy()
    worst = 0.0
    for qi in range(Q):
        want = np.argsort(-ref[qi], kind="stable")[:k]
        assert want.tolist() == plants[qi].winners.tolist()
        assert idx[qi].tolist() == want.tolist(), (qi, plants[qi].layout)
        worst = max(worst, float(np.abs(sims[qi].astype(np.float64) - ref[qi][want]).max()))
    print(f"batched similarities vs fp64: max |err| = {worst:.3g}")
    assert worst <= SIM_ATOL
    if prefilter:
        st = stats.cpu().numpy()
        print(f"stats: {st.tolist()}")
        assert (st >= 0).all()                                                # the shadow pass ran for every question
        if k == C["kListMaxK"] and n >= 4 * D["ShadowMultiDealing"].block_rows * D["ShadowMultiDealing"].cap // 2:
            assert st[:, 1].max() > 0                                         # k winners fill one list: the exact pass answered


# ---- (e) per-event routes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.event_cases(), ids=lambda c: c.id)
def test_per_event_routes_fold_their_pieces_without_losing_a_winner(buffer, bases, case):
    from hippomm_amd.vector_ops import EventStore
    sizes, k, Q = case.sizes(), case.k, case.n_questions
    c, winners = case.plant()
    n = int(sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    prefilter = case.route.endswith("prefilter")
    U, v, queries = bases(Q)
    if Q == 1:
        rows, q, sk = single_store(buffer, bases, n, c[0])
        es = EventStore.from_device_rows(rows, sizes)
        idx, sims, counts = es.search_segments_device(q, es.offsets, k, prefilter=prefilter)
        idx, sims, counts = idx.cpu().numpy()[None], sims.cpu().numpy()[None], counts.cpu().numpy()[None]
    else:
        rows = S.fill_rows(buffer[:n], c, U, v)
        ref = S.reference_sims(rows, queries)
        es = EventStore.from_device_rows(rows, sizes)
        idx, sims, counts = (t.cpu().numpy() for t in es.search_segments_multi_device(queries, es.offsets, k, prefilter=prefilter))
    assert idx.shape == (Q, len(sizes), k) and sims.shape == idx.shape and counts.shape == (Q, len(sizes))
    for e, m in enumerate(sizes):
        lo, cnt = offs[e], min(k, m)
        for qi in range(Q):
            assert counts[qi, e] == cnt
            assert idx[qi, e, cnt:].tolist() == [-1] * (k - cnt) and sims[qi, e, cnt:].view(np.int32).tolist() == [0] * (k - cnt)
            if Q == 1:
                want, want_sims = top_k_documented_order(sk[lo:lo + m], k)
                assert idx[0, e, :cnt].tolist() == want.tolist() == winners[0, e].tolist()
                assert canonical_bits(sims[0, e, :cnt]).tolist() == canonical_bits(want_sims).tolist()
            else:
                inner, outer = S.separation(ref[qi, lo:lo + m], k) if m else (np.inf, np.inf)
                assert min(inner, outer) > S.MIN_WINNER_GAP, (qi, e, inner, outer)
                want = np.argsort(-ref[qi, lo:lo + m], kind="stable")[:k]
                assert idx[qi, e, :cnt].tolist() == want.tolist(), (qi, e)
                assert want[:len(winners[qi, e])].tolist() == winners[qi, e].tolist()
                assert np.abs(sims[qi, e, :cnt].astype(np.float64) - ref[qi, lo:lo + m][want]).max(initial=0.0) <= SIM_ATOL


# ---- (f) hmm_rank_segment_hits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_events", [0, 1], ids=["quick_route_at_its_limit", "fold_route"])
@pytest.mark.parametrize("pattern", S.RANK_PATTERNS)
def test_rank_segment_hits_with_the_best_hits_in_one_thread(pattern, extra_events):
    """Python's stable descending sort (tests/test_gpu_retrieval.py) of 65 536 hits -- the quick route's largest input, where the 64
    threads' keys at or above the bound fill the 4096-key window to its last slot -- and of 65 540, which takes the fold route."""
    from hippomm_amd import _lib as L
    sims, counts, keep = S.rank_hits_case(pattern, extra_events)
    E, k = sims.shape
    assert (E * k <= C["kRankQuickMax"]) == (extra_events == 0)
    idx_h = np.random.default_rng(1).integers(0, 10_000, (E, k))
    idx, s, cn = torch.from_numpy(idx_h).cuda(), torch.from_numpy(sims).cuda(), torch.from_numpy(counts).cuda()
    ev, row = torch.empty(keep, dtype=torch.int64, device="cuda"), torch.empty(keep, dtype=torch.int64, device="cuda")
    val, n_out = torch.empty(keep, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(L.load().hmm_rank_segment_hits(idx.data_ptr(), s.data_ptr(), cn.data_ptr(), E, k, keep, ev.data_ptr(), row.data_ptr(),
                                           val.data_ptr(), n_out.data_ptr(), None), "hmm_rank_segment_hits")
    flat = sims.reshape(-1).tolist()
    want = sorted(range(E * k), key=lambda pos: -flat[pos])[:keep]          # stable: equal similarities stay in event order
    assert int(n_out.item()) == keep
    assert ev.cpu().tolist() == [pos // k for pos in want]
    assert row.cpu().tolist() == [int(idx_h.reshape(-1)[pos]) for pos in want]
    assert val.cpu().numpy().view(np.int32).tolist() == sims.reshape(-1)[want].view(np.int32).tolist()
