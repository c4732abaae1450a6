"""The layouts of tests/scan_layout_cases.py, checked without a GPU: the Python restatement of the row dealing is a partition with
the inverse the finish kernels use; the constants read out of the sources satisfy the conditions the kernels state for them; every
case of the GPU tables puts its rows where its layout says -- the same workgroup, the same iterations, the same side of a
compaction; and the separation condition behind the zero-exemption assertions of tests/test_gpu_scan_layouts.py holds for the
recipe's own fp32 rows in fp64: adjacent winners more than 5e-4 apart, the lowest winner more than 5e-2 above everything else."""
import numpy as np
import pytest
import torch

import scan_layout_cases as S

C = S.source_constants()
D = S.dealings()
FOUR = ("ScanDealing", "PrefilterDealing", "MultiDealing", "ShadowMultiDealing")


def test_constants_read_from_the_sources_are_the_documented_ones():
    assert [(D[n].rows, D[n].waves) for n in FOUR] == [(2, 4), (4, 4), (16, 4), (16, 8)]
    assert [D[n].cap for n in FOUR] == [C["kNumCU"] * 3 // 2, C["kNumCU"] * 3, C["kNumCU"], C["kNumCU"]]
    assert C["g_scan_blocks"] == D["ScanDealing"].cap and C["g_prefilter_blocks"] == D["PrefilterDealing"].cap
    assert D["MultiDealing"].rows == C["kMTileRows"] == D["ShadowMultiDealing"].rows
    # the kernels' own stated conditions
    assert C["kMCap"] >= C["kListMaxK"] + D["MultiDealing"].block_rows and C["kMCap"] & (C["kMCap"] - 1) == 0
    assert C["kSCap"] >= C["kListMaxK"] + D["ShadowMultiDealing"].block_rows and C["kSCap"] & (C["kSCap"] - 1) == 0
    assert C["kListMaxK"] == 64 == C["kMMaxK"] and 64 * 64 <= C["kChunk"]
    assert C["kListMaxK"] * C["kListMaxK"] <= C["kChunk"]                        # gather_winning_lists of the shadow finish
    assert C["kPrefilterMinRows"] == C["kMPMinRows"] == 4 * C["kChunk"]
    assert [S.prefilter_list_len(k) for k in (1, 5, 16, 17, 32, 64)] == [32, 32, 32, 34, 64, 64]
    assert S.compact_every(D["ScanDealing"], 128) == 112 and S.compact_every(D["PrefilterDealing"], 64) == 60
    assert all(S.compact_every(D["ScanDealing"], k) >= 1 for k in range(1, C["kFusedK"] + 1))
    assert C["kRankQuickMax"] == 65536 and C["kFusedCap"] >= 2 * C["kFusedK"]
    # the cases above a compaction compute their n from these
    assert {c.n for c in S.exact_cases() if c.route == "fused_compact"} == {(S.compact_every(D["ScanDealing"], k) + 2) * 3072 + 3 for k in (64, 128)}
    assert {c.n for c in S.shadow_cases() if c.route == "shadow_compact"} == {62 * 12288 + 3}


@pytest.mark.parametrize("name", FOUR)
def test_rows_of_block_partitions_the_store_and_block_of_row_inverts_it(name):
    d = D[name]
    shapes = []
    for nb in (1, 7, d.cap - 1, d.cap):
        per = d.rows_per_iteration(nb)
        shapes += [(n, nb) for n in (1, d.rows - 1 or 1, per - 1, per, per + 1, 2 * per - d.rows - 1, 2 * per, 2 * per + 3)]
    for n, nb in shapes:
        seen = np.zeros(n, np.int64)
        for b in range(nb):
            rows = d.rows_of_block(b, n, nb)
            assert np.all(np.diff(rows) > 0)                                    # the order the workgroup meets them in
            assert np.all(d.block_of_row(rows, nb) == b)
            by_it = d.rows_by_iteration(b, n, nb)
            assert len(by_it) == d.iterations(n, nb) and all(len(r) <= d.block_rows for r in by_it)
            for it, r in enumerate(by_it):
                assert np.all(d.iteration_of_row(r, nb) == it)
            seen[rows] += 1
        assert np.all(seen == 1), (name, n, nb)
    for n in (1, d.block_rows, d.block_rows + 1, d.cap * d.block_rows - 1, d.cap * d.block_rows + 1, 10 ** 6):
        assert d.grid(n) == min(-(-n // d.block_rows), d.cap)


def _check_plant(p: S.Plant, name: str, d: S.Dealing, n: int, nb: int, k: int, window, c: np.ndarray, exclusive: bool):
    """The rows of one question sit where ``name`` says.  ``exclusive``: no other question took rows first, so "the first / last k
    rows" are literal."""
    kind = S.layout_kind(name)
    w_blk, w_it = d.block_of_row(p.winners, nb), d.iteration_of_row(p.winners, nb)
    if kind != "tie_block":
        assert len(p.winners) == min(k, n) and len(set(p.winners.tolist())) == len(p.winners)
        np.testing.assert_allclose(c[p.winners], S.winner_value(np.arange(len(p.winners)), k), rtol=0, atol=0)
    if len(p.decoys):
        assert S.DECOY_LO <= c[p.decoys].min() and c[p.decoys].max() <= S.DECOY_HI
    if kind.startswith("one_workgroup"):
        assert np.all(w_blk == p.block)
        its = [it for it, r in enumerate(d.rows_by_iteration(p.block, n, nb)) if len(r)]
        need = -(-k // d.block_rows)
        if kind == "one_workgroup_first_iterations" and exclusive:
            assert w_it.max() == its[need - 1]
        elif kind == "one_workgroup_last_iterations" and exclusive:
            assert w_it.min() >= its[-1] - need
        elif kind == "one_workgroup" and exclusive and k > 1:
            assert w_it.min() == its[0] and w_it.max() == its[-1]               # spread over all its iterations
    elif kind == "one_per_workgroup":
        assert w_blk.tolist() == list(range(k)) and d.block_of_row(p.decoys, nb).tolist() == [k]
    elif kind == "head" and exclusive:
        assert sorted(p.winners.tolist()) == list(range(k))
    elif kind == "tail" and exclusive:
        assert sorted(p.winners.tolist()) == list(range(n - k, n)) and n % 2 == 1 and n % d.rows != 0
    elif kind == "ascending":
        assert np.all(np.diff(c) > 0) if exclusive else np.all(np.diff(c[p.winners]) < 0)      # every row beats all rows before it
        assert np.all(np.diff(p.winners) < 0) and (not exclusive or p.winners[0] == n - 1)
    elif kind == "descending":
        assert np.all(np.diff(c) < 0) if exclusive else np.all(np.diff(c[p.winners]) < 0)
        assert np.all(np.diff(p.winners) > 0) and (not exclusive or p.winners[0] == 0)
    elif kind in ("decoys_then_winners", "winners_then_decoys"):
        assert np.all(w_blk == p.block) and np.all(d.block_of_row(p.decoys, nb) == p.block) and len(p.decoys) >= 1
        d_it = d.iteration_of_row(p.decoys, nb)
        compacts = bool(window) and d.iterations(n, nb) > window
        if kind == "decoys_then_winners":
            first_window = p.decoys[d_it < window] if compacts else p.decoys
            assert first_window.max() < p.winners.min()                         # the list is full of decoys when the winners come
            if compacts:
                assert len(first_window) == k and w_it.max() >= window          # winners on the far side of a compaction
        else:
            assert p.winners.max() < p.decoys.min()
            if compacts:
                assert w_it.max() < window and d_it.max() >= window and (d_it < window).sum() == k     # decoys before and after it
    elif kind == "nan_block":
        assert len(p.zero) == k + 3 and np.all(d.block_of_row(p.zero, nb) == p.block)
    elif kind == "tie_block":
        blk = d.block_of_row(p.ties, nb)
        assert (blk == p.block).sum() == k + 5 and len(p.ties) == k + 5 + (2 if nb > 2 else nb - 1)
        assert len(set(p.ties.tolist())) == len(p.ties)


def _separation_on_the_recipe(c: np.ndarray, rows: np.ndarray):
    """fp64 similarities (Q, len(rows)) of the recipe's fp32 rows ``rows``, built on the CPU."""
    U, v = S.basis(c.shape[0], "cpu")
    cc = torch.from_numpy(np.ascontiguousarray(c[:, rows])).float()
    built = S.recipe_rows(cc, torch.from_numpy(rows), U, v)
    return S.reference_sims(built, S.queries_of(U))


def _assert_separated(c: np.ndarray, plants, k: int, n: int, seed: int):
    """Winner and decoy rows of every question plus a sample of the background: the condition on the recipe itself."""
    special = np.concatenate([p.special() for p in plants])
    rng = np.random.default_rng(seed)
    rows = np.unique(np.concatenate([special, rng.integers(0, n, 1500), np.arange(min(n, 40)), np.arange(max(n - 40, 0), n)]))
    ref = _separation_on_the_recipe(c, rows)
    assert np.abs(ref - c[:, rows]).max() < 1e-6                                # the planted value IS the similarity
    for q, p in enumerate(plants):
        if len(p.ties) or len(p.zero):
            continue
        pos = np.searchsorted(rows, p.winners)
        win = ref[q, pos]
        rest = np.delete(ref[q], pos)
        assert np.all(np.diff(win) < -S.MIN_WINNER_GAP), (q, p.layout)
        assert len(rest) == 0 or win.min() - rest.max() > S.MIN_WINNER_MARGIN, (q, p.layout, win.min(), rest.max())
        inner, outer = S.separation(ref[q], k)
        assert inner > S.MIN_WINNER_GAP and outer > S.MIN_WINNER_MARGIN


@pytest.mark.parametrize("case", S.exact_cases() + S.shadow_cases() + S.fallback_cases(), ids=lambda c: c.id)
def test_flat_case_sits_where_its_layout_says_and_is_separated(case):
    d, nb, ce = case.geometry()
    p = case.plant()
    c = S.planted_vector(p, case.n, case.k)
    if case.route == "shadow_fallback":                                          # the shadow pass must give up: one saturated list
        pre = D["PrefilterDealing"]
        rows, vals = S.saturators(case, p)
        lowest = S.WINNER_TOP if len(p.ties) else float(S.winner_value(case.k - 1, case.k))
        assert case.n >= C["kPrefilterMinRows"] and len(rows) > S.prefilter_list_len(case.k)
        assert len(set(pre.block_of_row(rows, pre.grid(case.n)).tolist())) == 1 and not np.isin(rows, p.special()).any()
        assert lowest - C["kPrefilterEps"] < vals.min() and vals.max() < lowest - 1e-3
    assert np.abs(c).max() <= S.WINNER_TOP and p.layout == S.layout_kind(case.layout)
    _check_plant(p, case.layout, d, case.n, nb, case.k, ce, c, exclusive=True)
    if case.route in ("fused_compact", "shadow_compact"):
        assert d.iterations(case.n, nb) > ce + 1 and nb == d.cap
    if case.k <= 128:                                                           # beyond it the winners' steps are finer: those routes
        _assert_separated(c[None, :], [p], case.k, case.n, seed=case.k)         # are compared bit for bit with no condition at all


def test_every_route_has_the_three_required_layouts():
    flat = S.exact_cases() + S.shadow_cases()
    for route in {c.route for c in flat}:
        kinds = {S.layout_kind(c.layout) for c in flat if c.route == route}
        assert set(S.REQUIRED_LAYOUTS) <= kinds, (route, kinds)
    assert {c.k for c in flat if c.route == "fused_final"} == {1, 5, 32, 64}
    assert {c.k for c in flat if c.route == "shadow"} == {1, 5, 32, 64}
    for case in S.batch_cases():
        if case.geometry()[1] == case.geometry()[0].cap:
            fixed = ["ascending", "descending", "one_workgroup@last", "decoys_then_winners@last"]
            assert S.batch_layouts(case.n_questions)[:4] == fixed[:case.n_questions]
    assert S.max_flat_rows() * 4096 < 4 << 30                                   # the module's buffer


@pytest.mark.parametrize("case", S.batch_cases(), ids=lambda c: c.id)
def test_batch_case_plants_every_question_on_rows_of_its_own(case):
    d, nb = case.geometry()
    plants, c = case.plant()
    names = [p.layout for p in plants]
    assert len(plants) == case.n_questions and names[:2] == ["ascending", "descending"]
    special = np.concatenate([p.special() for p in plants])
    assert len(set(special.tolist())) == len(special)                           # a winner or a decoy of one question only
    assert (c * c).sum(0).max() < 1.0
    layouts = S.batch_layouts(case.n_questions) if nb == d.cap else ["ascending", "descending", "one_workgroup@0.6", "decoys_then_winners@0.4"]
    for q, (p, name) in enumerate(zip(plants, layouts)):
        _check_plant(p, name, d, case.n, nb, case.k, None, c[q], exclusive=q < 2)
    if case.k == C["kListMaxK"] and case.route == "multi" and nb == d.cap:
        # question 0 at k = 64: every row of every round beats the threshold, so a list of k keys takes kBlockRows more:
        # the append index reaches kMCap - 1 exactly
        assert case.k + d.block_rows == C["kMCap"] and np.all(np.diff(c[0]) > 0)
    _assert_separated(c, plants, case.k, case.n, seed=case.n_questions)


@pytest.mark.parametrize("case", S.event_cases(), ids=lambda c: c.id)
def test_event_case_plants_its_pieces_and_is_separated(case):
    sizes, k = case.sizes(), case.k
    chunk = S.event_chunk(sizes, k)
    assert chunk == (C["kChunk"] if case.large or k > 64 else C["kSmallSegChunk"])
    c, winners = case.plant()
    assert (c * c).sum(0).max() < 1.0
    offs = np.concatenate([[0], np.cumsum(sizes)])
    n_pieces = set()
    picked = []
    for e, m in enumerate(sizes):
        pieces = S.fold_pieces(m, k, chunk)
        n_pieces.add(len(pieces))
        assert sum(hi - lo for lo, hi in pieces) == m and all(hi - lo <= chunk for lo, hi in pieces)
        for q in range(case.n_questions):
            w = winners[q, e]
            mode = S.EVENT_MODES[(case.mode_shift + q) % len(S.EVENT_MODES)]
            assert len(w) <= min(k, m)
            if q == 0 and m:
                assert len(w) == min(k, m)
                if mode == "first_piece":
                    assert np.all(w < pieces[0][1])
                elif mode == "last_piece" and pieces[-1][1] - pieces[-1][0] >= k:
                    assert np.all(w >= pieces[-1][0])
                elif mode == "seam" and len(pieces) > 1 and k > 1:
                    assert w.min() < pieces[0][1] <= w.max()
                elif mode == "ascending" and m:
                    assert w[0] == m - 1 and np.all(np.diff(c[0, offs[e]:offs[e + 1]]) > 0)
                elif mode == "descending" and m:
                    assert w[0] == 0 and np.all(np.diff(c[0, offs[e]:offs[e + 1]]) < 0)
            top = np.argsort(-c[q, offs[e]:offs[e + 1]], kind="stable")[:k + 2]
            picked.append(offs[e] + top)
    if k <= 64:                                                                 # one, two and three pieces of the small shape
        assert n_pieces >= ({2} if case.large else {0, 1, 2, 3})
    rows = np.unique(np.concatenate(picked))
    ref = _separation_on_the_recipe(c, rows)
    assert np.abs(ref - c[:, rows]).max() < 1e-6
    for e in range(len(sizes)):
        inside = (rows >= offs[e]) & (rows < offs[e + 1])
        for q in range(case.n_questions):
            if inside.any():
                inner, outer = S.separation(ref[q, inside], k)
                assert min(inner, outer) > S.MIN_WINNER_GAP, (q, e, inner, outer)


@pytest.mark.parametrize("pattern", S.RANK_PATTERNS)
def test_rank_hits_cases_load_one_thread_of_the_quick_route(pattern):
    sims, counts, keep = S.rank_hits_case(pattern, 0)
    assert sims.size == C["kRankQuickMax"] and S.rank_hits_case(pattern, 1)[0].size == C["kRankQuickMax"] + 4
    best = np.argsort(-sims.reshape(-1), kind="stable")[:keep]
    threads = set((best % C["kRankThreads"]).tolist())
    assert threads == {7} if pattern != "one_per_thread" else len(threads) == keep
    # `keep` threads hold keys at or above the bound, total / 1024 keys each: the candidate window can fill, never overflow
    per_thread = sims.size // C["kRankThreads"]
    assert keep * per_thread == C["kChunk"]
    if pattern == "full_window":                                                # ... and here it all but does
        maxima = np.sort(sims.reshape(-1, C["kRankThreads"]).max(axis=0))[::-1]
        assert maxima[keep - 1] == np.float32(0.61) > maxima[keep]
        assert int((sims > maxima[keep - 1]).sum()) + 1 == (keep - 1) * per_thread + 1 == C["kChunk"] - per_thread + 1
