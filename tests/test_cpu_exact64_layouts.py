"""No GPU: every case of tests/exact64_layout_cases.py is what it claims to be.  The constants come out of the source; each case
reaches the branch it names under the plan model; the closed form equals the exact oracle of tests/exact64_cases.py in every bit
on a sample of every store; the selection model agrees with ``exact64_cases.rank``; and every named mutant of the model changes
the answer of a named case (a mutant that no case catches is a hole in the table)."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import exact64_cases as cases  # noqa: E402
import exact64_layout_cases as L  # noqa: E402

SMALL = 8200                                                       # up to here the expected order is exact64_cases.rank itself


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _order(sims):
    """The expected order: exact64_cases.rank where it is affordable (and there rank_fast must agree), rank_fast beyond."""
    fast = L.rank_fast(sims)
    if len(sims) <= SMALL:
        assert fast.tolist() == cases.rank(sims)
    return fast


def _all_stores():
    for case in L.FLAT:
        yield case.id, case.store(), case.ks
    for kind, n, ks in L.order_cases():
        yield f"{kind}-n{n}-k{ks}", L.get_order_store(kind, n, ks), ks
    yield "segmented", L.segmented_store(), L.SEG_KS


# ---- the source ---------------------------------------------------------------------------------------------------------------------
def test_constants_come_from_the_source():
    c = L.source_constants()
    text = (L.CSRC / L.SOURCE).read_text()
    for name in ("kF64ArgmaxK", "kF64MaxK", "kF64Slice", "kF64MaxGroups", "kF64MaxGroupsSort", "kF64Held"):
        assert f"constexpr int {name} = {c[name]};" in text
    assert c["kF64ArgmaxK"] < c["kF64MaxK"] == c["lds_chunk"] and c["kF64MaxGroupsSort"] < c["kF64MaxGroups"]
    assert L.argmax_threads(c["argmax_small"] * c["kF64Held"]) == c["argmax_small"]
    assert L.argmax_threads(c["argmax_small"] * c["kF64Held"] + 1) == c["argmax_large"]
    assert L.scan_grid(1) == 1 and L.scan_grid(8) == 1 and L.scan_grid(9) == 2 and L.scan_grid(1 << 20) == c["scan_cap"]
    # no second level outgrows the registers of its arg-max workgroup, and the one unreached branch needs what the docstring says
    assert c["kF64MaxGroups"] * c["kF64ArgmaxK"] <= c["kF64Held"] * c["argmax_large"]
    first_reread_1024 = c["kF64MaxGroups"] * c["kF64Held"] * c["argmax_large"] + 1
    p = L.flat_plan(first_reread_1024, 5)
    assert (p.threads1, p.held1) == (1024, False) and L.flat_plan(first_reread_1024 - 1, 5).held1
    assert first_reread_1024 * 4096 > 16 * 2 ** 30 and "16 GiB" in L.__doc__


# ---- branches -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.FLAT, ids=lambda c: c.id)
def test_every_flat_case_reaches_its_branch(case):
    for k in case.ks:
        p = L.flat_plan(case.n, k)
        for name, value in case.reaches[k].items():
            assert getattr(p, name) == value, f"{case.id} k={k}: {name} is {getattr(p, name)}, the case claims {value}"


def _top(case, k):
    sims = case.store().closed_form()
    return L.rank_fast(sims)[:min(k, case.n)], L.flat_plan(case.n, k)


def _slice_of(p, rows):
    return np.minimum(np.asarray(rows) // p.per, p.groups - 1)


def _case(name, n):
    return next(c for c in L.FLAT if c.name == name and c.n == n)


def test_one_group_has_its_winners_in_the_last_register_slot_and_at_both_ends():
    c = L.source_constants()
    top, p = _top(_case("one group", 4096), 64)
    assert top[:2].tolist() == [4095, 0] and p.held1
    assert (top // p.threads1 == c["kF64Held"] - 1).sum() >= 62 and top[2:].min() >= 3840


@pytest.mark.parametrize("n", [4097, 8192, 8193])
def test_seam_layouts_put_their_winners_where_they_say(n):
    for k in L.KS4:
        top, p = _top(_case("straddle", n), k)
        near = top[:min(k, 64)]
        assert set(_slice_of(p, near[:4]).tolist()) >= {0, 1} and (p.groups == 2 or set(_slice_of(p, near[:8]).tolist()) == {0, 1, 2})
        assert all(min(abs(r - s) for s in L.seams(n, [k])) <= 40 for r in near.tolist())
        top, p = _top(_case("last slice", n), k)
        assert (_slice_of(p, top) == p.groups - 1).all() and top[0] == n - 1
        top, p = _top(_case("first slice", n), k)
        assert (_slice_of(p, top) == 0).all() and top[0] == 0


def test_chunk_seam_layout():
    case = _case("chunk seams", 4097)
    top, p = _top(case, 65)
    assert p.per % 1024 == 1                                       # the slice's last chunk holds one row only
    offsets = {(int(r) - lo) for lo, hi in p.slices() for r in top if lo <= r < hi}
    assert offsets >= {1022, 1023, 1024, 1025, 2047} and 2048 in {int(r) for r in top}
    tie = case.store().tie
    assert tie[1022] == tie[1025] >= 0 and tie[2049 + 1022] == tie[2049 + 1025] >= 0


def test_k_boundary_and_full_sort_stores_hold_nan_rows_and_ties():
    for case in [_case("k boundaries", 4097)] + [c for c in L.FLAT if c.name == "full sort"]:
        st = case.store()
        top, p = _top(case, max(case.ks))
        assert len(st.nan_rows()) == 5 and top[:5].tolist() == sorted(st.nan_rows().tolist(), reverse=True)
        assert (st.tie >= 0).sum() >= 18
        if p.k_eff == case.n:                                       # the tail of a whole-store list is negative: below a pad read as 0.0
            assert (st.closed_form()[top[-300:]] < 0).all()
    assert L.flat_plan(2048, 1025).n_pad == 2048 and L.flat_plan(2049, 1025).n_pad == 2 * 2049 - 2
    assert L.flat_plan(1025, 1025).n_pad - 1025 == 1023


def test_large_layouts():
    case = _case("sort-path cap", 32 * 4096 + 1)
    for k in case.ks:
        top, p = _top(case, k)
        head = top[:64].tolist()
        assert head[:2] == [case.n - 1, case.n - 2] and _slice_of(p, head[:2]).tolist() == [p.groups - 1] * 2
        at = [lo for lo, _ in p.slices()[1:]]
        assert sum(1 for r in head if r in at or r + 1 in at) >= 16     # rows on both sides of this plan's own seams
    case = _case("1024-thread second level", 64 * 4096 + 1)
    top, p = _top(case, 64)
    slot = lambda r: (int(_slice_of(p, [r])[0]) * p.k_eff) // p.threads2
    assert p.threads2 == 1024 and [slot(r) for r in top[:17]] == [4] + [0] * 16
    assert len(set(_slice_of(p, top).tolist())) == 64              # one winner per group
    assert L.flat_plan(case.n, 63).threads2 == 256
    case = _case("arg-max cap", 256 * 4096 + 1)
    top, p = _top(case, 64)
    c = L.source_constants()
    assert p.cand == c["kF64Held"] * p.threads2 == 16384 and _slice_of(p, top[:1])[0] == p.groups - 1
    offs = [int(r) - p.slices()[int(g)][0] for r, g in zip(top, _slice_of(p, top))]
    assert {o // p.threads1 for o in offs} == {0, 1, 2, 3, 4}      # every register slot a slice of 4097 rows fills
    assert case.n * 4096 == 4 * 2 ** 30 + 4096


# ---- the closed form ------------------------------------------------------------------------------------------------------------------
def test_closed_form_equals_the_exact_oracle_in_every_bit():
    q, seen = L.query(), 0
    A = cases.host_query_norm(q)
    for label, st, _ in _all_stores():
        rng = np.random.default_rng(len(label) + st.n)
        special = np.flatnonzero((st.tie >= 0) | (st.xc == 0))[:6]
        rows = np.unique(np.concatenate([special, L.rank_fast(st.closed_form())[:6], rng.integers(0, st.n, 30), [0, st.n - 1]]))
        want = cases.exact_sims(st.dense(rows), q, A)
        got = st.closed_form()[rows]
        assert np.array_equal(_bits(got), _bits(want)), label
        seen += len(rows)
    assert seen >= 1500
    # the fp64 host query holds the same values: the same products, numpy's float64 norm
    st = L.FLAT[1].store()
    q64 = L.query("float64")
    rows = np.arange(0, st.n, 97)
    assert np.array_equal(_bits(st.closed_form(q64)[rows]), _bits(cases.exact_sims(st.dense(rows), q64, cases.host_query_norm(q64))))
    # a genuine double: the products round, the closed form stays within TOL of the oracle
    qd = L.query("double")
    assert np.max(np.abs(st.closed_form(qd)[rows] - cases.exact_sims(st.dense(rows), qd, cases.host_query_norm(qd)))) <= L.TOL / 64


def test_stores_meet_the_generators_conditions_and_cover_every_column():
    for label, st, _ in _all_stores():
        st.check()
        cols = set(st.c.tolist()) | set(st.d[(st.xd != 0)].tolist())
        if st.background and st.n >= 4096:                        # (a smaller store loses a column to a planted row)
            assert len(cols) == 1024, label
        elif not st.background:                                     # tied rows cannot use the query's zero columns (zeros: only those)
            assert len(cols) in (1020, 12), (label, len(cols))
        sims = st.closed_form()
        assert np.nanmax(np.abs(sims)) < 0.4


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_model_agrees_with_rank_on_every_case():
    for label, st, ks in _all_stores():
        if label == "segmented":
            continue
        sims = st.closed_form()
        order = _order(sims)
        for k in ks:
            assert L.model_flat(sims, k).tolist() == order[:min(k, st.n)].tolist(), (label, k)
    sims = L.segmented_store().closed_form()
    for table in L.SEG_TABLES.values():
        for lo, hi in zip(table[:-1], table[1:]):
            for k in L.SEG_KS:
                assert L.model_segment(sims[lo:hi], k).tolist() == cases.rank(sims[lo:hi])[:k]


# mutant -> the case that catches it: (flat case name, n, k) | ("order", kind, n, k) | ("plan", flat case name, n, k)
CAUGHT_BY = {
    "tie rule reversed in the second level": ("order", "ties for first", 4097, 5),
    "tie rule reversed between LDS chunks": ("order", "identical", 4097, 1024),
    "first level keeps k - 1": ("last slice", 4097, 64),
    "per by floor": ("last slice", 4097, 5),
    "register slot kF64Held - 1 not loaded": ("one group", 4096, 64),
    "chunk offset 1023 dropped in a merge": ("chunk seams", 4097, 65),
    "padding counted as a hit in the full sort": ("full sort", 1025, 1025),
    "NaN ranked last": ("order", "many NaN", 4097, 5),
    "arg-max dispatch limit off by one": ("plan", "sort-path cap", 32 * 4096 + 1, 65),
    "1024 limit off by one": ("k boundaries", 4097, 1025),
}
ALSO_CAUGHT_BY = {                                                 # the same mistakes on the other path or level
    "first level keeps k - 1": ("last slice", 8193, 1024),
    "register slot kF64Held - 1 not loaded": ("arg-max cap", 256 * 4096 + 1, 64),      # slot 15 of the SECOND level's 1024 threads
    "chunk offset 1023 dropped in a merge": ("chunk seams", 4097, 1024),
    "NaN ranked last": ("full sort", 2049, 1025),
    "tie rule reversed in the second level": ("order", "identical", 8193, 65),
    "per by floor": ("sort-path cap", 32 * 4096 + 1, 1024),
}


def _caught(mutant, where):
    if where[0] == "plan":                                         # the answer is the same on either path: the case's claimed branch is not
        case = _case(where[1], where[2])
        p = L.flat_plan(case.n, where[3], mutant)
        return any(getattr(p, name) != value for name, value in case.reaches[where[3]].items())
    if where[0] == "order":
        st, k = L.get_order_store(where[1], where[2], (where[3],)), where[3]
    else:
        st, k = _case(where[0], where[1]).store(), where[2]
    sims = st.closed_form()
    return L.model_flat(sims, k, mutant).tolist() != L.rank_fast(sims)[:min(k, st.n)].tolist()


def test_every_mutant_is_caught_by_a_named_case():
    assert set(CAUGHT_BY) == set(L.MUTANTS)
    for mutant in L.MUTANTS:
        assert _caught(mutant, CAUGHT_BY[mutant]), f"no longer caught: {mutant} by {CAUGHT_BY[mutant]}"
    for mutant, where in ALSO_CAUGHT_BY.items():
        assert _caught(mutant, where), f"no longer caught: {mutant} by {where}"
    # the segmented call runs the same two selections: its events catch the slot and the chunk mutants as well
    sims, table = L.segmented_store().closed_form(), L.SEG_TABLES["large"]
    ev = sims[table[1]:table[2]]                                    # 4096 rows: held, winners at its first and last row
    assert L.model_segment(ev, 64, "register slot kF64Held - 1 not loaded").tolist() != cases.rank(ev)[:64]
    assert L.model_segment(ev, 65, "chunk offset 1023 dropped in a merge").tolist() != cases.rank(ev)[:65]


# ---- order ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 8193, 2049])
def test_order_stores_have_the_answers_they_are_named_for(n):
    ks = [k for m, k in L.ORDER_SHAPES if m == n]
    order = lambda kind, k=0: L.rank_fast(L.get_order_store(kind, n, (k,) if kind in L._PER_K else tuple(ks)).closed_form()).tolist()
    assert order("identical") == list(range(n - 1, -1, -1))
    st = L.get_order_store("zeros", n, tuple(ks))
    plus, minus = n // 2 + 1, n - 1
    sims = st.closed_form()
    assert (_bits(np.delete(sims, [plus, minus])) == 0).all() and sims[plus] >= L.GAP and sims[minus] <= -L.GAP
    assert order("zeros") == [plus] + [r for r in range(n - 1, -1, -1) if r not in (plus, minus)] + [minus]
    assert order("ascending") == list(range(n - 1, -1, -1)) and order("descending") == list(range(n))
    for k in ks:
        p = L.flat_plan(n, k)
        st = L.get_order_store("ties for first", n, (k,))
        tied = np.flatnonzero(st.tie >= 0)
        assert len(tied) == k + 3 and order("ties for first", k)[:k + 3] == sorted(tied.tolist(), reverse=True)
        st = L.get_order_store("many NaN", n, (k,))
        assert len(st.nan_rows()) == k + 3 and order("many NaN", k)[:k + 3] == sorted(st.nan_rows().tolist(), reverse=True)
        if p.path != "sort":                                       # spread over every slice and every 1024-pair chunk of it
            chunks = {(int(g), (int(r) - int(g) * p.per) // 1024) for r, g in zip(tied, _slice_of(p, tied))}
            assert len(chunks) >= sum((hi - lo) // 1024 for lo, hi in p.slices()) or k + 3 < 16      # every full chunk
            assert set(_slice_of(p, tied).tolist()) == set(range(p.groups))
            assert set(_slice_of(p, st.nan_rows()).tolist()) == set(range(p.groups))
        st = L.get_order_store("NaN at seams", n, tuple(ks))
        at = L.seams(n, [k]) or [n // 2]
        assert all(s - 1 in st.nan_rows() and s in st.nan_rows() for s in at)


# ---- segmented ------------------------------------------------------------------------------------------------------------------------
def test_segmented_tables_hold_every_size_and_both_sides_of_the_held_limit():
    sizes = [hi - lo for t in L.SEG_TABLES.values() for lo, hi in zip(t[:-1], t[1:])]
    assert set(L.SEG_SIZES) <= set(sizes) and all(t[-1] == L.SEG_N and t == sorted(t) for t in L.SEG_TABLES.values())
    assert sum(L.SEG_SIZES) > L.SEG_N                               # why there are two tables
    assert all(any(lo % 2 == 1 and hi > lo for lo, hi in zip(t[:-1], t[1:])) for t in L.SEG_TABLES.values())
    assert L.segment_plan(4096, 64) == ("argmax", 256, True) and L.segment_plan(4097, 64) == ("argmax", 256, False)
    assert L.segment_plan(4097, 65) == ("lds", 1024, False) and L.segment_plan(1, 1024)[0] == "lds"
    st = L.segmented_store()
    sims = st.closed_form()
    ends = {r for t in L.SEG_TABLES.values() for lo, hi in zip(t[:-1], t[1:]) for r in (lo, hi - 1)}
    for t in L.SEG_TABLES.values():
        for lo, hi in zip(t[:-1], t[1:]):
            if hi - lo >= 2:
                top = set(cases.rank(sims[lo:hi])[:40])
                assert {0, hi - lo - 1} <= top or np.isnan(sims[lo:hi]).any()            # winners at the first and the last row
            for seam in range(lo + 1024, hi, 1024):
                assert st.tie[seam - 1] == st.tie[seam] >= 0 or {seam - 1, seam} & ends      # (an end row is a winner already)


def test_clamping_rule():
    n = L.SEG_N
    assert L.clamped_segments(L.CLAMP_TABLES["negative first offset"], n) == [(0, 10), (10, 20)]
    assert L.clamped_segments(L.CLAMP_TABLES["offset beyond n_rows"], n) == [(0, 100), (100, n)]
    assert L.clamped_segments(L.CLAMP_TABLES["descending pair"], n) == [(0, 500), (500, 500), (300, 800)]
    assert L.clamped_segments([0, 5, 9], 0) == [(0, 0), (0, 0)]


# ---- eligibility ----------------------------------------------------------------------------------------------------------------------
def test_eligibility_inputs_and_the_host_rule():
    from hippomm_amd.vector_ops import first_not_f32
    c = L.source_constants()
    n_values = L.ELIG_ROWS * L.DIM
    grid = L.eligibility_grid(n_values)
    per_block = c["elig_threads"] * c["elig_per_thread"]
    assert grid == c["kScanBlocks"] and (8193 * L.DIM + per_block - 1) // per_block > grid == 8192 * L.DIM // per_block   # binds from 8193 rows
    at = L.eligibility_offenders()
    block = lambda o: (o // c["elig_threads"]) % grid
    step = lambda o: o // (grid * c["elig_threads"])
    assert at["last"] == n_values - 1
    assert (block(at["high workgroup, first step"]), step(at["high workgroup, first step"])) == (grid - 1, 0)
    assert block(at["low workgroup, late step"]) == 0 and step(at["low workgroup, late step"]) >= 15
    assert at["high workgroup, first step"] < at["low workgroup, late step"] < at["last"]
    src = L.eligibility_source()
    assert first_not_f32(src) is None
    flat = src.reshape(-1)
    for o in at.values():
        flat[o] = 0.1
    assert first_not_f32(src) == at["high workgroup, first step"]
    flat[at["high workgroup, first step"]] = 0.5
    assert first_not_f32(src) == at["low workgroup, late step"]
    special = np.tile(L.f32_specials(), 103)[:1024][None, :]
    assert first_not_f32(special) is None and cases.is_f32_valued(special)
    for name, v in L.not_f32_values().items():
        one = special.copy()
        one[0, 517] = v
        assert first_not_f32(one) == 517, name
    x = 0.7314
    assert float(np.float32(x)) + 2.0 ** -60 * x == float(np.float32(x))     # why not_f32_values takes the next double instead


def test_branch_table_prints():
    """The branch table of the summary, as the plan model prints it (pytest -s shows it)."""
    for case in L.FLAT:
        for k in case.ks:
            print(f"{case.id:40s} k={k:<5d} {L.flat_plan(case.n, k).branch()}")
