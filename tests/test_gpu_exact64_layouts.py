"""GPU: the float64 route's own selection pipeline (hippomm_amd/csrc/cosine_topk_f64.hip) under the adversarial layouts of
tests/exact64_layout_cases.py -- winners, exact ties and NaN rows planted at every slice seam, 1024-pair chunk seam, k boundary
and group cap, on stores whose exact similarities come in closed form.

What is asserted, and with what: for an fp32-VALUED HOST query (fp32, or the same values as fp64) the indices are the closed
form's ranking and the similarities have the closed form's BITS (a NaN row is a NaN on both sides: 0 / 0 has no agreed payload).
TOL = 2^-42 of exact64_cases applies in two places only -- a genuine-double query, whose products round, and a device query,
whose norm the kernel forms itself (compared with ``exact_query_norm``) -- and there the order is still equal.  No other number.

The stores are scattered into zeros on the device from four per-row arrays; the three large ones (131,073 / 262,145 /
1,048,577 rows: 0.5 / 1 / 4 GiB) are built one at a time and freed before the next.  The expected order of every store is one
np.lexsort.  One branch is not reached, on purpose: the re-read arg-max with 1024 threads needs more than 4.19 M rows (16 GiB)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import arena as A  # noqa: E402
import exact64_cases as cases  # noqa: E402
import exact64_layout_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = cases.TOL
DEV = "cuda"


def _vo():
    from hippomm_amd import _lib, vector_ops
    _lib.require_gpu()
    return vector_ops


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _device_rows(st) -> torch.Tensor:
    """The (n, 1024) fp32 store on the device: the two non-zero elements of every row scattered into zeros."""
    rows = torch.zeros((st.n, L.DIM), dtype=torch.float32, device=DEV)
    i = torch.arange(st.n, device=DEV)
    rows[i, torch.from_numpy(st.c).to(DEV)] = torch.from_numpy(st.xc).to(DEV)
    rows[i, torch.from_numpy(st.d).to(DEV)] = torch.from_numpy(st.xd).to(DEV)
    return rows


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero(_bits(got)[~nan] != _bits(want)[~nan])
    assert bad.size == 0, f"{what}: {bad.size} similarities differ from the closed form, first at slot {bad[:1]}"


def _within_tol(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert got.dtype == np.float64 and np.array_equal(np.isnan(got), nan), what
    assert np.max(np.abs(got[~nan] - want[~nan]), initial=0.0) <= TOL, what


def _run_flat(fs, st, ks, label, double_query=False):
    """Every k with the three queries of the issue (and the genuine double where asked).  -> {k: (idx, bits)} of the fp32 host run."""
    q, q64 = L.query(), L.query("float64")
    out = {}
    for name, query in (("fp32 host", q), ("fp64 host", q64)):
        want = st.closed_form(query, cases.host_query_norm(query))
        order = L.rank_fast(want)
        for k in ks:
            what = f"{label} k={k} {name} query"
            idx, sims = fs.search(query, k, exact64=True)
            top = order[:min(k, st.n)]
            assert idx.dtype == np.int64 and idx.tolist() == top.tolist(), what
            _same_bits(sims, want[top], what)
            if name == "fp32 host":
                out[k] = (idx, _bits(sims))
    tolerant = [("fp32 device", torch.from_numpy(q).to(DEV), q, cases.exact_query_norm(q))]
    if double_query:
        qd = L.query("double")
        tolerant.append(("genuine double host", qd, qd, cases.host_query_norm(qd)))
        tolerant.append(("genuine double device", torch.from_numpy(qd).to(DEV), qd, cases.exact_query_norm(qd)))
    for name, query, host, norm in tolerant:
        want = st.closed_form(host, norm)
        order = L.rank_fast(want)
        for k in ks:
            what = f"{label} k={k} {name} query"
            idx, sims = fs.search_device(query, k, exact64=True)
            top = order[:min(k, st.n)]
            assert idx.cpu().numpy().tolist() == top.tolist(), what
            _within_tol(sims.cpu().numpy(), want[top], what)
    return out


# ---- flat -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in L.FLAT if not c.large], ids=lambda c: c.id)
def test_flat_layouts(case):
    vo = _vo()
    st = case.store()
    fs = vo.FeatureStore(_device_rows(st))
    assert fs.f64_exact is None                                    # a device fp32 tensor: exact64=True is taken
    got = _run_flat(fs, st, case.ks, case.id, case.double_query)
    ks = sorted(case.ks)
    for a, b in zip(ks[:-1], ks[1:]):                              # every shorter list is a prefix of every longer one, the same bits
        n_a = len(got[a][0])
        assert got[b][0][:n_a].tolist() == got[a][0].tolist() and np.array_equal(got[b][1][:n_a], got[a][1]), (case.id, a, b)


@pytest.mark.parametrize("case", [c for c in L.FLAT if c.large], ids=lambda c: c.id)
def test_flat_layouts_at_the_group_caps(case):
    """One store at a time: built, run and freed (``del`` and ``empty_cache``) before the next is built."""
    vo = _vo()
    st = case.store()
    rows = fs = None
    try:
        rows = _device_rows(st)
        fs = vo.FeatureStore(rows)
        got = _run_flat(fs, st, case.ks, case.id)
        a, b = sorted(case.ks)[:2]                                 # the same answer wherever two plans overlap
        assert got[b][0][:a].tolist() == got[a][0].tolist() and np.array_equal(got[b][1][:a], got[a][1])
    finally:
        del rows, fs
        case.forget()
        torch.cuda.empty_cache()


# ---- order ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,ks", L.order_cases(), ids=lambda v: str(v).replace(" ", "_"))
def test_order_layouts(kind, n, ks):
    vo = _vo()
    st = L.get_order_store(kind, n, ks)
    fs = vo.FeatureStore(_device_rows(st))
    got = _run_flat(fs, st, ks, f"{kind} n={n}")
    if kind == "identical":
        for k in ks:
            assert got[k][0].tolist() == list(range(n - 1, n - 1 - min(k, n), -1)) and len(set(got[k][1].tolist())) == 1
    if kind == "zeros":
        for k in ks:
            assert got[k][0][0] == n // 2 + 1 and (got[k][1][1:min(k, n - 1)] == 0).all()       # +eps, then +0.0 bits


# ---- segmented --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def segmented():
    vo = _vo()
    st = L.segmented_store()
    return vo, st, vo.FeatureStore(_device_rows(st)), st.closed_form()


@pytest.mark.parametrize("k", L.SEG_KS)
def test_segmented_equals_the_closed_form_and_the_flat_call_on_every_event(segmented, k):
    vo, st, fs, want = segmented
    q = L.query()
    for name, table in L.SEG_TABLES.items():
        offsets = torch.tensor(table, dtype=torch.int64, device=DEV)
        idx, sims, counts = (t.cpu().numpy() for t in fs.search_segments_device(q, offsets, k, exact64=True))
        E = len(table) - 1
        assert idx.shape == sims.shape == (E, k) and sims.dtype == np.float64 and counts.dtype == np.int32
        for e, (lo, hi) in enumerate(zip(table[:-1], table[1:])):
            what = f"table {name} event {e} rows [{lo}, {hi}) k={k}"
            n_e = hi - lo
            assert counts[e] == min(k, n_e), what
            assert (idx[e, counts[e]:] == -1).all() and (_bits(sims[e, counts[e]:]) == 0).all(), what       # padding: -1 / 0 bits
            if n_e == 0:
                continue
            top = L.rank_fast(want[lo:hi])[:k]
            assert idx[e, :counts[e]].tolist() == top.tolist(), what
            _same_bits(sims[e, :counts[e]], want[lo:hi][top], what)
            i_f, v_f = vo.FeatureStore(fs.rows[lo:hi]).search(q, k, exact64=True)                          # the flat call on its rows
            assert i_f.tolist() == idx[e, :counts[e]].tolist(), what
            nan = np.isnan(v_f)
            assert np.array_equal(_bits(v_f)[~nan], _bits(sims[e, :counts[e]])[~nan]), what
        # the fp64 host query holds the same values (bits again); a device query forms its own norm (TOL, the order equal)
        q64 = L.query("float64")
        want64 = st.closed_form(q64, cases.host_query_norm(q64))
        want_dev = st.closed_form(q, cases.exact_query_norm(q))
        i64, s64, c64 = (t.cpu().numpy() for t in fs.search_segments_device(q64, offsets, k, exact64=True))
        i_d, s_d, c_d = (t.cpu().numpy() for t in fs.search_segments_device(torch.from_numpy(q).to(DEV), offsets, k, exact64=True))
        assert np.array_equal(i64, idx) and np.array_equal(i_d, idx) and np.array_equal(c64, counts) and np.array_equal(c_d, counts)
        for e, (lo, hi) in enumerate(zip(table[:-1], table[1:])):
            _same_bits(s64[e, :counts[e]], want64[lo:hi][idx[e, :counts[e]]], f"table {name} event {e} k={k} fp64 host query")
            _within_tol(s_d[e, :counts[e]], want_dev[lo:hi][idx[e, :counts[e]]], f"table {name} event {e} k={k} device query")


def _segmented_raw(lib, _lib, pattern, st_rows, n_rows, table, k, f64=True):
    """hmm_cosine_topk_segmented[_f64] through the library itself, every buffer at its exact size in a guarded, poisoned arena."""
    q = L.query()
    E = len(table) - 1
    size = lib.hmm_cosine_topk_segmented_f64_workspace_bytes if f64 else lib.hmm_cosine_topk_segmented_workspace_bytes
    ws_bytes = size(n_rows, E, k)
    cell = 8 if f64 else 4
    sizes = [max(n_rows, 1) * 4096, 4096, 8, 8 * (E + 1), 8 * E * k, cell * E * k, 4 * E, ws_bytes]
    ar = A.GuardedArena(A.needed_bytes(sizes), DEV, A.PATTERNS[pattern])
    s_v = ar.put(st_rows[:max(n_rows, 1)], "store")
    q_v = ar.put(torch.from_numpy(q).to(DEV), "query")
    norm_v = ar.put(torch.tensor([cases.host_query_norm(q)], dtype=torch.float64, device=DEV), "norm")
    off_v = ar.put(torch.tensor(table, dtype=torch.int64, device=DEV), "offsets")
    idx_v, sim_v = ar.carve(8 * E * k, "idx"), ar.carve(cell * E * k, "sims")
    cnt_v, ws_v = ar.carve(4 * E, "counts"), ar.carve(ws_bytes, "workspace")
    p = ar.address
    if f64:
        rc = lib.hmm_cosine_topk_segmented_f64(p(s_v), n_rows, 1024, p(q_v), 0, p(norm_v), p(off_v), E, k, p(idx_v), p(sim_v), p(cnt_v),
                                               p(ws_v), ws_bytes, _lib.stream_ptr())
    else:
        rc = lib.hmm_cosine_topk_segmented(p(s_v), n_rows, 1024, p(q_v), p(off_v), E, k, p(idx_v), p(sim_v), p(cnt_v), p(ws_v),
                                           ws_bytes, _lib.stream_ptr())
    assert rc == 0, lib.hmm_last_error()
    torch.cuda.synchronize()
    ar.check_guards()
    return (idx_v.view(torch.int64).cpu().numpy().reshape(E, k), sim_v.view(torch.float64 if f64 else torch.float32).cpu().numpy().reshape(E, k),
            cnt_v.view(torch.int32).cpu().numpy())


@pytest.mark.parametrize("name", list(L.CLAMP_TABLES))
@pytest.mark.parametrize("k", [5, 65])
def test_segmented_clamps_a_wrong_offsets_table(segmented, name, k):
    """The kernel clamps every event into [0, n_rows] (lo first, then hi into [lo, n_rows]): a wrong table reads less, never
    elsewhere.  The fp32 call reads its table as given -- its header asks for a non-decreasing table that ends at n_rows -- so it
    is run on the CLAMPED table, where its counts must be the float64 call's."""
    from hippomm_amd import _lib
    vo, st, fs, want = segmented
    lib = _lib.load()
    table = L.CLAMP_TABLES[name]
    events = L.clamped_segments(table, st.n)
    for pattern in ("ones", "zeros"):
        idx, sims, counts = _segmented_raw(lib, _lib, pattern, fs.rows, st.n, table, k)
        for e, (lo, hi) in enumerate(events):
            what = f"{name} event {e} -> rows [{lo}, {hi}) k={k}"
            assert counts[e] == min(k, hi - lo), what
            assert (idx[e, counts[e]:] == -1).all() and (_bits(sims[e, counts[e]:]) == 0).all(), what
            top = L.rank_fast(want[lo:hi])[:k]
            assert idx[e, :counts[e]].tolist() == top.tolist(), what
            _same_bits(sims[e, :counts[e]], want[lo:hi][top], what)
    legal, kept = [0], []                                          # the clamped events as a table the fp32 call accepts
    for e, (lo, hi) in enumerate(events):
        if lo == legal[-1]:
            legal.append(hi)
            kept.append(e)
    counts32 = _segmented_raw(lib, _lib, "ones", fs.rows, st.n, legal, k, f64=False)[2]
    assert len(kept) >= 2 and counts32.tolist() == counts[kept].tolist()


@pytest.mark.parametrize("k", [5, 65])
def test_segmented_without_rows(segmented, k):
    from hippomm_amd import _lib
    fs = segmented[2]
    idx, sims, counts = _segmented_raw(_lib.load(), _lib, "ones", fs.rows, 0, [0, 0, 0], k)
    assert counts.tolist() == [0, 0] and (idx == -1).all() and (_bits(sims) == 0).all()
    idx, sims, counts = _segmented_raw(_lib.load(), _lib, "big", fs.rows, 0, [0, 5, 9], k)        # a table for rows that are not there
    assert counts.tolist() == [0, 0] and (idx == -1).all() and (_bits(sims) == 0).all()


# ---- eligibility ------------------------------------------------------------------------------------------------------------------
def _report(lib, _lib, src):
    report = torch.empty(2, dtype=torch.int64, device=DEV)
    assert lib.hmm_rows_f64_are_f32(src.data_ptr(), src.shape[0], 1024, report.data_ptr(), _lib.stream_ptr()) == 0
    return report.cpu().tolist()


def test_eligibility_report_across_workgroups():
    """8,200 rows: the grid is capped, every workgroup takes several steps.  Offenders in a high workgroup's first step, in a low
    workgroup's late step and at the very last value: {count, LOWEST offset}, whichever workgroup reports first."""
    from hippomm_amd import _lib
    vo = _vo()
    lib = _lib.load()
    at = L.eligibility_offenders()
    host = L.eligibility_source()
    src = torch.from_numpy(host).to(DEV)
    assert _report(lib, _lib, src) == [0, -1] and vo.first_not_f32(host) is None
    flat, hflat = src.view(-1), host.reshape(-1)
    for count, name in enumerate(("last", "low workgroup, late step", "high workgroup, first step"), 1):   # the lowest one last
        flat[at[name]] = 0.1
        hflat[at[name]] = 0.1
        lowest = min(at[n] for n in list(("last", "low workgroup, late step", "high workgroup, first step"))[:count])
        assert _report(lib, _lib, src) == [count, lowest] == [count, vo.first_not_f32(host)]
    fs = vo.FeatureStore(src)
    assert fs.f64_exact is False and fs._f64_first_bad == divmod(at["high workgroup, first step"], 1024)


def test_eligibility_of_special_values():
    from hippomm_amd import _lib
    vo = _vo()
    lib = _lib.load()
    host = np.tile(L.f32_specials(), (L.DIM * 24) // len(L.f32_specials()) + 1)[:L.DIM * 24].reshape(24, L.DIM).copy()
    src = torch.from_numpy(host).to(DEV)
    assert np.array_equal(src.cpu().numpy().view(np.uint64), host.view(np.uint64))
    assert _report(lib, _lib, src) == [0, -1] and vo.first_not_f32(host) is None
    for i, (name, v) in enumerate(L.not_f32_values().items()):
        offset = 1024 * (7 + i) + 517 + i
        hone = host.copy()
        hone.reshape(-1)[offset] = v
        one = torch.from_numpy(hone).to(DEV)
        assert _report(lib, _lib, one) == [1, offset] == [1, vo.first_not_f32(hone)], name
