"""GPU: the batched float64 route (exact64=True on the ``_multi`` calls; hmm_cosine_topk_multi_f64, hmm_cosine_topk_segmented_multi_f64).

The route's property is that a (row, query) similarity has the same bits whatever the entry point, batch size, batch position, N or
k, so most of these tests compare BITS with the single-question route, which tests/test_gpu_exact64.py pins to the exact oracle of
tests/exact64_cases.py.  Where the oracle is asked directly (N <= 257 only: it is a Python loop over rows) the tolerance is
cases.TOL = 2^-42, the route's derived bound, and no other number.  Single-question results are computed once per (store, query
kind, k) and shared."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import arena as A  # noqa: E402
import exact64_cases as cases  # noqa: E402
import exact64_multi_cases as multi  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = cases.TOL
DEV = "cuda"
KINDS = ("host32", "host64", "dev32", "dev64")                   # host batches travel with numpy's norms; for device ones the kernel makes them
POOL = 33                                                         # every batch is a prefix of one pool of questions per dtype


def _vo():
    from hippomm_amd import _lib, vector_ops
    _lib.require_gpu()
    return vector_ops


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _as_kind(q, kind):
    """A host array as the batch (or single question) of `kind`: as it is, or a device tensor."""
    return _dev(q) if kind.startswith("dev") else q


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the generators' arrays are shared and read-only


def _pool(kind):
    return multi.query_batch(POOL, "float64" if kind.endswith("64") else "float32")


@functools.lru_cache(maxsize=None)
def _store(n):
    return _vo().FeatureStore(multi.store_rows(n))


def _ks(n):
    return sorted({1, 5, 64, 65, min(n, 1024)})


@functools.lru_cache(maxsize=None)
def _single(n, kind, k):
    """[(idx, sim bits)] of the single-question route for every question of the pool."""
    fs, pool = _store(n), _as_kind(_pool(kind), kind)
    out = []
    for i in range(POOL):
        idx, sims = fs.search(pool[i], k, exact64=True)
        out.append((idx.tolist(), _bits(sims).tolist()))
    return out


def _same(got, want, what):
    idx, sims = got
    assert sims.dtype == np.float64 and idx.dtype == np.int64, what
    assert idx.tolist() == want[0] and _bits(sims).tolist() == want[1], what


# ---- bits equal the single route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", multi.STORE_SIZES)
def test_every_question_has_the_single_routes_bits(n, kind):
    fs, pool = _store(n), _as_kind(_pool(kind), kind)
    for k in _ks(n):
        want = _single(n, kind, k)
        for Q in multi.BATCH_SIZES:
            got = fs.search_multi(pool[:Q], k, exact64=True)
            assert len(got) == Q
            for i in range(Q):
                _same(got[i], want[i], f"n={n} {kind} k={k} Q={Q} question {i}")
    idx, sims = fs.search_multi_device(pool[:17], 5, exact64=True)                  # the device call: tensors, the same rows
    assert idx.is_cuda and sims.dtype == torch.float64 and idx.shape == sims.shape == (17, min(5, n))
    for i in range(17):
        _same((idx[i].cpu().numpy(), sims[i].cpu().numpy()), _single(n, kind, 5)[i], f"device call n={n} {kind} question {i}")


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cases.LADDER_SEEDS)
def test_ladder_ranks_as_the_oracle_at_every_batch_position(seed):
    vo = _vo()
    store, q, order, sims, ladder = cases.ladder_case(seed)
    fs = vo.FeatureStore(store.astype(np.float64))
    assert fs.f64_exact is True
    for position in (0, 7, 15):
        idx, got = fs.search_multi(multi.batch_with(q, position, 16, seed), 12, exact64=True)[position]
        assert idx.tolist() == ladder == order[:12]
        assert np.max(np.abs(got - sims[ladder])) <= TOL


def test_a_whole_store_equals_the_oracle():
    store, q, order, sims = cases.random_case(257)
    got = _vo().FeatureStore(store).search_multi(multi.batch_with(q, 3, 5), 257, exact64=True)[3]
    assert got[0].tolist() == order and np.max(np.abs(got[1] - sims[order])) <= TOL


# ---- independence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_questions_bytes_do_not_depend_on_position_or_batch_mates(dtype):
    fs = _store(257)
    q = multi.query_batch(1, dtype, seed=99)[0]
    zero, with_nan = np.zeros_like(q), q.copy()
    with_nan[517] = np.nan
    for k in (5, 257):
        i0, v0 = fs.search(q, k, exact64=True)
        want = (i0.tolist(), _bits(v0).tolist())
        for position in range(16):                                 # every slot of a full pass
            _same(fs.search_multi(multi.batch_with(q, position, 16), k, exact64=True)[position], want, f"position {position} k={k}")
        _same(fs.search_multi(multi.batch_with(q, 16, 17), k, exact64=True)[16], want, f"the lone tail of Q = 17, k={k}")
        for mate, name in ((zero, "an all-zero mate"), (with_nan, "a mate that holds a NaN")):
            for at in (0, 1):                                      # the mate before and behind the question
                batch = multi.batch_with(q, 1 - at, 4).copy()
                batch[at] = mate
                got = fs.search_multi(batch, k, exact64=True)
                _same(got[1 - at], want, f"{name} at {at}, k={k}")
                # the mate's own answer: every similarity NaN, ranked by the NaN-first rule (higher row first), the single route's bytes
                i_m, v_m = fs.search(mate, k, exact64=True)
                assert np.isnan(got[at][1]).all() and got[at][0].tolist() == list(range(256, 256 - k, -1))
                _same(got[at], (i_m.tolist(), _bits(v_m).tolist()), f"{name}'s own answer, k={k}")


# ---- segmented --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [3, 17])
@pytest.mark.parametrize("k", [5, 70])
def test_segmented_slices_equal_the_flat_single_call(k, Q):
    vo = _vo()
    fs, off = _store(1003), multi.SEGMENT_OFFSETS
    offsets = torch.tensor(off, dtype=torch.int64, device=DEV)
    pool = _pool("host32")[:Q]
    idx, sims, counts = (t.cpu().numpy() for t in fs.search_segments_multi_device(pool, offsets, k, exact64=True))
    E = len(off) - 1
    assert idx.shape == sims.shape == (Q, E, k) and counts.shape == (Q, E)
    assert idx.dtype == np.int64 and sims.dtype == np.float64 and counts.dtype == np.int32
    events = [vo.FeatureStore(fs.rows[off[e]: off[e + 1]]) if off[e + 1] > off[e] else None for e in range(E)]
    for qi in range(Q):
        for e in range(E):
            c = min(k, off[e + 1] - off[e])
            assert counts[qi, e] == c
            assert (idx[qi, e, c:] == -1).all() and (_bits(sims[qi, e, c:]) == 0).all()           # -1 / 0.0 padding
            if c:
                i_f, v_f = events[e].search(pool[qi], k, exact64=True)
                assert idx[qi, e, :c].tolist() == i_f.tolist() and np.array_equal(_bits(sims[qi, e, :c]), _bits(v_f)), (qi, e)
    # the device batch of genuine doubles: every slice the single segmented call's
    pool64 = _dev(_pool("dev64")[:Q])
    got = [t.cpu().numpy() for t in fs.search_segments_multi_device(pool64, offsets, k, exact64=True)]
    for qi in (0, Q - 1):
        want = [t.cpu().numpy() for t in fs.search_segments_device(pool64[qi], offsets, k, exact64=True)]
        assert np.array_equal(got[0][qi], want[0]) and np.array_equal(_bits(got[1][qi]), _bits(want[1]))
        assert np.array_equal(got[2][qi], want[2])


# ---- ties, NaN and k beyond n -------------------------------------------------------------------------------------------------------
def test_ties_nan_and_k_beyond_n_per_question():
    store, copies, zero_rows = multi.ties_store()
    fs = _vo().FeatureStore(store)
    batch = multi.batch_with(cases.random_case(257)[1], 1, 3)
    n = len(store)
    for k in (1, 3, n, n + 3):
        got = fs.search_multi(batch, k, exact64=True)
        for qi in range(3):
            want = cases.exact_sims(store, batch[qi], cases.host_query_norm(batch[qi]))
            order = cases.rank(want)
            distinct = np.unique(want[~np.isnan(want)])
            assert np.min(np.diff(distinct)) >= cases.GAP, "the distinct similarities must be 8 TOL apart for the oracle to decide"
            assert order[:2] == sorted(zero_rows, reverse=True)                        # NaN first, the higher row first
            for low, high in copies:
                assert order.index(high) + 1 == order.index(low)                       # exact ties: the higher row first
            idx, sims = got[qi]
            assert idx.tolist() == order[:k] and len(idx) == min(k, n)
            assert np.isnan(sims[:min(k, 2)]).all() and np.max(np.abs(sims[2:] - want[order[2:k]]), initial=0.0) <= TOL
            if k >= n:
                for low, high in copies:
                    assert _bits(sims)[order.index(low)] == _bits(sims)[order.index(high)]


def test_the_full_sort_path_per_question():
    fs = _store(1500)
    pool = _pool("host32")[:2]
    got = fs.search_multi(pool, 1100, exact64=True)
    for qi in range(2):
        i_s, v_s = fs.search(pool[qi], 1100, exact64=True)
        assert len(i_s) == 1100
        _same(got[qi], (i_s.tolist(), _bits(v_s).tolist()), f"k = 1100 on N = 1500, question {qi}")


# ---- store level ------------------------------------------------------------------------------------------------------------------
def _same_hits(got, want):
    assert [(e, r) for e, r, _ in got] == [(e, r) for e, r, _ in want]
    assert _bits([s for _, _, s in got]).tolist() == _bits([s for _, _, s in want]).tolist()


@pytest.mark.parametrize("seed", cases.THRESHOLD_SEEDS)
def test_event_store_calls_equal_the_single_calls_per_question(seed):
    vo = _vo()
    events, q, defer, _ = cases.threshold_case(seed)
    bystanders = [multi.store_rows(4100)[100:106], multi.store_rows(4100)[200:209]]
    es = vo.EventStore([ev.astype(np.float64) for ev in events + bystanders])
    assert es.f64_exact is True
    flags = list(defer) + [False, True]
    limits = [len(ev) for ev in events] + [3, 9]
    for Q, position in ((5, 2), (17, 16)):
        batch = multi.batch_with(q, position, Q, seed)
        per_event = es.top_k_per_event_multi(batch, 5, exact64=True)
        top = es.top_hits_multi(batch, 5, 7, exact64=True)
        relevant = es.relevant_hits_multi(batch, 5, 5, row_limits=limits, defer=flags, exact64=True)
        assert len(per_event) == len(top) == len(relevant) == Q
        for qi in range(Q):
            want = es.top_k_per_event(batch[qi], 5, exact64=True)
            assert len(per_event[qi]) == len(want) == 5
            for (i_g, v_g), (i_w, v_w) in zip(per_event[qi], want):
                assert v_g.dtype == np.float64 and i_g.tolist() == i_w.tolist() and np.array_equal(_bits(v_g), _bits(v_w))
            _same_hits(top[qi], es.top_hits(batch[qi], 5, 7, exact64=True))
            hits_w, deferred_w = es.relevant_hits(batch[qi], 5, 5, row_limits=limits, defer=flags, exact64=True)
            _same_hits(relevant[qi][0], hits_w)
            assert [e for e, _, _ in relevant[qi][1]] == [e for e, _, _ in deferred_w]
            for (_, i_g, v_g), (_, i_w, v_w) in zip(relevant[qi][1], deferred_w):
                assert v_g.dtype == np.float64 and i_g.tolist() == i_w.tolist() and np.array_equal(_bits(v_g), _bits(v_w))
        hits, deferred = relevant[position]
        assert 0 in [e for e, _, _ in deferred] and 1 not in [e for e, _, _ in deferred]         # A below 0.4 as a double, its twin B above
        assert hits[0][0] == 1 and all(e != 0 for e, _, _ in hits)


def test_early_returns_give_float64():
    vo = _vo()
    batch = np.array(_pool("host32")[:3])
    empty = vo.EventStore([])
    assert empty.top_k_per_event_multi(batch, 5, exact64=True) == [[], [], []]
    assert empty.top_hits_multi(batch, 5, 5, exact64=True) == [[], [], []]
    assert empty.relevant_hits_multi(batch, 5, 5, exact64=True) == [([], []), ([], []), ([], [])]
    es = vo.EventStore([multi.store_rows(4100)[:6].astype(np.float64)])
    assert es.top_hits_multi(batch, 5, 0, exact64=True) == [[], [], []]
    rows = vo.FeatureStore(np.zeros((0, 1024), np.float32))
    idx, sims = rows.search_multi_device(batch, 5, exact64=True)
    assert idx.shape == sims.shape == (3, 0) and sims.dtype == torch.float64
    got = rows.search_multi(batch, 5, exact64=True)
    assert len(got) == 3 and got[0][1].dtype == np.float64 and got[0][1].size == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    vo = _vo()
    batch = np.array(_pool("host32")[:3])
    rows = multi.store_rows(4100)[:20]
    es = vo.EventStore([rows[:8], rows[8:]])                       # an fp32-origin store is accepted
    assert es.f64_exact is None
    assert len(es.search_multi(batch, 5, exact64=True)) == 3 and len(es.top_hits_multi(batch, 5, 5, exact64=True)) == 3
    calls = {"search_multi": lambda s, **kw: s.search_multi(batch, 5, **kw),
             "search_multi_device": lambda s, **kw: s.search_multi_device(_dev(batch), 5, **kw),
             "search_segments_multi_device": lambda s, **kw: s.search_segments_multi_device(batch, s.offsets, 5, **kw),
             "top_k_per_event_multi": lambda s, **kw: s.top_k_per_event_multi(batch, 5, **kw),
             "top_hits_multi": lambda s, **kw: s.top_hits_multi(batch, 5, 5, **kw),
             "relevant_hits_multi": lambda s, **kw: s.relevant_hits_multi(batch, 5, 5, **kw)}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="prefilter"):
            call(es, prefilter=True, exact64=True)
    dirty = rows.astype(np.float64)
    dirty[11, 77] = 1 / 3                                          # one float64 value that is no fp32 value
    bad = vo.EventStore([dirty[:8], dirty[8:]])
    assert bad.f64_exact is False
    for name, call in calls.items():
        with pytest.raises(ValueError, match=r"row 11, column 77"):
            call(bad, exact64=True)
    with pytest.raises(ValueError):
        es.search_multi(np.zeros((2, 1000), np.float32), 5, exact64=True)


# ---- the default is untouched -------------------------------------------------------------------------------------------------------
def test_without_the_keyword_the_fp32_results_are_as_before_any_exact64_call():
    """Fresh stores: the default calls first, then exact64 calls on the same stores (which use their workspace and staging buffers),
    then the default calls again -- the same fp32 bytes, also with the module switch on, which reaches only top_k_cosine_similarity."""
    vo = _vo()
    rows, batch = multi.store_rows(4100), np.array(_pool("host32")[:17])
    fs = vo.FeatureStore(rows)
    es = vo.EventStore([rows[a:b].astype(np.float64) for a, b in ((0, 500), (500, 501), (501, 1003))])

    def default_calls():
        flat = fs.search_multi(batch, 5)
        assert all(v.dtype == np.float32 for _, v in flat)
        return ([(i.tobytes(), v.tobytes()) for i, v in flat], es.top_hits_multi(batch, 5, 5),
                [[(i.tobytes(), v.tobytes()) for i, v in per] for per in es.top_k_per_event_multi(batch, 5)])

    before = default_calls()
    fs.search_multi(batch, 5, exact64=True)
    es.top_hits_multi(batch, 5, 5, exact64=True)
    es.relevant_hits_multi(batch, 5, 5, exact64=True)
    assert default_calls() == before
    vo.enable_exact64()
    try:
        assert default_calls() == before
        assert (fs.search_multi(batch, 5, exact64=False)[0][1].dtype, es.top_hits_multi(batch, 5, 5, exact64=False)) == (np.float32, before[1])
    finally:
        vo.disable_exact64()


# ---- memory contract ----------------------------------------------------------------------------------------------------------------
def _contract_run(pattern, align, shape, dtype):
    from hippomm_amd import _lib
    lib = _lib.load()
    Q, n, k, off = shape
    q64 = dtype == "float64"
    store = torch.from_numpy(multi.store_rows(4100)[:n])
    queries = _pool("host64" if q64 else "host32")[:Q]
    E = len(off) - 1 if off else 0
    ws_bytes = (lib.hmm_cosine_topk_segmented_multi_f64_workspace_bytes(n, E, Q, k) if off
                else lib.hmm_cosine_topk_multi_f64_workspace_bytes(n, Q, k))
    assert ws_bytes > 0
    cells = Q * (E * k if off else min(k, n))
    counts = Q * max(E, 1)
    norms = np.array([np.linalg.norm(row) for row in queries], dtype=np.float64)
    sizes = [store.numel() * 4, queries.nbytes, 8 * Q, 8 * (E + 1), 8 * cells, 8 * cells, 4 * counts, ws_bytes]
    ar = A.GuardedArena(A.needed_bytes(sizes), DEV, A.PATTERNS[pattern])
    s_v = ar.put(store.to(DEV), "store", align)
    q_v = ar.put(_dev(queries), "queries", align)         # exactly Q * 1024 * itemsize bytes
    assert q_v.numel() == Q * 1024 * (8 if q64 else 4)
    norm_v = ar.put(torch.from_numpy(norms).to(DEV), "norms")                  # exactly 8 Q bytes; a float64 batch lets the kernel make them
    off_v = ar.put(torch.tensor(off or [0], dtype=torch.int64, device=DEV), "offsets")
    idx_v, sim_v = ar.carve(8 * cells, "idx"), ar.carve(8 * cells, "sims")
    cnt_v = ar.carve(4 * counts, "counts")
    ws_v = ar.carve(ws_bytes, "workspace", align)
    p = ar.address
    norms_ptr = None if q64 else p(norm_v)
    if off:
        rc = lib.hmm_cosine_topk_segmented_multi_f64(p(s_v), n, 1024, p(q_v), int(q64), norms_ptr, Q, p(off_v), E, k, p(idx_v),
                                                     p(sim_v), p(cnt_v), p(ws_v), ws_bytes, _lib.stream_ptr())
    else:
        rc = lib.hmm_cosine_topk_multi_f64(p(s_v), n, 1024, p(q_v), int(q64), norms_ptr, Q, k, p(idx_v), p(sim_v), p(cnt_v),
                                           p(ws_v), ws_bytes, _lib.stream_ptr())
    assert rc == 0, lib.hmm_last_error()
    torch.cuda.synchronize()
    ar.check_guards()
    return tuple(v.cpu().numpy().tobytes() for v in (idx_v, sim_v, cnt_v))


# ---- a single query is a batch of one -----------------------------------------------------------------------------------------------
ONE_FLAT = ((1, 1), (3, 5), (4097, 64), (4097, 65), (1100, 1100))  # held arg-max, the second level across a slice seam, LDS chunks, full sort
ONE_EVENTS = [0, 0, 1, 3, 303, 1328]                              # 5 events of 0, 1, 2, 300 and 1025 rows


def _single_and_batch_of_one(n, k, dtype, handed_norm, off=None):
    """The raw single-query entry point and the batched one with Q = 1 on the same guarded inputs -> their (idx, sims, n_out) bytes."""
    from hippomm_amd import _lib
    lib = _lib.load()
    q64 = dtype == "float64"
    store = torch.from_numpy(multi.store_rows(4100)[:n])
    query = _pool("host64" if q64 else "host32")[5]
    norm = np.array([np.linalg.norm(query)], dtype=np.float64)    # in the query's dtype, widened: what a host query travels with
    E = len(off) - 1 if off else 0
    sizes_of = ((lib.hmm_cosine_topk_segmented_f64_workspace_bytes(n, E, k), lib.hmm_cosine_topk_segmented_multi_f64_workspace_bytes(n, E, 1, k))
                if off else (lib.hmm_cosine_topk_f64_workspace_bytes(n, k), lib.hmm_cosine_topk_multi_f64_workspace_bytes(n, 1, k)))
    assert sizes_of[0] == sizes_of[1] > 0
    cells, counts = (E * k, E) if off else (min(k, n), 1)
    ar = A.GuardedArena(A.needed_bytes([store.numel() * 4, query.nbytes, 8, 8 * (E + 1)] + 2 * [8 * cells, 8 * cells, 4 * counts, sizes_of[0]]),
                        DEV, A.PATTERNS["big"])
    p = ar.address
    s, q = p(ar.put(store.to(DEV), "store")), p(ar.put(_dev(query), "query"))
    norm_ptr = p(ar.put(torch.from_numpy(norm).to(DEV), "norm")) if handed_norm else None
    off_ptr = p(ar.put(torch.tensor(off or [0], dtype=torch.int64, device=DEV), "offsets"))
    outs = []
    for batched in (False, True):
        views = [ar.carve(8 * cells, "idx"), ar.carve(8 * cells, "sims"), ar.carve(4 * counts, "n_out")]
        ws = p(ar.carve(sizes_of[0], "workspace"))
        idx, sim, cnt = (p(v) for v in views)
        Q = (1,) if batched else ()
        if off:
            call = lib.hmm_cosine_topk_segmented_multi_f64 if batched else lib.hmm_cosine_topk_segmented_f64
            rc = call(s, n, 1024, q, int(q64), norm_ptr, *Q, off_ptr, E, k, idx, sim, cnt, ws, sizes_of[0], _lib.stream_ptr())
        else:
            call = lib.hmm_cosine_topk_multi_f64 if batched else lib.hmm_cosine_topk_f64
            rc = call(s, n, 1024, q, int(q64), norm_ptr, *Q, k, idx, sim, cnt, ws, sizes_of[0], _lib.stream_ptr())
        assert rc == 0, lib.hmm_last_error()
        torch.cuda.synchronize()
        ar.check_guards()
        outs.append(tuple(v.cpu().numpy().tobytes() for v in views))
    return outs


@pytest.mark.parametrize("handed_norm", [True, False])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_single_entry_points_write_the_bytes_of_a_batch_of_one(dtype, handed_norm):
    for n, k in ONE_FLAT:
        single, batch = _single_and_batch_of_one(n, k, dtype, handed_norm)
        assert np.frombuffer(single[2], np.int32).tolist() == [min(k, n)], (n, k)
        assert single == batch, f"flat n={n} k={k}"
    sizes = np.diff(ONE_EVENTS)
    for k in (5, 65):
        single, batch = _single_and_batch_of_one(ONE_EVENTS[-1], k, dtype, handed_norm, ONE_EVENTS)
        assert np.frombuffer(single[2], np.int32).tolist() == np.minimum(sizes, k).tolist(), k
        assert single == batch, f"per event k={k}"


CONTRACT = {"flat argmax": (17, 4100, 5, None), "flat chunks": (17, 4100, 70, None), "flat below one block": (2, 3, 5, None),
            "segmented": (17, 1003, 5, multi.SEGMENT_OFFSETS), "segmented chunks": (17, 1003, 70, multi.SEGMENT_OFFSETS)}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", list(CONTRACT))
def test_memory_contract(name, dtype):
    """Every buffer carved at its exact size from a poisoned, guarded arena -- the queries exactly Q x 1024 values and the norms
    exactly Q doubles, so a pass that loads 16 query slots whatever Q is reads poison --, the workspace exactly what
    *_workspace_bytes answers, at 256- and at 16-byte alignment: guards untouched, and the same output bytes whatever the buffers
    held before.  Those bytes are the Python route's."""
    vo = _vo()
    Q, n, k, off = CONTRACT[name]
    outs = [_contract_run(pattern, align, CONTRACT[name], dtype) for pattern in A.PATTERNS for align in (256, 16)]
    assert all(o == outs[0] for o in outs[1:])
    fs = _store(n)
    batch = _as_kind(_pool("host64" if dtype == "float64" else "host32")[:Q], "dev64" if dtype == "float64" else "host32")
    if off:
        offsets = torch.tensor(off, dtype=torch.int64, device=DEV)
        want = [t.cpu().numpy() for t in fs.search_segments_multi_device(batch, offsets, k, exact64=True)]
    else:
        idx, sims = fs.search_multi_device(batch, k, exact64=True)
        want = [idx.cpu().numpy(), sims.cpu().numpy(), np.full(Q, min(k, n), np.int32)]
    assert outs[0] == tuple(np.ascontiguousarray(w).tobytes() for w in want)
