"""GPU: the float64 route (exact64=True; hmm_cosine_topk_f64, hmm_cosine_topk_segmented_f64, hmm_rows_f64_are_f32) against the exact
oracle of tests/exact64_cases.py.  Indices equal the oracle's wherever its neighbours are 8 TOL apart (the generators assert that),
similarities are within TOL = 2^-42, the route's derived bound, and no other number.  The oracle's sums are computed once per
store and shared (functools caches in exact64_cases)."""
import json
import logging
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import arena as A  # noqa: E402
import exact64_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = cases.TOL
DEV = "cuda"
KS = (1, 5, 32, 64, 65)                                           # and N + 3


def _vo():
    from hippomm_amd import _lib, vector_ops
    _lib.require_gpu()
    return vector_ops


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _query(q, dtype):
    return q.astype(np.float64) if dtype == "float64" else q


def _case(n, dtype):
    """(store fp32, query of `dtype`, exact (D, S) sums) for N = n; 52 is the first ladder."""
    if n == 52:
        store, q = cases.ladder_case(cases.LADDER_SEEDS[0])[:2]
        q = _query(q, dtype)
        return store, q, _ladder_parts(dtype)
    store, q, _, _ = cases.random_case(n, 0, dtype)
    return store, q, cases._PARTS[n, 0, dtype]


_LADDER_PARTS = {}


def _ladder_parts(dtype):
    if dtype not in _LADDER_PARTS:
        store, q = cases.ladder_case(cases.LADDER_SEEDS[0])[:2]
        _LADDER_PARTS[dtype] = cases.exact_parts(store, _query(q, dtype))
    return _LADDER_PARTS[dtype]


def _check(idx, sims, want_sims, k, n, what):
    order = cases.rank(want_sims)
    assert cases.min_gap(want_sims, order) >= cases.GAP, what
    k_eff = min(k, n)
    assert sims.dtype == np.float64 and idx.dtype == np.int64, what
    assert idx.tolist() == order[:k_eff], what
    assert np.max(np.abs(sims - want_sims[order[:k_eff]])) <= TOL, what


# ---- flat -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", [1, 3, 52, 257, 4100, 16500])
def test_flat_equals_the_oracle(n, dtype):
    vo = _vo()
    store, q, parts = _case(n, dtype)
    fs = vo.FeatureStore(store)
    host_sims = cases.sims_from_parts(*parts, cases.host_query_norm(q))
    dev_sims = cases.sims_from_parts(*parts, cases.exact_query_norm(q))
    q_dev = torch.from_numpy(q).to(DEV)
    for k in KS + (n + 3,):
        idx, sims = fs.search(q, k, exact64=True)                                   # a host query: numpy's own norm travels with it
        _check(idx, sims, host_sims, k, n, f"host query n={n} k={k} {dtype}")
        idx_d, sims_d = fs.search_device(q_dev, k, exact64=True)                    # a device query: the kernel forms the norm
        assert sims_d.dtype == torch.float64 and idx_d.dtype == torch.int64
        _check(idx_d.cpu().numpy(), sims_d.cpu().numpy(), dev_sims, k, n, f"device query n={n} k={k} {dtype}")


@pytest.fixture(scope="module")
def golden():
    return json.loads((HERE / "golden" / "exact64_golden.json").read_text())


@pytest.mark.parametrize("seed", cases.LADDER_SEEDS)
def test_ladder_ranks_as_the_reference_recorded(golden, seed):
    """The reference's call: a float64 store of fp32 values, an fp32 host query.  The twelve rungs come out in the reference's
    order with its similarities; the default route gives them one value (fp32 arithmetic cannot tell them apart)."""
    vo = _vo()
    store, q, order, sims, ladder = cases.ladder_case(seed)
    ref = golden["ladder"][str(seed)]
    b64 = store.astype(np.float64)
    idx, got = vo.top_k_cosine_similarity(q, b64, golden["ladder_k"], exact64=True)
    assert idx.tolist() == ref["idx"] == order[:len(ref["idx"])] and got.dtype == np.float64
    assert np.max(np.abs(got - np.array(ref["sims"]))) <= TOL and np.max(np.abs(got - sims[idx])) <= TOL
    idx0, got0 = vo.top_k_cosine_similarity(q, b64, 12)           # the default: fp32 arithmetic, widened
    assert got0.dtype == np.float64 and sorted(idx0.tolist()) == sorted(ladder)
    assert len(set(got0.tolist())) < 12 and np.array_equal(got0, got0.astype(np.float32).astype(np.float64))


# ---- invariance: a row's bits depend on the row, the query and A alone --------------------------------------------------------------
PLACES = [0, 63, 64, 1000, 2047, 2048, 2049, 3000, 4095, 4096, 4098, 4099]


def test_ladder_bits_do_not_depend_on_n_position_k_or_entry_point():
    vo = _vo()
    store, q, order, sims, ladder = cases.ladder_case(cases.LADDER_SEEDS[0])
    small = vo.FeatureStore(store)
    idx, val = small.search(q, 52, exact64=True)
    bits = {int(i): int(b) for i, b in zip(idx, _bits(val))}
    rung_bits = [bits[r] for r in ladder]                          # in the oracle's order
    assert len(set(rung_bits)) == 12
    for k in KS + (55,):                                           # every k: a prefix of the same list, the same bits
        i_k, v_k = small.search(q, k, exact64=True)
        assert i_k.tolist() == idx[:k].tolist() and np.array_equal(_bits(v_k), _bits(val)[:k])
    big_rows = cases.random_case(4100)[0].copy()
    for place, r in zip(PLACES, ladder):
        big_rows[place] = store[r]
    big = vo.FeatureStore(big_rows)
    for k in (12, 70, 4100):                                       # arg-max rounds, LDS chunks, the full sort
        i_b, v_b = big.search(q, k, exact64=True)
        assert i_b[:12].tolist() == PLACES and _bits(v_b)[:12].tolist() == rung_bits
    offsets = torch.tensor([0, 1, 70, 2048, 2049, 4100], dtype=torch.int64, device=DEV)
    i_s, v_s, c_s = big.search_segments_device(q, offsets, 70, exact64=True)
    i_s, b_s, c_s, off = i_s.cpu().numpy(), _bits(v_s.cpu().numpy()), c_s.cpu().numpy(), offsets.cpu().numpy()
    seen = {}
    for e in range(5):
        for slot in range(int(c_s[e])):
            seen[int(off[e] + i_s[e, slot])] = int(b_s[e, slot])
    assert [seen[p] for p in PLACES] == rung_bits


# ---- order ------------------------------------------------------------------------------------------------------------------------
def test_ties_nan_and_k_beyond_n():
    vo = _vo()
    store = cases.random_case(257)[0][:40].copy()
    q = cases.random_case(257)[1]
    store[7] = store[3]
    store[9] = store[3]
    store[31] = store[30]
    store[5] = 0.0
    store[22] = 0.0
    want = cases.exact_sims(store, q, cases.host_query_norm(q))
    order = cases.rank(want)
    assert order[:2] == [22, 5] and order.index(9) + 1 == order.index(7) and order.index(7) + 1 == order.index(3)
    fs = vo.FeatureStore(store)
    for k in (1, 2, 3, 40, 43, 70):
        idx, sims = fs.search(q, k, exact64=True)
        assert idx.tolist() == order[:k] and len(idx) == min(k, 40)
        assert np.isnan(sims[:min(k, 2)]).all() and np.max(np.abs(sims[2:] - want[order[2:k]]), initial=0.0) <= TOL
        if k >= 40:
            assert _bits(sims)[order.index(9)] == _bits(sims)[order.index(7)] == _bits(sims)[order.index(3)]


# ---- segmented --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 70])
def test_segmented_equals_the_flat_call_on_every_slice(k):
    """Empty events, one-row events, a 500-row event, an event that starts at an odd row (inside a wave's row pair)."""
    vo = _vo()
    store, q, _, _ = cases.random_case(4100)
    fs = vo.FeatureStore(store)
    off = [0, 0, 1, 2, 2, 502, 503, 1003, 1003, 4100]
    offsets = torch.tensor(off, dtype=torch.int64, device=DEV)
    idx, sims, counts = (t.cpu().numpy() for t in fs.search_segments_device(q, offsets, k, exact64=True))
    assert idx.shape == sims.shape == (9, k) and sims.dtype == np.float64 and counts.dtype == np.int32
    for e in range(9):
        n_e = off[e + 1] - off[e]
        assert counts[e] == min(k, n_e)
        assert (idx[e, counts[e]:] == -1).all() and (_bits(sims[e, counts[e]:]) == 0).all()        # today's padding: -1 / 0
        if n_e:
            i_f, v_f = vo.FeatureStore(fs.rows[off[e]: off[e + 1]]).search(q, k, exact64=True)
            assert idx[e, :counts[e]].tolist() == i_f.tolist()
            assert np.array_equal(_bits(sims[e, :counts[e]]), _bits(v_f))
    # one event of 4100 rows: more than a workgroup of the arg-max rounds keeps in registers (16 x 256), so it re-reads its range
    whole = torch.tensor([0, 4100], dtype=torch.int64, device=DEV)
    i_w, v_w, c_w = (t.cpu().numpy() for t in fs.search_segments_device(q, whole, k, exact64=True))
    i_f, v_f = fs.search(q, k, exact64=True)
    assert c_w.tolist() == [k] and i_w[0].tolist() == i_f.tolist() and np.array_equal(_bits(v_w[0]), _bits(v_f))
    per_event = vo.EventStore([store[a:b] for a, b in zip(off[:-1], off[1:])]).top_k_per_event(q, k, exact64=True)
    for e, (i_e, v_e) in enumerate(per_event):
        assert i_e.tolist() == idx[e, :counts[e]].tolist() and np.array_equal(_bits(v_e), _bits(sims[e, :counts[e]]))


# ---- relevant_hits / top_hits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cases.THRESHOLD_SEEDS)
def test_threshold_decision_and_ranking_are_the_oracles(seed):
    vo = _vo()
    events, q, defer, sims = cases.threshold_case(seed)
    es = vo.EventStore([ev.astype(np.float64) for ev in events])
    assert es.f64_exact is True
    k = 5
    idx = np.stack([np.array(cases.rank(s)[:k]) for s in sims])
    val = np.stack([s[i] for s, i in zip(sims, idx)])
    want_hits, want_deferred = cases.model_hits(idx, val, np.full(3, k, np.int32), 5, None, defer)
    assert want_deferred == [0] and want_hits[0][0] == 1
    hits, deferred = es.relevant_hits(q, k, 5, defer=defer, exact64=True)
    assert [e for e, _, _ in deferred] == [0]                     # A is below 0.4 as a double: deferred; its twin B is ranked
    assert [(e, r) for e, r, _ in hits] == [(e, r) for e, r, _ in want_hits]
    assert max(abs(s - w) for (_, _, s), (_, _, w) in zip(hits, want_hits)) <= TOL
    assert deferred[0][1].tolist() == idx[0].tolist() and np.max(np.abs(deferred[0][2] - val[0])) <= TOL
    assert deferred[0][2].dtype == np.float64
    # top_hits: no rule, every hit ranked
    all_hits = cases.model_hits(idx, val, np.full(3, k, np.int32), 7, None, None)[0]
    got = es.top_hits(q, k, 7, exact64=True)
    assert [(e, r) for e, r, _ in got] == [(e, r) for e, r, _ in all_hits]
    from hippomm_amd import retrieval                              # the callers' step carries the keyword down

    class Ev:
        def __init__(self, n, flag):
            self.features = {"vision": None}
            self.frame_times = [float(t) for t in range(n)]
            self.frames = [f"f{t}" for t in range(n)]
            self.frame_captions = ["c"] if flag else []

    evs = [Ev(len(ev), f) for ev, f in zip(events, defer)]
    asked = []
    retrieval.find_relevant_video_segments(evs, q, store=es, deferred=lambda ev, i, s: asked.append(evs.index(ev)) or [], exact64=True)
    assert asked == [0]


def test_switch_off_is_todays_route_bit_for_bit():
    vo = _vo()
    events, q, defer, _ = cases.threshold_case(cases.THRESHOLD_SEEDS[0])
    es = vo.EventStore([ev.astype(np.float64) for ev in events])
    base = es.relevant_hits(q, 5, 5, defer=defer)
    per_event = es.top_k_per_event(q, 5)
    assert all(v.dtype == np.float32 for _, v in per_event)
    import relevant_hits_model as model
    want = model.relevant_hits(per_event, 5, None, defer)
    assert base[0] == want[0] and [e for e, _, _ in base[1]] == [e for e, _, _ in want[1]]
    vo.enable_exact64()                                            # the module switch does not reach the EventStore methods
    try:
        again = es.relevant_hits(q, 5, 5, defer=defer, exact64=False)
        assert again[0] == base[0] and [e for e, _, _ in again[1]] == [e for e, _, _ in base[1]]
        assert es.top_hits(q, 5, 5) == es.top_hits(q, 5, 5, exact64=False)
        store, lq = cases.ladder_case(cases.LADDER_SEEDS[0])[:2]
        i32, v32 = vo.top_k_cosine_similarity(lq, store, 12)       # fp32 in, fp32 out: the switch does not apply
        assert v32.dtype == np.float32
        i64, v64 = vo.top_k_cosine_similarity(lq, store.astype(np.float64), 12)      # float64 out anyway: the route is taken
        ie, ve = vo.top_k_cosine_similarity(lq, store.astype(np.float64), 12, exact64=True)
        assert i64.tolist() == ie.tolist() and np.array_equal(_bits(v64), _bits(ve))
    finally:
        vo.disable_exact64()
    i_off, v_off = vo.top_k_cosine_similarity(lq, store.astype(np.float64), 12)
    assert np.array_equal(v_off, v32.astype(np.float64)) and i_off.tolist() == i32.tolist()


# ---- eligibility ------------------------------------------------------------------------------------------------------------------
def test_eligibility_of_device_sources(caplog):
    vo = _vo()
    clean = torch.from_numpy(cases.random_case(257)[0][:20].astype(np.float64)).to(DEV)
    q = cases.random_case(257)[1]
    assert vo.FeatureStore(clean).f64_exact is True
    assert vo.FeatureStore(clean.float()).f64_exact is None
    dirty = clean.clone()
    dirty[11, 77] = 1 / 3
    dirty[15, 3] = 0.1
    fs = vo.FeatureStore(dirty)
    assert fs.f64_exact is False
    with pytest.raises(ValueError, match=r"row 11, column 77"):
        fs.search(q, 5, exact64=True)
    with pytest.raises(ValueError, match=r"row 11, column 77"):
        vo.top_k_cosine_similarity(q, fs, 5, exact64=True)
    vo.enable_exact64()
    try:
        vo._warned_not_exact = False
        with caplog.at_level(logging.WARNING, logger="hippomm_amd.vector_ops"):
            i1, v1 = vo.top_k_cosine_similarity(q, fs, 5)          # not eligible: one warning, today's route
            vo.top_k_cosine_similarity(q, fs, 5)
        assert len([r for r in caplog.records if "row 11" in r.getMessage()]) == 1
    finally:
        vo.disable_exact64()
    i0, v0 = vo.top_k_cosine_similarity(q, fs, 5)
    assert i1.tolist() == i0.tolist() and np.array_equal(v1, v0)
    es = vo.EventStore([cases.random_case(257)[0][:4].astype(np.float64)])
    assert es.f64_exact is True
    assert vo.EventStore.from_device_rows(clean.float().contiguous(), [20]).f64_exact is None
    es.append_event(clean)                                         # clean float64 rows, on the device: stays True
    es.append_event(cases.random_case(257)[0][:2])                 # fp32 rows do not change it
    assert es.f64_exact is True
    es.append_event(dirty)                                         # event 3, rows 26 .. 45
    assert es.f64_exact is False
    with pytest.raises(ValueError, match=r"row 37, column 77"):
        es.relevant_hits(q, 5, 5, exact64=True)
    es.remove_events([3])
    assert es.f64_exact is False                                   # conservative: False until the store is rebuilt
    es.replace_event(0, clean[:3])
    assert es.f64_exact is False
    with pytest.raises(ValueError, match="prefilter"):
        vo.EventStore([cases.random_case(257)[0][:4]]).top_hits(q, 5, 5, prefilter=True, exact64=True)


# ---- memory contract ----------------------------------------------------------------------------------------------------------------
def _contract_run(pattern, ws_align, kind, n, k, off):
    from hippomm_amd import _lib
    lib = _lib.load()
    store, q = cases.random_case(4100)[:2]
    store = torch.from_numpy(store[:n])
    E = len(off) - 1 if off else 0
    ws_bytes = (lib.hmm_cosine_topk_segmented_f64_workspace_bytes(n, E, k) if off else lib.hmm_cosine_topk_f64_workspace_bytes(n, k))
    cells = E * k if off else min(k, n)
    sizes = [store.numel() * 4, 4096, 8, 8 * (E + 1), 8 * cells, 8 * cells, 4 * max(E, 1), ws_bytes]
    ar = A.GuardedArena(A.needed_bytes(sizes), DEV, A.PATTERNS[pattern])
    s_v = ar.put(store.to(DEV), "store")
    q_v = ar.put(torch.from_numpy(q).to(DEV), "query")
    norm_v = ar.put(torch.tensor([cases.host_query_norm(q)], dtype=torch.float64, device=DEV), "norm")
    off_v = ar.put(torch.tensor(off or [0], dtype=torch.int64, device=DEV), "offsets")
    idx_v, sim_v = ar.carve(8 * cells, "idx"), ar.carve(8 * cells, "sims")
    cnt_v = ar.carve(4 * max(E, 1), "counts")
    ws_v = ar.carve(ws_bytes, "workspace", ws_align)
    p = ar.address
    if off:
        rc = lib.hmm_cosine_topk_segmented_f64(p(s_v), n, 1024, p(q_v), 0, p(norm_v), p(off_v), E, k, p(idx_v), p(sim_v), p(cnt_v),
                                               p(ws_v), ws_bytes, _lib.stream_ptr())
    else:
        rc = lib.hmm_cosine_topk_f64(p(s_v), n, 1024, p(q_v), 0, p(norm_v), k, p(idx_v), p(sim_v), p(cnt_v), p(ws_v), ws_bytes,
                                     _lib.stream_ptr())
    assert rc == 0, lib.hmm_last_error()
    torch.cuda.synchronize()
    ar.check_guards()
    return tuple(v.cpu().numpy().tobytes() for v in (idx_v, sim_v, cnt_v))


CONTRACT = {"flat argmax": ("flat", 4100, 5, None), "flat chunks": ("flat", 4100, 70, None), "flat one block": ("flat", 3, 5, None),
            "flat full sort": ("flat", 1500, 1100, None), "segmented": ("seg", 1003, 5, [0, 0, 1, 2, 2, 502, 503, 1003]),
            "segmented chunks": ("seg", 1003, 70, [0, 1, 503, 1003])}


@pytest.mark.parametrize("name", list(CONTRACT))
def test_memory_contract(name):
    """Every buffer carved at its exact size from a poisoned, guarded arena; the workspace exactly what *_workspace_bytes answers,
    at 256- and at 16-byte alignment: guards untouched, and the same output bytes whatever the workspace and outputs held before."""
    _vo()
    kind, n, k, off = CONTRACT[name]
    outs = [_contract_run(pattern, align, kind, n, k, off) for pattern in A.PATTERNS for align in (256, 16)]
    assert all(o == outs[0] for o in outs[1:])
    idx = np.frombuffer(outs[0][0], np.int64)
    if kind == "flat":
        q = cases.random_case(4100)[1]
        D, S = cases._PARTS[4100, 0, "float32"]                    # the sums the flat tests share
        want = cases.rank(cases.sims_from_parts(D[:n], S[:n], cases.host_query_norm(q)))[:k]
        assert idx.tolist() == want and np.frombuffer(outs[0][2], np.int32)[0] == min(k, n)


def test_eligibility_report_contract():
    from hippomm_amd import _lib
    _vo()
    lib = _lib.load()
    src = torch.from_numpy(cases.random_case(257)[0][:9].astype(np.float64))
    src[8, 1023] = 1 / 3                                           # the very last value
    src[4, 0] = 0.1
    for pattern in A.PATTERNS:
        ar = A.GuardedArena(A.needed_bytes([src.numel() * 8, 16]), DEV, A.PATTERNS[pattern])
        s_v, r_v = ar.put(src.to(DEV), "source"), ar.carve(16, "report")
        assert lib.hmm_rows_f64_are_f32(ar.address(s_v), 9, 1024, ar.address(r_v), _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        ar.check_guards()
        assert r_v.view(torch.int64).tolist() == [2, 4 * 1024]
        assert lib.hmm_rows_f64_are_f32(ar.address(s_v), 4, 1024, ar.address(r_v), _lib.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert r_v.view(torch.int64).tolist() == [0, -1]
