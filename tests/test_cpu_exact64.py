"""CPU: the float64 route's inputs, oracle, recorded reference results, exports and host-side rules (no GPU needed).

The GPU half is tests/test_gpu_exact64.py; both use tests/exact64_cases.py and its TOL = 2^-42, the route's derived bound."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE / "golden"))
import exact64_cases as cases  # noqa: E402

TOL = cases.TOL


@pytest.fixture(scope="module")
def golden():
    return json.loads((HERE / "golden" / "exact64_golden.json").read_text())


# ---- the generators' own conditions ---------------------------------------------------------------------------------------------
def test_tol_is_the_derived_bound():
    u = 2.0 ** -53
    derived = 1023 * u + (1023 * u / 2 + u) + 3 * u              # the dot, the root of S, the product and the division
    assert derived < 1.8e-13 < TOL == 2.0 ** -42


@pytest.mark.parametrize("seed", cases.LADDER_SEEDS)
def test_ladder_inputs_meet_their_conditions(seed):
    store, q, order, sims, ladder = cases.ladder_case(seed)       # asserts: fp32 values, gaps >= 8 TOL, fp32 order differs
    assert store.shape == (52, 1024) and store.dtype == np.float32 and q.dtype == np.float32
    gaps = -np.diff(sims[ladder])
    assert gaps.min() >= 8 * TOL and gaps.max() < 1e-9           # near-ties: far below fp32 resolution (6e-8)
    f32_sims = cases.f32_order(store, q)[1]
    assert len(set(f32_sims[ladder].tolist())) < len(ladder)     # fp32 arithmetic cannot tell the rungs apart


@pytest.mark.parametrize("seed", cases.THRESHOLD_SEEDS)
def test_threshold_inputs_meet_their_conditions(seed):
    events, q, defer, sims = cases.threshold_case(seed)
    below, above = 0.4 - sims[0].max(), sims[1].max() - 0.4
    assert 8 * TOL <= below <= 2e-8 and 8 * TOL <= above <= 2e-8
    assert defer == [True, True, False]


def test_oracle_is_exact_on_a_case_with_a_known_answer():
    x = np.zeros((3, 1024), np.float32)
    x[0, :4] = [3, 4, 0, 0]
    x[1, :4] = [1, 0, 0, 0]
    q = np.zeros(1024, np.float32)
    q[:2] = [3, 4]
    sims = cases.exact_sims(x, q, cases.host_query_norm(q))
    assert sims[0] == 1.0 and sims[1] == 0.6 and np.isnan(sims[2])
    assert cases.rank(sims) == [2, 0, 1]                          # NaN first
    assert cases.rank([0.5, 0.5, -0.0, 0.0]) == [1, 0, 3, 2]      # ties: higher index first; -0.0 == +0.0
    # a genuine float64 query: the two-product tail is what keeps the sum exact
    qd = q.astype(np.float64)
    qd[0] = 3.0 + 2.0 ** -40
    from fractions import Fraction
    D = Fraction(3) * Fraction(qd[0]) + Fraction(16)
    want = float(D / (5 * Fraction(cases.host_query_norm(qd))))
    assert abs(cases.exact_sims(x[:1], qd, cases.host_query_norm(qd))[0] - want) <= 2.0 ** -52


def test_device_query_norm_rule():
    store, q, _, _ = cases.random_case(3)
    assert cases.norm_is_unambiguous(q)
    assert cases.exact_query_norm(q) == float(np.float32(cases.exact_query_norm(q)))          # an fp32 number, widened
    assert abs(cases.exact_query_norm(q) - cases.host_query_norm(q)) <= 2.0 ** -23 * 1.7     # numpy's may differ in the last fp32 bit


# ---- the recorded reference against the exact oracle ----------------------------------------------------------------------------
def _check_against_oracle(ref, store, q):
    idx, sims = cases.top_k(store, q, len(ref["idx"]), cases.host_query_norm(q))
    assert ref["idx"] == idx.tolist()
    assert np.max(np.abs(np.array(ref["sims"]) - sims)) <= TOL


@pytest.mark.parametrize("seed", cases.LADDER_SEEDS)
def test_golden_ladder_equals_the_oracle(golden, seed):
    store, q = cases.ladder_case(seed)[:2]
    ref = golden["ladder"][str(seed)]
    assert len(ref["idx"]) == golden["ladder_k"] == 20
    _check_against_oracle(ref, store, q)


@pytest.mark.parametrize("seed", cases.THRESHOLD_SEEDS)
def test_golden_threshold_equals_the_oracle(golden, seed):
    events, q = cases.threshold_case(seed)[:2]
    for ref, ev in zip(golden["threshold"][str(seed)], events):
        _check_against_oracle(ref, ev, q)
    best = [ref["sims"][0] for ref in golden["threshold"][str(seed)]]
    assert best[0] < 0.4 < best[1]                                # the reference itself defers A and ranks B


def test_live_reference_equals_the_golden_file(golden):
    """Where the reference tree is present: the unmodified function, run in a subprocess, returns what the file records."""
    import make_golden
    if not Path(make_golden.REF, "hippomm", "utils", "vector_ops.py").exists():
        pytest.skip("the reference checkout is not on this machine")
    out = subprocess.run([sys.executable, str(HERE / "golden" / "make_exact64_golden.py"), "--stdout"], capture_output=True,
                         text=True, check=True).stdout
    assert json.loads(out) == golden


# ---- exports ----------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ["hmm_cosine_topk_f64", "hmm_cosine_topk_f64_workspace_bytes", "hmm_cosine_topk_segmented_f64",
               "hmm_cosine_topk_segmented_f64_workspace_bytes", "hmm_rows_f64_are_f32"]


def test_exports_are_declared_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, vector_ops
    header = (HERE.parent / "include" / "hippomm_hip.h").read_text()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert name + "(" in header and name in _lib._SIGNATURES and hasattr(lib, name)
    assert lib.hmm_abi_version() == 7
    assert {v[0] for v in vector_ops._F64_ROUTES.values()} | {v[1] for v in vector_ops._F64_ROUTES.values()} <= set(NEW_EXPORTS)
    assert not any("f64" in name for route in vector_ops._ROUTES.values() for name in route[:2])     # the shared table is untouched
    assert lib.hmm_cosine_topk_f64_workspace_bytes(1000, 5) >= 8000
    assert lib.hmm_cosine_topk_segmented_f64_workspace_bytes(1000, 3, 5) >= 8000
    assert lib.hmm_cosine_topk_f64_workspace_bytes(0, 5) == 0 and lib.hmm_cosine_topk_f64_workspace_bytes(10, 0) == 0


def test_argument_errors_are_reported_without_a_gpu():
    from hippomm_amd import _lib
    lib = _lib.load()
    A = 4096                                                      # an aligned dummy address: nothing is dereferenced on a refusal

    def flat(store=A, n=10, dim=1024, q=A, qd=0, norm=None, k=5, idx=A, sim=A, n_out=None, ws=A, ws_bytes=1 << 20):
        return lib.hmm_cosine_topk_f64(store, n, dim, q, qd, norm, k, idx, sim, n_out, ws, ws_bytes, None)

    def seg(store=A, n=10, dim=1024, q=A, qd=0, norm=None, off=A, E=2, k=5, idx=A, sim=A, cnt=A, ws=A, ws_bytes=1 << 20):
        return lib.hmm_cosine_topk_segmented_f64(store, n, dim, q, qd, norm, off, E, k, idx, sim, cnt, ws, ws_bytes, None)

    for call, kwargs, code, text in [
            (flat, {"idx": None}, -1, b"null output"), (flat, {"dim": 512}, -1, b"dim must be 1024"),
            (flat, {"qd": 2}, -1, b"query_dtype"), (flat, {"k": 0}, -1, b"k must be"), (flat, {"q": None}, -1, b"null query"),
            (flat, {"n": 0}, -1, b"n_rows"), (flat, {"store": A + 4}, -1, b"aligned"), (flat, {"norm": A + 4}, -1, b"aligned"),
            (flat, {"ws_bytes": 16}, -2, b"workspace too small"), (flat, {"ws": None}, -1, b"workspace"),
            (seg, {"dim": 77}, -1, b"dim must be 1024"), (seg, {"k": 1025}, -1, b"k <= 1024"), (seg, {"E": 0}, -1, b"n_segments"),
            (seg, {"off": None}, -1, b"null pointer"), (seg, {"cnt": None}, -1, b"null pointer"),
            (seg, {"ws_bytes": 8}, -2, b"workspace too small"), (seg, {"n": -1}, -1, b"n_rows")]:
        assert call(**kwargs) == code and text in lib.hmm_last_error(), (kwargs, lib.hmm_last_error())
    assert lib.hmm_rows_f64_are_f32(A, 4, 512, A, None) == -1 and b"dim must be 1024" in lib.hmm_last_error()
    assert lib.hmm_rows_f64_are_f32(A, 4, 1024, None, None) == -1 and b"report" in lib.hmm_last_error()
    assert lib.hmm_rows_f64_are_f32(None, 4, 1024, A, None) == -1 and b"source" in lib.hmm_last_error()


# ---- the host-side rules of relevant_hits(exact64=True) ---------------------------------------------------------------------------
def _planted(rng, E, k):
    counts = rng.integers(1, k + 1, E).astype(np.int32)
    idx = np.full((E, k), -1, np.int64)
    sims = np.zeros((E, k))
    for e in range(E):
        s = np.sort(rng.uniform(0.2, 0.6, counts[e]))[::-1]
        sims[e, :counts[e]] = s
        idx[e, :counts[e]] = rng.permutation(20)[:counts[e]]
    return idx, sims, counts


def test_host_rules_equal_the_model_on_planted_hits():
    from hippomm_amd.vector_ops import rank_hits_exact64
    rng = np.random.default_rng(5)
    for trial in range(20):
        E, k = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        idx, sims, counts = _planted(rng, E, k)
        if trial % 3 == 0 and counts[0] > 1:                     # a NaN best similarity never defers and ranks first
            sims[0, 0] = np.nan
        if trial % 4 == 0 and E > 1:                             # an exact tie across events: event order decides (stable sort)
            sims[1, 0] = sims[0, 0]
        row_limits = None if trial % 2 else rng.integers(0, 20, E)
        defer = None if trial % 5 == 0 else rng.integers(0, 2, E).astype(bool)
        keep = int(rng.integers(1, 12))
        hits, deferred = rank_hits_exact64(idx, sims, counts, keep, row_limits, defer, 0.4)
        want_hits, want_deferred = cases.model_hits(idx, sims, counts, keep, row_limits, defer)
        assert [(e, r) for e, r, _ in hits] == [(e, r) for e, r, _ in want_hits]
        np.testing.assert_array_equal([s for _, _, s in hits], [s for _, _, s in want_hits])
        assert [e for e, _, _ in deferred] == want_deferred
        for e, d_idx, d_sims in deferred:
            np.testing.assert_array_equal(d_idx, idx[e, :counts[e]])
            np.testing.assert_array_equal(d_sims, sims[e, :counts[e]])
            assert d_sims.dtype == np.float64


@pytest.mark.parametrize("seed", cases.THRESHOLD_SEEDS)
def test_host_rules_decide_the_threshold_cases_on_doubles(seed):
    from hippomm_amd.vector_ops import rank_hits_exact64
    events, q, defer, sims = cases.threshold_case(seed)
    k = 5
    idx = np.stack([np.array(cases.rank(s)[:k]) for s in sims])
    val = np.stack([s[i] for s, i in zip(sims, idx)])
    counts = np.full(3, k, np.int32)
    hits, deferred = rank_hits_exact64(idx, val, counts, 5, None, defer, 0.4)
    assert [e for e, _, _ in deferred] == [0]                    # A lies below 0.4 as a double, B above
    assert hits[0][0] == 1 and hits[0][2] == val[1, 0] and all(e != 0 for e, _, _ in hits)
    assert (hits, [e for e, _, _ in deferred]) == cases.model_hits(idx, val, counts, 5, None, defer)
    # as fp32 both best similarities are the same number: the default route cannot separate them
    assert np.float32(val[0, 0]) == np.float32(val[1, 0])


# ---- eligibility of host arrays -----------------------------------------------------------------------------------------------------
def test_eligibility_check_on_host_arrays():
    from hippomm_amd.vector_ops import first_not_f32
    a = np.random.default_rng(0).standard_normal((4, 1024)).astype(np.float32).astype(np.float64)
    assert first_not_f32(a) is None
    b = a.copy()
    b[2, 7] = 1 / 3
    b[3, 0] = 0.1
    assert first_not_f32(b) == 2 * 1024 + 7                      # the FIRST offending value
    c = a.copy()
    c[0, 0], c[0, 1], c[0, 2], c[0, 3] = np.nan, float(np.float32(1e-40)), -0.0, np.inf
    assert first_not_f32(c) is None                              # a plain NaN, an fp32 subnormal, -0.0 and inf are fp32 values
    d = a.copy()
    d[1, 5] = 1e-46                                              # below the smallest fp32 subnormal: narrows to 0
    assert first_not_f32(d) == 1024 + 5
    e = a.copy()
    e.view(np.uint64)[0, 9] = 0x7FF8000000000001                # a NaN whose payload does not narrow exactly
    assert first_not_f32(e) == 9
