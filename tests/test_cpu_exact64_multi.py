"""CPU: the batched float64 route's exports, workspace answers, argument checks, query upload and host-side ranking (no GPU needed).

The GPU half is tests/test_gpu_exact64_multi.py; both use tests/exact64_cases.py and tests/exact64_multi_cases.py."""
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import exact64_cases as cases  # noqa: E402
import exact64_multi_cases as multi  # noqa: E402

NEW_EXPORTS = ["hmm_cosine_topk_multi_f64", "hmm_cosine_topk_multi_f64_workspace_bytes", "hmm_cosine_topk_segmented_multi_f64",
               "hmm_cosine_topk_segmented_multi_f64_workspace_bytes"]
SINGLE_EXPORTS = ["hmm_cosine_topk_f64", "hmm_cosine_topk_f64_workspace_bytes", "hmm_cosine_topk_segmented_f64",
                  "hmm_cosine_topk_segmented_f64_workspace_bytes"]


def test_exports_are_declared_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, vector_ops
    header = (HERE.parent / "include" / "hippomm_hip.h").read_text()
    api = (HERE.parent / "hippomm_amd" / "csrc" / "hmm_api.cpp").read_text()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert name + "(" in header and name in _lib._SIGNATURES and hasattr(lib, name)
    assert "hmm_cosine_topk_multi_f64, hmm_cosine_topk_segmented_multi_f64" in api
    assert lib.hmm_abi_version() == 7
    named = {v[0] for v in vector_ops._F64_MULTI_ROUTES.values()} | {v[1] for v in vector_ops._F64_MULTI_ROUTES.values()}
    assert named == set(NEW_EXPORTS)
    single = {v[0] for v in vector_ops._F64_ROUTES.values()} | {v[1] for v in vector_ops._F64_ROUTES.values()}
    assert single == set(SINGLE_EXPORTS)                          # the single table is as it was
    assert not any("f64" in name for route in vector_ops._ROUTES.values() for name in route[:2])


def test_workspace_answers():
    from hippomm_amd import _lib
    lib = _lib.load()
    flat, seg = lib.hmm_cosine_topk_multi_f64_workspace_bytes, lib.hmm_cosine_topk_segmented_multi_f64_workspace_bytes
    assert flat(0, 4, 5) == 0 and flat(-1, 4, 5) == 0 and flat(100, 0, 5) == 0 and flat(100, 4, 0) == 0
    assert seg(100, 3, 0, 5) == 0 and seg(100, 3, 4, 0) == 0 and seg(100, 0, 4, 5) == 0
    for n in (1, 3, 4100, 100000):
        for k in (1, 5, 70, 1100):
            assert flat(n, 16, k) == flat(n, 40, k) and seg(n, 7, 16, k) == seg(n, 7, 40, k)      # one pass, however many questions
            for Q in (1, 2, 15, 16, 17, 33):
                assert flat(n, Q, k) >= min(Q, 16) * n * 8 and seg(n, 7, Q, k) >= min(Q, 16) * n * 8
            assert flat(n, 1, k) <= flat(n, 2, k) <= flat(n, 16, k)


def test_a_single_query_gets_the_workspace_of_a_batch_of_one():
    from hippomm_amd import _lib
    lib = _lib.load()
    for n in (1, 3, 4096, 4097, 100000):
        for k in (1, 64, 65, 1024, 1025):
            assert lib.hmm_cosine_topk_f64_workspace_bytes(n, k) == lib.hmm_cosine_topk_multi_f64_workspace_bytes(n, 1, k) > 0
            assert (lib.hmm_cosine_topk_segmented_f64_workspace_bytes(n, 7, k)
                    == lib.hmm_cosine_topk_segmented_multi_f64_workspace_bytes(n, 7, 1, k) > 0)


def test_argument_errors_are_reported_without_a_gpu():
    from hippomm_amd import _lib
    lib = _lib.load()
    A = 4096                                                      # an aligned dummy address: nothing is dereferenced on a refusal

    def flat(store=A, n=10, dim=1024, q=A, qd=0, norms=None, Q=3, k=5, idx=A, sim=A, n_out=None, ws=A, ws_bytes=1 << 20):
        return lib.hmm_cosine_topk_multi_f64(store, n, dim, q, qd, norms, Q, k, idx, sim, n_out, ws, ws_bytes, None)

    def seg(store=A, n=10, dim=1024, q=A, qd=0, norms=None, Q=3, off=A, E=2, k=5, idx=A, sim=A, cnt=A, ws=A, ws_bytes=1 << 20):
        return lib.hmm_cosine_topk_segmented_multi_f64(store, n, dim, q, qd, norms, Q, off, E, k, idx, sim, cnt, ws, ws_bytes, None)

    shared = [({"store": None}, -1, b"null pointer"), ({"q": None}, -1, b"null pointer"), ({"idx": None}, -1, b"null pointer"),
              ({"sim": None}, -1, b"null pointer"), ({"ws": None}, -1, b"null pointer"), ({"dim": 512}, -1, b"dim must be 1024"),
              ({"qd": 2}, -1, b"query_dtype"), ({"qd": -1}, -1, b"query_dtype"), ({"Q": 0}, -1, b"n_queries must be >= 1"),
              ({"k": 0}, -1, b"k must be >= 1"), ({"store": A + 8}, -1, b"16-byte aligned"), ({"q": A + 8}, -1, b"16-byte aligned"),
              ({"ws": A + 8}, -1, b"16-byte aligned"), ({"norms": A + 4}, -1, b"8-byte aligned"), ({"idx": A + 4}, -1, b"8-byte aligned"),
              ({"sim": A + 4}, -1, b"8-byte aligned"), ({"ws_bytes": 16}, -2, b"workspace too small")]
    for call, name, extra in [
            (flat, b"cosine_topk_multi_f64", [({"n": 0}, -1, b"n_rows")]),
            (seg, b"cosine_topk_segmented_multi_f64", [({"k": 1025}, -1, b"k <= 1024"), ({"E": 0}, -1, b"n_segments"),
                                                       ({"off": None}, -1, b"null pointer"), ({"cnt": None}, -1, b"null pointer"),
                                                       ({"off": A + 4}, -1, b"8-byte aligned"), ({"n": -1}, -1, b"n_rows")])]:
        for kwargs, code, text in shared + extra:
            assert call(**kwargs) == code, (name, kwargs, lib.hmm_last_error())
            assert name + b":" in lib.hmm_last_error() and text in lib.hmm_last_error(), (kwargs, lib.hmm_last_error())
    # the workspace of one pass is enough for any number of questions, and one byte less is refused
    need = lib.hmm_cosine_topk_multi_f64_workspace_bytes(10, 40, 5)
    assert flat(Q=40, ws_bytes=need - 1) == -2


# ---- the query upload -------------------------------------------------------------------------------------------------------------
def _uploaded(batch):
    """(norms float64[Q], queries as uploaded) read back out of the buffer _exact64_queries built on the host."""
    buf, q_ptr, q_dtype, norms_ptr, Q = batch
    raw = buf.numpy()
    base = buf.data_ptr()
    norms = raw[norms_ptr - base: norms_ptr - base + 8 * Q].view(np.float64)
    item = 8 if q_dtype else 4
    rows = raw[q_ptr - base: q_ptr - base + Q * 1024 * item].view(np.float64 if q_dtype else np.float32).reshape(Q, 1024)
    return norms, rows


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("Q", [1, 2, 15, 17])
def test_host_batches_travel_with_numpys_own_norm_of_every_row(Q, dtype):
    from hippomm_amd.vector_ops import _exact64_queries
    q = multi.query_batch(Q, dtype, seed=Q)
    batch = _exact64_queries(q, "cpu")
    norms, rows = _uploaded(batch)
    assert batch[2] == int(dtype == "float64") and batch[4] == Q and batch[1] % 16 == 0 and batch[3] % 8 == 0
    want = np.array([np.linalg.norm(row) for row in q], dtype=np.float64)          # the 1-D call, one per row
    assert np.array_equal(norms.view(np.uint64), want.view(np.uint64))
    assert rows.dtype == q.dtype and np.array_equal(rows.view(np.uint8), q.view(np.uint8))
    # a strided view of a wider array is uploaded as its contiguous rows, with the norms of those
    wide = np.zeros((Q, 2048), q.dtype)
    wide[:, ::2] = q
    norms2, rows2 = _uploaded(_exact64_queries(wide[:, ::2], "cpu"))
    assert np.array_equal(norms2.view(np.uint64), want.view(np.uint64)) and np.array_equal(rows2, q)


def test_other_dtypes_become_float32_and_a_wrong_width_is_refused():
    from hippomm_amd.vector_ops import _exact64_queries
    ints = np.arange(3 * 1024, dtype=np.int64).reshape(3, 1024) % 7 - 3
    batch = _exact64_queries(ints, "cpu")
    norms, rows = _uploaded(batch)
    assert batch[2] == 0 and rows.dtype == np.float32 and np.array_equal(rows, ints.astype(np.float32))
    want = np.array([np.linalg.norm(row) for row in ints.astype(np.float32)], dtype=np.float64)
    assert np.array_equal(norms.view(np.uint64), want.view(np.uint64))
    half = _exact64_queries(multi.query_batch(2, "float32").astype(np.float16), "cpu")
    assert half[2] == 0 and _uploaded(half)[1].dtype == np.float32
    for bad in (np.zeros((3, 1000), np.float32), np.zeros(1024, np.float32), np.zeros((2, 3, 1024), np.float64),
                np.zeros((0, 1024), np.float32)):
        with pytest.raises(ValueError):
            _exact64_queries(bad, "cpu")


# ---- ranking per question on the host -----------------------------------------------------------------------------------------------
def test_host_rules_per_question_equal_the_model_on_planted_hits():
    from hippomm_amd.vector_ops import rank_hits_exact64
    rng = np.random.default_rng(11)
    for trial in range(8):
        Q, E, k = int(rng.integers(1, 6)), int(rng.integers(1, 9)), int(rng.integers(1, 7))
        idx, sims, counts = multi.planted_hits(rng, Q, E, k)
        row_limits = None if trial % 2 else rng.integers(0, 20, E)
        defer = None if trial % 3 == 0 else rng.integers(0, 2, E).astype(bool)
        keep = int(rng.integers(1, 12))
        for qi in range(Q):
            hits, deferred = rank_hits_exact64(idx[qi], sims[qi], counts[qi], keep, row_limits, defer, 0.4)
            want_hits, want_deferred = cases.model_hits(idx[qi], sims[qi], counts[qi], keep, row_limits, defer)
            assert [(e, r) for e, r, _ in hits] == [(e, r) for e, r, _ in want_hits]
            np.testing.assert_array_equal([s for _, _, s in hits], [s for _, _, s in want_hits])
            assert [e for e, _, _ in deferred] == want_deferred


def test_the_packed_layout_serves_a_batch():
    from hippomm_amd.vector_ops import _hits_layout_f64
    layout = _hits_layout_f64(3, 4, 5)
    assert layout.offsets == [0, 3 * 4 * 5 * 8, 2 * 3 * 4 * 5 * 8] and layout.nbytes == 2 * 480 + 3 * 4 * 4
    raw = np.zeros(layout.nbytes, np.uint8)
    idx, sims, counts = layout.host_views(raw)
    assert idx.shape == sims.shape == (3, 4, 5) and counts.shape == (3, 4) and sims.dtype == np.float64
