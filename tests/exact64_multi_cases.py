"""Inputs for the batched float64 route (exact64=True on the ``_multi`` calls); beside tests/exact64_cases.py, whose oracle,
generators and TOL = 2^-42 the batched tests reuse.  The generators ASSERT what the tests rely on.  numpy only."""
import functools

import numpy as np

import exact64_cases as cases

DIM = cases.DIM
SEGMENT_OFFSETS = [0, 0, 1, 2, 2, 502, 503, 1003]               # empty events, one-row events, boundaries inside a block of four rows
BATCH_SIZES = (1, 2, 15, 16, 17, 33)                            # below one pass, one pass, one past it, three passes with a lone tail
STORE_SIZES = (1, 2, 3, 52, 257, 4100)


@functools.lru_cache(maxsize=None)
def query_batch(Q: int, dtype: str = "float32", seed: int = 0) -> np.ndarray:
    """(Q,1024) random questions of norm ~1.7, distinct rows.  float64: genuine doubles, no row of which is fp32-valued."""
    rng = np.random.default_rng(7000 + 31 * Q + seed)
    q = rng.standard_normal((Q, DIM))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True) * 1.7).astype(np.float32)
    if dtype == "float64":
        q = q.astype(np.float64) * (1.0 + rng.uniform(-1e-9, 1e-9, (Q, DIM)))
        assert not any(cases.is_f32_valued(row) for row in q)
    else:
        assert dtype == "float32"
    assert len({row.tobytes() for row in q}) == Q
    q.setflags(write=False)
    return q


def batch_with(query, position: int, Q: int, seed: int = 0) -> np.ndarray:
    """A batch of Q questions in the dtype of ``query`` with ``query`` at ``position`` among random ones."""
    query = np.asarray(query).reshape(-1)
    assert query.size == DIM and 0 <= position < Q and query.dtype in (np.float32, np.float64)
    batch = query_batch(Q, str(query.dtype), seed).copy()
    batch[position] = query
    assert batch.dtype == query.dtype and batch[position].tobytes() == query.tobytes()
    return batch


@functools.lru_cache(maxsize=None)
def store_rows(n: int) -> np.ndarray:
    """(n,1024) fp32 rows, n <= 4100: the 52-row ladder store or the first n rows of the 4100-row random store (unit rows)."""
    assert 1 <= n <= 4100
    rows = cases.ladder_case(cases.LADDER_SEEDS[0])[0] if n == 52 else cases.random_case(4100)[0][:n]
    assert rows.shape == (n, DIM) and rows.dtype == np.float32 and cases.is_f32_valued(rows)
    return rows


def ties_store():
    """(store (40,1024), the rows that are exact copies [(original, copy), ...], the zero rows): duplicate rows tie exactly, a
    zero row gives 0 / 0 = NaN for every question."""
    store = cases.random_case(257)[0][:40].copy()
    store[7] = store[3]
    store[9] = store[3]
    store[31] = store[30]
    store[5] = 0.0
    store[22] = 0.0
    assert np.array_equal(store[3], store[9]) and not store[5].any() and cases.is_f32_valued(store)
    return store, [(3, 7), (7, 9), (30, 31)], [5, 22]


def planted_hits(rng, Q: int, E: int, k: int):
    """(idx (Q,E,k) int64 -1 padded, sims (Q,E,k) float64 0 padded, descending per event, counts (Q,E) int32 >= 1).  For the first
    question a NaN best similarity and, across the first two events, an exact tie of best similarities are planted over that."""
    counts = np.broadcast_to(rng.integers(1, k + 1, E).astype(np.int32), (Q, E)).copy()
    idx = np.full((Q, E, k), -1, np.int64)
    sims = np.zeros((Q, E, k))
    for q in range(Q):
        for e in range(E):
            c = counts[q, e]
            sims[q, e, :c] = np.sort(rng.uniform(0.2, 0.6, c))[::-1]
            idx[q, e, :c] = rng.permutation(20)[:c]
    if counts[0, 0] > 1:
        sims[0, 0, 0] = np.nan
    if E > 1:
        sims[0, 1, 0] = sims[0, 0, 0]
    assert (counts >= 1).all() and (idx[..., 0] >= 0).all()
    return idx, sims, counts
