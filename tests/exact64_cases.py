"""Inputs and an exact oracle for the float64 route (exact64=True; include/hippomm_hip.h, "float64-origin stores").

The oracle evaluates sim_r = D_r / (sqrt(S_r) * A) with D_r and S_r summed EXACTLY (math.fsum over exact products) and then sqrt,
* and / in Python floats: at most a few roundings of 2^-53 away from the real quotient.  The route's derived bound is
TOL = 2^-42 on a cosine; every comparison of these tests uses TOL and no other number.  The generators ASSERT what the tests
rely on (every row an fp32 value; neighbours in the expected order at least 8 TOL apart; fp32 arithmetic not reproducing the
order): an input that does not meet them is an error here, never a skipped case.  numpy only; nothing here needs a GPU."""
import functools
import math

import numpy as np

TOL = 2.0 ** -42
GAP = 8 * TOL
DIM = 1024
THRESHOLD = 0.4                      # the reference's `max(similarities) < 0.4`, a Python float

LADDER_SEEDS = (0, 3, 4)             # seeds whose inputs meet the generators' assertions (1 and 2 leave a gap under 8 TOL)
THRESHOLD_SEEDS = (1, 6)
LADDER_RUNGS, LADDER_FILL = 12, 40


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
def _two_prod(x, y):
    """x * y = p + e exactly (Dekker, Veltkamp split; no overflow at unit scale)."""
    p = x * y
    c = 134217729.0                                              # 2^27 + 1
    xh = (c * x) - ((c * x) - x)
    yh = (c * y) - ((c * y) - y)
    xl, yl = x - xh, y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return p, e


def is_f32_valued(a) -> bool:
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        back = a.astype(np.float32).astype(np.float64)
    return bool(np.array_equal(back.view(np.uint64), a.view(np.uint64)))


def exact_query_norm(a) -> float:
    """The A of a query that lives on the device: sqrt of the exact sum of squares; rounded to fp32 for an fp32 query."""
    a = np.asarray(a).reshape(-1)
    p, e = _two_prod(a.astype(np.float64), a.astype(np.float64))
    root = math.sqrt(math.fsum(p.tolist() + e.tolist()))
    return float(np.float32(root)) if a.dtype == np.float32 else root


def host_query_norm(a) -> float:
    """The A of a host query: numpy's own np.linalg.norm in the query's dtype, widened -- the reference's a_norm."""
    return float(np.linalg.norm(np.asarray(a).reshape(-1)))


def norm_is_unambiguous(a) -> bool:
    """For an fp32 query: sqrt(fsum(a^2)) is farther than 1e-12 relative from the midpoint of two fp32 neighbours, so rounding
    the device's fp64 root to fp32 has one answer."""
    a = np.asarray(a).reshape(-1)
    if a.dtype != np.float32:
        return True
    p, e = _two_prod(a.astype(np.float64), a.astype(np.float64))
    root = math.sqrt(math.fsum(p.tolist() + e.tolist()))
    near = np.float32(root)
    other = np.nextafter(near, np.float32(np.inf) if float(near) < root else np.float32(-np.inf))
    mid = (float(near) + float(other)) / 2
    return abs(root - mid) > 1e-12 * root


def exact_parts(rows, a):
    """(D float64[N], S float64[N]): per row the exactly summed dot with the query a (fp32 or fp64) and the exactly summed square
    norm, each rounded once (math.fsum).  The expensive half of the oracle; it does not depend on the norm rule."""
    x = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, DIM)
    assert is_f32_valued(x), "the oracle takes rows that are fp32 values"
    q = np.asarray(a).reshape(-1).astype(np.float64)
    p, e = _two_prod(x, q[None, :])
    tail = bool(np.any(e != 0.0))                                # an fp32-valued query: every product is exact already
    sq = x * x                                                    # exact: 24 + 24 bits
    D, S = np.empty(x.shape[0]), np.empty(x.shape[0])
    for r in range(x.shape[0]):
        D[r] = math.fsum(p[r].tolist() + e[r].tolist()) if tail else math.fsum(p[r].tolist())
        S[r] = math.fsum(sq[r].tolist())
    return D, S


def sims_from_parts(D, S, A: float) -> np.ndarray:
    """D / (sqrt(S) * A): sqrt, * and / on IEEE doubles, each correctly rounded, as Python floats do them; 0 / 0 is NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return D / (np.sqrt(S) * np.float64(A))


def exact_sims(rows, a, A: float) -> np.ndarray:
    """float64[N]: the oracle's similarity of every row (fp32 values, any float dtype) to the query a (fp32 or fp64) under norm A."""
    return sims_from_parts(*exact_parts(rows, a), A)


def rank(sims) -> list:
    """Row indices under the library's total order: NaN first, similarity descending, exact ties higher index first."""
    sims = np.asarray(sims, dtype=np.float64)
    return sorted(range(len(sims)), key=lambda i: ((0, 0.0) if sims[i] != sims[i] else (1, -(sims[i] + 0.0)), -i))


def top_k(rows, a, k: int, A: float):
    sims = exact_sims(rows, a, A)
    order = rank(sims)[:max(0, min(int(k), len(sims)))]
    return np.array(order, dtype=np.int64), sims[order]


def min_gap(sims, order) -> float:
    """The smallest distance between neighbours of the expected list (NaN entries and exact ties are not distances: inf / 0)."""
    v = np.asarray(sims, dtype=np.float64)[list(order)]
    v = v[~np.isnan(v)]
    return float(np.min(-np.diff(v))) if len(v) > 1 else math.inf


def f32_order(rows, a) -> list:
    """What fp32 arithmetic (numpy's, on the narrowed store) makes of the order."""
    b = np.asarray(rows, dtype=np.float32).reshape(-1, DIM)
    q = np.asarray(a, dtype=np.float32).reshape(-1)
    sims = np.dot(b, q) / (np.linalg.norm(b, axis=1) * np.linalg.norm(q))
    return rank(sims.astype(np.float64)), sims


# ---- generators -----------------------------------------------------------------------------------------------------------------
def _unit_rows(rng, n) -> np.ndarray:
    g = rng.standard_normal((n, DIM))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def _query_at(rng, base, cosine) -> np.ndarray:
    b = base.astype(np.float64)
    b /= np.linalg.norm(b)
    g = rng.standard_normal(DIM)
    g -= np.dot(g, b) * b
    g /= np.linalg.norm(g)
    return (cosine * b + math.sqrt(1.0 - cosine * cosine) * g).astype(np.float32)


def _nudged(base, q, n_elements, ulps=1) -> np.ndarray:
    """base with its n_elements of largest |q_e| moved `ulps` fp32 ulps towards sign(q_e): the dot with q grows."""
    row = base.copy()
    for e in np.argsort(-np.abs(q), kind="stable")[:n_elements]:
        for _ in range(ulps):
            row[e] = np.nextafter(row[e], np.float32(np.inf) if q[e] > 0 else np.float32(-np.inf))
    return row


@functools.lru_cache(maxsize=None)
def ladder_case(seed: int):
    """(store fp32 (52,1024), query fp32, expected order of all 52 rows, exact sims, ladder rows in expected order).

    Twelve copies of one unit row at cosine ~0.945 to the query; in copy j the j elements with the largest |q_e| are moved by one
    fp32 ulp towards sign(q_e) (two, if one leaves a gap under 8 TOL).  The copies are shuffled behind 40 random unit rows."""
    for ulps in (1, 2):
        rng = np.random.default_rng(1000 + seed)
        base = _unit_rows(rng, 1)[0]
        q = _query_at(rng, base, 0.945)
        rungs = [_nudged(base, q, j, ulps) for j in range(LADDER_RUNGS)]
        place = rng.permutation(LADDER_RUNGS)
        store = np.concatenate([_unit_rows(rng, LADDER_FILL), np.stack([rungs[j] for j in place])]).astype(np.float32)
        sims = exact_sims(store, q, host_query_norm(q))
        order = rank(sims)
        if min_gap(sims, order) >= GAP:
            break
    ladder_rows = order[:LADDER_RUNGS]                           # the rungs, in the exact oracle's order
    assert is_f32_valued(store)
    assert min_gap(sims, order) >= GAP, f"ladder seed {seed}: neighbours closer than 8 TOL"
    assert sorted(ladder_rows) == list(range(LADDER_FILL, LADDER_FILL + LADDER_RUNGS)), f"ladder seed {seed}: the rungs are not the twelve best"
    assert f32_order(store, q)[0][:LADDER_RUNGS] != ladder_rows, f"ladder seed {seed}: fp32 arithmetic reproduces the order"
    assert norm_is_unambiguous(q)
    return store, q, order, sims, ladder_rows


@functools.lru_cache(maxsize=None)
def threshold_case(seed: int):
    """(event matrices [A, B, C] fp32, query fp32, defer flags, per-event exact sims).  The best exact similarity of event A lies
    between 8 TOL and 2e-8 BELOW 0.4, that of its twin B as far ABOVE: one element of the query was bisected in fp32 steps until
    0.4 fell between them.  Both are flagged; C is an unflagged bystander.  Expected: A is deferred, B is ranked."""
    rng = np.random.default_rng(2000 + seed)
    best_a = _unit_rows(rng, 1)[0]
    q = _query_at(rng, best_a, 0.4)
    best_b = _nudged(best_a, q, 6)                               # a twin a few 1e-10 above
    e = int(np.argmax(np.abs(best_a)))                            # the query element that moves the cosine fastest
    start = q[e].copy()
    up = np.float32(np.inf) if best_a[e] > 0 else np.float32(-np.inf)

    def with_steps(m):
        v = q.copy()
        x = start.view(np.int32).copy()
        # fp32 values of one sign are ordered like their bit patterns: m steps towards `up` / away from it
        towards_larger_magnitude = (up > 0) == (start > 0)
        v[e] = np.int32(x + (m if towards_larger_magnitude else -m)).view(np.float32)
        return v

    def sims_of(m):
        v = with_steps(m)
        return exact_sims(np.stack([best_a, best_b]), v, host_query_norm(v))

    lo, hi = -(1 << 16), 1 << 16                                  # sims_of(lo)[0] < 0.4 <= sims_of(hi)[0]
    assert sims_of(lo)[0] < THRESHOLD <= sims_of(hi)[0], f"threshold seed {seed}: 0.4 is not bracketed"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if sims_of(mid)[0] < THRESHOLD:
            lo = mid
        else:
            hi = mid
    chosen = None
    for m in range(lo, lo - 64, -1):                              # walk down until 0.4 lies well inside (sim A, sim B)
        sa, sb = sims_of(m)
        if GAP <= THRESHOLD - sa <= 2e-8 and GAP <= sb - THRESHOLD <= 2e-8:
            if chosen is None or abs((THRESHOLD - sa) - (sb - THRESHOLD)) < chosen[0]:
                chosen = (abs((THRESHOLD - sa) - (sb - THRESHOLD)), m)
    assert chosen is not None, f"threshold seed {seed}: no query step puts 0.4 between the twins with 8 TOL on each side"
    query = with_steps(chosen[1])
    events = [np.concatenate([_unit_rows(rng, 3), best_a[None], _unit_rows(rng, 3)]),
              np.concatenate([_unit_rows(rng, 2), best_b[None], _unit_rows(rng, 4)]),
              _unit_rows(rng, 5)]
    A = host_query_norm(query)
    sims = [exact_sims(ev, query, A) for ev in events]
    assert all(is_f32_valued(ev) for ev in events) and norm_is_unambiguous(query)
    assert rank(sims[0])[0] == 3 and rank(sims[1])[0] == 2
    assert GAP <= THRESHOLD - sims[0][3] <= 2e-8 and GAP <= sims[1][2] - THRESHOLD <= 2e-8
    for s in sims:
        assert min_gap(s, rank(s)) >= GAP
    return events, query, [True, True, False], sims


@functools.lru_cache(maxsize=None)
def random_case(n: int, seed: int = 0, query_dtype: str = "float32"):
    """(store fp32 (n,1024), query, expected order of all rows, exact sims under the HOST norm rule).  Random unit rows; every
    pair of neighbours in the full expected order is at least 8 TOL apart (asserted), so the order is decided within TOL."""
    rng = np.random.default_rng(3000 + 17 * n + seed)
    store = _unit_rows(rng, n)
    q = rng.standard_normal(DIM)
    q = (q / np.linalg.norm(q) * 1.7).astype(np.float32)
    if query_dtype == "float64":                                  # a genuine double: not an fp32 value
        q = q.astype(np.float64) * (1.0 + rng.uniform(-1e-9, 1e-9, DIM))
        assert not is_f32_valued(q)
    parts = exact_parts(store, q)
    sims = sims_from_parts(*parts, host_query_norm(q))
    order = rank(sims)
    assert min_gap(sims, order) >= GAP, f"random case n={n} seed={seed}: neighbours closer than 8 TOL"
    assert norm_is_unambiguous(q)
    _PARTS[n, seed, query_dtype] = parts
    return store, q, order, sims


_PARTS = {}


def random_case_sims(n: int, seed: int, query_dtype: str, A: float) -> np.ndarray:
    """The exact similarities of random_case(n, seed, query_dtype) under another norm A (a device query's), from the same sums."""
    random_case(n, seed, query_dtype)
    return sims_from_parts(*_PARTS[n, seed, query_dtype], A)


# ---- the reference's rules after the scan, on doubles ---------------------------------------------------------------------------
def model_hits(idx, sims, counts, keep, row_limits=None, defer=None, min_similarity=THRESHOLD):
    """(hits, deferred event numbers) of relevant_hits(exact64=True) from planted (E, k) hits.  tests/relevant_hits_model.py ranks;
    the deferral is decided on DOUBLES here (that model narrows to fp32, which is the default route's rule): a deferred event
    enters the model with a row limit of 0, so none of its hits is a candidate."""
    import relevant_hits_model as model
    E = idx.shape[0]
    deferred = [e for e in range(E) if defer is not None and defer[e] and counts[e] > 0 and sims[e, 0] < float(min_similarity)]
    limits = [int(1 << 40) if row_limits is None else int(row_limits[e]) for e in range(E)]
    for e in deferred:
        limits[e] = 0
    per_event = [(idx[e, :counts[e]], sims[e, :counts[e]]) for e in range(E)]
    return model.relevant_hits(per_event, keep, limits, None)[0], deferred
