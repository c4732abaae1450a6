"""Shared by the key-frame relation tests (plain helper module, not a fixture plugin): inputs whose similarity relation is
planted -- far tile pairs, columns beyond bitmap word 64, non-transitive triples and paths, a (kept tiles x new tiles) grid,
threshold and NaN-row edges -- with the planted relation and the kept list in closed form, the numpy model of both routes
driven by a relation matrix, and the named mutants of that model that the clustered inputs of the older tests cannot tell
from the real thing.

Every builder returns (features fp32 (n,1024), threshold, planted relation bool (n,n) with its diagonal, expected kept list).
The relation is "not (cosine < threshold)" as the kernels evaluate it: a NaN cosine (zero row) or a NaN threshold is a hit."""
from __future__ import annotations

import functools

import numpy as np

import keyframe_stream_cases as K

D = 1024
TILE = 64                      # gram tile edge (gram_core.h kGT)
SCALES = (0.5, 2.0, 4.0)       # powers of two: a scaled copy normalises to its original's bits
MARGIN = 0.05                  # every finite off-diagonal cosine lies at least this far from its case's threshold


def _rows(n: int, seed: int):
    rng = np.random.default_rng(seed)
    return rng, rng.standard_normal((n, D)).astype(np.float32)


def _relation_of_pairs(n: int, pairs) -> np.ndarray:
    rel = np.eye(n, dtype=bool)
    for i, j in pairs:
        rel[i, j] = rel[j, i] = True
    return rel


# ---- builders ----------------------------------------------------------------------------------------------------------------
EXPLICIT_2113 = ((0, 2112), (5, 2050), (31, 2079), (63, 2048), (100, 2100), (2047, 2111))


def matching_pairs(n: int, seed: int, explicit=()):
    """(rows, pairs): the explicit pairs, then a random permutation of the other rows whose first n/2 entries are paired off
    as (i, j), i < j.  No row is in two pairs."""
    rng, f = _rows(n, seed)
    taken = {r for pair in explicit for r in pair}
    free = np.array([r for r in range(n) if r not in taken])
    perm = rng.permutation(free)[: n // 2].tolist()
    pairs = [tuple(p) for p in explicit] + [(min(a, b), max(a, b)) for a, b in zip(perm[0::2], perm[1::2])]
    return f, pairs


def matching(n: int, seed: int, explicit=()):
    """A perfect matching on half the rows: f[j] = f[i] * s.  Each planted hit decides one kept index by itself (j is dropped
    by i alone) and every spurious bit drops a row, wherever the two rows' tiles and bitmap words lie."""
    f, pairs = matching_pairs(n, seed, explicit)
    for k, (i, j) in enumerate(pairs):
        f[j] = f[i] * np.float32(SCALES[k % len(SCALES)])
    dropped = {j for _, j in pairs}
    return f, 0.9, _relation_of_pairs(n, pairs), [r for r in range(n) if r not in dropped]


NT_TRIPLES = ((10, 140, 75), (80, 150, 20), (30, 100, 170))      # (a, c, m): a < m < c, m first, m last
NT_PATH = (5, 66, 129, 190, 64)                                  # rows of path nodes 0..4; consecutive nodes are adjacent
NT_DROPPED = (66, 75, 80, 150, 170, 190)


def non_transitive():
    """n = 200, threshold 0.6.  Midpoint triples: m = normalise(u_a + u_c) * 3 has cosine ~0.707 with a and with c, which are
    unrelated to each other; a 5-node path in one plane at 40 degree steps (cos 40 = 0.766, cos 80 = 0.174).  Only kept rows
    block: in a < m < c the dropped m must not take c with it; on the path the dropped node 1 (row 66) must not block node 2
    (row 129), which in turn blocks node 3 (row 190); node 4 (row 64) comes before its only neighbour."""
    n = 200
    rng, f = _rows(n, 200)
    pairs = []
    for a, c, m in NT_TRIPLES:
        ua, uc = (f[r].astype(np.float64) / np.linalg.norm(f[r].astype(np.float64)) for r in (a, c))
        mid = ua + uc
        f[m] = (mid / np.linalg.norm(mid) * 3.0).astype(np.float32)
        pairs += [(a, m), (c, m)]
    e1, e2 = rng.standard_normal(D), rng.standard_normal(D)
    e1 /= np.linalg.norm(e1)
    e2 -= e2.dot(e1) * e1
    e2 /= np.linalg.norm(e2)
    for node, row in enumerate(NT_PATH):
        angle = np.deg2rad(40.0 * node)
        f[row] = ((np.cos(angle) * e1 + np.sin(angle) * e2) * (1.0 + 0.5 * node)).astype(np.float32)
    pairs += list(zip(NT_PATH[:-1], NT_PATH[1:]))
    return f, 0.6, _relation_of_pairs(n, pairs), [r for r in range(n) if r not in NT_DROPPED]


GRID_KEPT, GRID_NEW = 260, 130                  # five kept tiles (the last holds 4 rows), three new tiles (the last holds 2)
GRID_LAST = {"a": (0, 4), "b": (1, 3), "c": (2, 2)}
_EDGE_POS = (0, 31, 32, 63)                     # first / last bit of either word of a tile row


def kept_grid_pairs(last: str):
    """[(kept row, new row)] of the growing-route grid, new rows as global indices.  The two full new tiles take one copy from
    each of the five kept tiles; original and copy sit at positions 0, 31, 32, 63 of their tiles where the tile has them (the
    4-row kept tile offers its first row and its last, the row a partial tile's padding is read from).  A new row can copy one
    kept row only, so the 2-row new tile has room for two independent hits: the variants a, b, c give them to the kept tiles
    (0, 4), (1, 3), (2, 2), and between them every cell of the 5 x 3 grid decides a row on its own."""
    new_pos = _EDGE_POS + (47,)
    pairs = []
    for nt in range(2):
        for kt in range(5):
            kp = _EDGE_POS[(kt + nt) % 4] if kt < 4 else (0, GRID_KEPT - 4 * TILE - 1)[nt]
            pairs.append((kt * TILE + kp, GRID_KEPT + nt * TILE + new_pos[(kt + 2 * nt) % 5]))
    for slot, kt in enumerate(GRID_LAST[last]):
        kp = _EDGE_POS[(kt + 2 + slot) % 4] if kt < 4 else 2          # a kept row the full tiles have not copied
        pairs.append((kt * TILE + kp, GRID_KEPT + 2 * TILE + slot))
    return pairs


GRID_NEW_PAIRS = ((GRID_KEPT + 5, GRID_KEPT + TILE + 10), (GRID_KEPT + 40, GRID_KEPT + 2 * TILE - 2))   # fresh row -> later new tile


def kept_grid(last: str = "a"):
    """Growing route: 260 unrelated rows are all kept, then ONE batch of 130 rows in which the chosen rows are scaled copies of
    kept rows (one hit per (kept tile, new tile) cell), two more are copies of fresh rows of an earlier new tile, and the rest
    are fresh.  The copies are dropped, the fresh rows kept."""
    n = GRID_KEPT + GRID_NEW
    _, f = _rows(n, 390)
    pairs = kept_grid_pairs(last) + list(GRID_NEW_PAIRS)
    for k, (i, j) in enumerate(pairs):
        f[j] = f[i] * np.float32(SCALES[k % len(SCALES)])
    dropped = {j for _, j in pairs}
    return f, 0.9, _relation_of_pairs(n, pairs), [r for r in range(n) if r not in dropped]


EDGE_THRESHOLDS = (-1.5, 1.5, float("inf"), float("nan"), 0.9)      # 0.9: the ordinary rule on the same rows, for contrast
EDGE_DUP = (127, 128)                                               # an exact duplicate pair across the edge of tiles 1 | 2
EDGE_NAN_ROWS = (64, 129)                                           # first row of a tile; last row of the partial tile


def threshold_edges(thr: float, nan_rows: bool = False):
    """n = 130.  The rule is `similarity < thr` keeps (hippocampal_memory.py:960): under NaN and -1.5 nothing is below the
    threshold, every pair is a hit and only row 0 survives; under 1.5 and +inf everything is below it, the diagonal included,
    and every row is kept, the duplicate too.  A zero row has NaN similarity with every row: it is never kept (row 0 blocks
    it) and, never kept, blocks nobody."""
    n = 130
    _, f = _rows(n, 130)
    f[EDGE_DUP[1]] = f[EDGE_DUP[0]]
    cosine = _relation_of_pairs(n, [EDGE_DUP]).astype(np.float64)       # 1 on the diagonal and the pair, ~0 elsewhere
    with np.errstate(invalid="ignore"):
        rel = ~(cosine < thr)
    if nan_rows:
        f[list(EDGE_NAN_ROWS)] = 0.0
        rel[list(EDGE_NAN_ROWS), :] = True
        rel[:, list(EDGE_NAN_ROWS)] = True
    if np.isnan(thr) or thr <= -1.0:
        kept = [0]
    else:
        gone = set(EDGE_NAN_ROWS if nan_rows else ()) | ({EDGE_DUP[1]} if thr <= 1.0 else set())
        kept = [r for r in range(n) if r not in gone]
    return f, thr, rel, kept


def _edge_name(thr: float, nan_rows: bool) -> str:
    return f"edges_thr_{thr}" + ("_nan_rows" if nan_rows else "")


BUILDERS = {
    "matching_n320": functools.partial(matching, 320, 320),
    "matching_n2113": functools.partial(matching, 2113, 2113, EXPLICIT_2113),
    "non_transitive": non_transitive,
    **{f"kept_grid_{v}": functools.partial(kept_grid, v) for v in GRID_LAST},
    **{_edge_name(t, z): functools.partial(threshold_edges, t, z) for z in (False, True) for t in EDGE_THRESHOLDS},
}
CASES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(features, threshold, planted relation, expected kept), built once; callers leave the arrays unchanged."""
    f, thr, rel, kept = BUILDERS[name]()
    rel.setflags(write=False)
    return f, thr, rel, kept


def partitions(name: str, n: int) -> dict:
    """The batch partitions of the growing route: everything at once, K.CYCLE, 64s and 100s; the kept grid's 260 rows under
    K.CYCLE and its 130 new rows as the one batch the case is about; the 2113-row input at once and in 450s."""
    if name.startswith("kept_grid"):
        return {"cycle+130": K.batches(GRID_KEPT, K.CYCLE) + [(GRID_KEPT, n)]}
    if name == "matching_n2113":
        return {"all": K.batches(n, [n]), "450": K.batches(n, [450])}
    return {"all": K.batches(n, [n]), "cycle": K.batches(n, K.CYCLE), "64": K.batches(n, [64]), "100": K.batches(n, [100])}


# ---- numpy model, driven by a relation matrix --------------------------------------------------------------------------------
def cosines(f: np.ndarray) -> np.ndarray:
    """float64 cosines of the fp32-normalised rows (the kernels' operands), before the one rounding to fp32."""
    u = K._unit(np.asarray(f, dtype=np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return u @ u.T


def relation(f: np.ndarray, thr: float) -> np.ndarray:
    """What gram_bits_kernel holds for the whole input: K._hits on the normalised rows, each unordered pair evaluated once."""
    u = K._unit(np.asarray(f, dtype=np.float32))
    hits = K._hits(u, u, np.float32(thr))
    return np.triu(hits) | np.triu(hits).T


@functools.lru_cache(maxsize=None)
def case_model(name: str):
    """(float64 cosines, modelled relation) of a case: one matmul, shared by every test that needs either."""
    f, thr, _, _ = case(name)
    cos = cosines(f)
    with np.errstate(invalid="ignore"):
        hits = ~(cos.astype(np.float32) < np.float32(thr))
    rel = np.triu(hits) | np.triu(hits).T
    rel.setflags(write=False)
    return cos, rel


MUTANTS = {
    "far_tiles": "a: gram_bits_kernel drops every hit between rows whose tiles are two or more apart",
    "word64": "b: the scans lose the second trip of `for (w = (i >> 5) + lane; w < W; w += 64)`: a kept row no longer blocks "
              "columns 64 or more bitmap words past its own word (rows below 2048 lose hits in columns from 2048 on)",
    "dropped_block": "c: a dropped row is OR-ed into blocked[] as well",
    "last_kept_tile": "d: the growing route compares new rows with the last kept tile only",
    "diag_tile_only": "e: the growing route ignores new x new hits outside the diagonal tiles",
}


def _mutated(adj: np.ndarray, mutant) -> np.ndarray:
    """The relation of one launch of gram_bits_kernel + scan (indices local to that launch) under a mutant."""
    if mutant not in ("far_tiles", "word64", "diag_tile_only"):
        return adj
    adj = adj.copy()
    idx = np.arange(adj.shape[0])
    tile = idx // TILE
    if mutant == "far_tiles":
        adj[np.abs(tile[:, None] - tile[None, :]) >= 2] = False
    elif mutant == "word64":
        adj[(idx[None, :] >> 5) - (idx[:, None] >> 5) >= 64] = False
    else:
        adj[tile[:, None] != tile[None, :]] = False
    return adj


def _scan(adj: np.ndarray, blocked: np.ndarray, first_is_global_zero: bool, mutant) -> list:
    """The ordered scan of both greedy kernels: keep row i iff it is global row 0 or not blocked; a kept row blocks."""
    kept = []
    for i in range(adj.shape[0]):
        if (first_is_global_zero and i == 0) or not blocked[i]:
            kept.append(i)
            blocked |= adj[i]
        elif mutant == "dropped_block":
            blocked |= adj[i]
    return kept


def one_shot(rel: np.ndarray, mutant=None) -> list:
    """hmm_gram_select on a relation matrix."""
    n = rel.shape[0]
    if n <= 2:
        return list(range(n))
    return _scan(_mutated(rel, None if mutant == "diag_tile_only" else mutant), np.zeros(n, bool), True, mutant)


def grown(rel: np.ndarray, part, mutant=None, after_each=None) -> list:
    """hmm_keyframe_extend batch by batch on a relation matrix (K.ModelSelector's steps 2-5 with the dots looked up);
    after_each(n_seen, kept list) is called after every batch."""
    kept = []
    for a, b in part:
        against = kept[(len(kept) - 1) // TILE * TILE:] if mutant == "last_kept_tile" else kept
        blocked = rel[a:b][:, against].any(axis=1) if against else np.zeros(b - a, bool)
        kept += [a + i for i in _scan(_mutated(rel[a:b, a:b], mutant), blocked, a == 0, mutant)]
        if after_each is not None:
            after_each(b, list(range(b)) if b <= 2 else list(kept))
    n = rel.shape[0]
    return list(range(n)) if n <= 2 else kept


def tile_pairs_hit(rel: np.ndarray) -> set:
    """{(ti, tj), ti <= tj} of the tile pairs that hold an off-diagonal hit."""
    i, j = np.nonzero(np.triu(rel, 1))
    return set(zip((i // TILE).tolist(), (j // TILE).tolist()))


def cosine_stats(name: str):
    """(weakest planted, strongest unplanted) finite off-diagonal cosine of a case; None where a side has no finite pair."""
    _, _, rel, _ = case(name)
    cos, _ = case_model(name)
    off = ~np.eye(rel.shape[0], dtype=bool) & np.isfinite(cos)
    hit, miss = cos[off & rel], cos[off & ~rel]
    return (float(hit.min()) if hit.size else None), (float(miss.max()) if miss.size else None)
