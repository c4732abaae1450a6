"""Adversarial row layouts for the float64 route's OWN selection pipeline (hippomm_amd/csrc/cosine_topk_f64.hip): a store recipe
whose exact similarities come in closed form, the launch plan and the selection restated in Python, the layouts and the case
tables.  Shared by tests/test_cpu_exact64_layouts.py (which proves without a GPU that every case is what it claims to be) and
tests/test_gpu_exact64_layouts.py.  numpy only.

THE RECIPE.  Row i holds two non-zero fp32 elements, xc_i at column c_i and xd_i at column d_i; the query is a dense fp32 vector
(eight "hot" columns of magnitude 0.33, four columns of 0, every other column +-0.01).  D = xc q_c + xd q_d and S = xc^2 + xd^2 are
then two exact products and ONE rounding each, in whatever order they are summed: the route's chains and butterfly only ever add
zeros to them.  With the norm A handed in (a host query), the kernel's similarity must therefore EQUAL

    (xc*qc + xd*qd) / (np.sqrt(xc*xc + xd*xd) * A)          evaluated in numpy float64, bit for bit.

``closed_form`` is that line; a full ranking of a million rows is one np.lexsort.  Only the four per-row arrays live on the host:
the GPU file scatters them into zeros on the device.

Planted relations, in units of r = |xd| / |xc| with xc = +-0.5 on a hot column (the sign is the query's, so the product is
positive): "level" j is r_j = 0.05 + j * LEVEL_STEP, similarity about 0.35 / sqrt(1 + r^2), strictly falling in j; rows of one
level are exact ties (identical products, identical squares).  Background rows draw r from [1.5, 6]: below every level up to
r = 0.95.  A NaN row is all zero.  A row of similarity exactly +0.0 has xc = +0.0 and its other element on a column where the
query is 0.  Every generator ASSERTS what the tests rely on (``Store.check``): fp32 values, intended ties bit-equal, every other
pair of neighbours in the full order at least ``exact64_cases.GAP`` apart; background rows that collide are drawn again.

Columns: c_i walks the hot columns and d_i every other column, so a store with background covers all 1024 columns -- every lane,
j and c of the fixed ownership carries a non-zero somewhere (asserted by the CPU file).  The four order stores without
background (identical rows, zeros, ascending, descending) cannot: tied rows need equal products, which a column of the query's
zeros cannot give; they cover what their relation allows and the CPU file says how much.

THE PLAN MODEL.  Every constant, the 256 / 1024 rule of argmax_threads, the held rule and the grid rules are read out of the
source (``source_constants``); ``flat_plan`` / ``segment_plan`` restate which path a call takes, its slices and the threads of each
level.  ``model_flat`` / ``model_segment`` restate the selection with the kernel's structure (a first level per slice, a second
level over the G k candidates, the LDS path as "keep the best 1024, merge the next 1024", the full sort over n_pad padded pairs)
under the key order (NaN first, similarity descending, -0 == +0, higher position first).  ``MUTANTS`` names the mistakes the
case table must be able to see.

ONE BRANCH IS OUT OF REACH and left out on purpose: the re-read arg-max with 1024 threads.  It needs a first-level slice above
16 * 1024 = 16,384 rows under the cap of 256 groups, that is more than 4.19 M rows, a store of 16 GiB."""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import exact64_cases as cases

CSRC = Path(__file__).resolve().parent.parent / "hippomm_amd" / "csrc"
SOURCE = "cosine_topk_f64.hip"
DIM = cases.DIM
TOL, GAP = cases.TOL, cases.GAP
NOPOS = 0xFFFFFFFF

HOT = (0, 255, 256, 257, 511, 512, 768, 1023)
ZERO_COLS = (2, 300, 700, 1021)
HOT_MAG, COLD_MAG = np.float32(0.33), np.float32(0.01)
_NONHOT = np.array([c for c in range(DIM) if c not in HOT], dtype=np.int64)
_COLD = np.array([c for c in _NONHOT if c not in ZERO_COLS], dtype=np.int64)
_HOT = np.array(HOT, dtype=np.int64)
_ZERO = np.array(ZERO_COLS, dtype=np.int64)

LEVEL_STEP = 0.9 / 1100            # levels 0 .. 1100 lie in r = 0.05 .. 0.95
MAX_LEVEL = 1100
EPS = np.float32(2.0 ** -20)


# ---- constants and rules out of the source ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def source_constants() -> dict:
    text = (CSRC / SOURCE).read_text()
    c = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+(kF64\w+)\s*=\s*(\d+)\s*;", text)}
    for name in ("kF64ArgmaxK", "kF64MaxK", "kF64Slice", "kF64MaxGroups", "kF64MaxGroupsSort", "kF64Held"):
        assert name in c, f"{name} is no longer a constexpr int of {SOURCE}"
    c["kNumCU"] = int(re.search(r"constexpr\s+int\s+kNumCU\s*=\s*(\d+)\s*;", (CSRC / "hmm_common.h").read_text()).group(1))
    m = re.search(r"constexpr\s+int\s+kScanBlocks\s*=\s*kNumCU\s*\*\s*(\d+)\s*;", (CSRC / "cosine_topk_shared.h").read_text())
    c["kScanBlocks"] = c["kNumCU"] * int(m.group(1))
    # argmax_threads: 256 while the range fits the registers of 256 threads, 1024 beyond
    m = re.search(r"argmax_threads\(int64_t n\)\s*\{\s*return n <= (\d+) \* kF64Held \? (\d+)u : (\d+)u;", text)
    assert m and m.group(1) == m.group(2), "argmax_threads changed its form"
    c["argmax_small"], c["argmax_large"] = int(m.group(2)), int(m.group(3))
    # the held rule of the arg-max rounds, and the chunk of the LDS path (2048 pairs sorted: the kept 1024 and the next 1024)
    assert re.search(r"held = in\.n <= \(uint32_t\)kF64Held \* blockDim\.x;", text), "the held rule changed its form"
    m = re.search(r"for \(uint32_t c0 = 0; c0 < in\.n; c0 \+= (\d+)\)", text)
    c["lds_chunk"] = int(m.group(1))
    assert re.search(r"lds_bitonic_desc_(\d+)", text).group(1) == str(2 * c["lds_chunk"])
    # scan_grid_f64: ceil(ceil(n / 2) / 4) workgroups, capped at kNumCU * 3 / 2
    m = re.search(r"blocks = \(\(n \+ 1\) / 2 \+ 3\) / 4;\s*const int64_t cap = kNumCU \* (\d+) / (\d+);", text)
    c["scan_cap"] = c["kNumCU"] * int(m.group(1)) // int(m.group(2))
    # flat_plan's own lines: the model below restates them
    for line in (r"p\.k_eff = \(int\)\(k < n \? k : n\);", r"p\.global_sort = p\.k_eff > kF64MaxK;",
                 r"by_slice = \(n \+ kF64Slice - 1\) / kF64Slice;",
                 r"cap = p\.k_eff <= kF64ArgmaxK \? kF64MaxGroups : kF64MaxGroupsSort;",
                 r"p\.n_pad = p\.global_sort \? next_pow2_i64\(n\) : 0;", r"\} else if \(p\.k_eff <= kF64ArgmaxK\) \{",
                 r"per = \(n_rows \+ gridDim\.x - 1\) / gridDim\.x;", r"if \(k <= kF64ArgmaxK\)\s*launch_select<false, true>\(grid, 256,"):
        assert re.search(line, text), f"{SOURCE}: `{line}` is gone; flat_plan / the dispatch changed its form"
    # the eligibility kernel's grid: 16 values per thread of 256, capped at kScanBlocks
    m = re.search(r"blocks = \(n_values \+ (\d+) \* (\d+) - 1\) / \(\1 \* \2\);", text)
    c["elig_threads"], c["elig_per_thread"] = int(m.group(1)), int(m.group(2))
    assert re.search(r"blocks > kScanBlocks \? kScanBlocks : blocks", text)
    return c


def scan_grid(n: int) -> int:
    c = source_constants()
    return max(1, min(((n + 1) // 2 + 3) // 4, c["scan_cap"]))


def eligibility_grid(n_values: int) -> int:
    c = source_constants()
    per_block = c["elig_threads"] * c["elig_per_thread"]
    return min((n_values + per_block - 1) // per_block, c["kScanBlocks"])


def argmax_threads(n: int) -> int:
    c = source_constants()
    return c["argmax_small"] if n <= c["argmax_small"] * c["kF64Held"] else c["argmax_large"]


MUTANTS = (
    "tie rule reversed in the second level",
    "tie rule reversed between LDS chunks",
    "first level keeps k - 1",
    "per by floor",
    "register slot kF64Held - 1 not loaded",
    "chunk offset 1023 dropped in a merge",
    "padding counted as a hit in the full sort",
    "NaN ranked last",
    "arg-max dispatch limit off by one",
    "1024 limit off by one",
)


@dataclass(frozen=True)
class Plan:
    n: int
    k: int
    k_eff: int
    path: str                   # "argmax" | "lds" | "sort"
    groups: int
    per: int
    n_pad: int
    threads1: int
    held1: bool
    cand: int
    threads2: int
    held2: bool
    scan_blocks: int

    def slices(self) -> List[Tuple[int, int]]:
        out = []
        for g in range(self.groups):
            lo = min(g * self.per, self.n)
            out.append((lo, min(lo + self.per, self.n)))
        return out

    def branch(self) -> str:
        if self.path == "sort":
            return f"full sort, n_pad={self.n_pad} ({self.n_pad - self.n} pads), 256 threads per step"
        hold = lambda h: "held" if h else "re-read"
        if self.path == "argmax":
            return (f"arg-max, G={self.groups} per={self.per}, level 1: {self.threads1} threads {hold(self.held1)}, "
                    f"level 2: {self.cand} candidates, {self.threads2} threads {hold(self.held2)}")
        chunks = lambda n: (n + 1023) // 1024
        return (f"LDS chunks, G={self.groups} per={self.per} ({chunks(self.per)} chunks), level 1: 1024 threads, "
                f"level 2: {self.cand} candidates ({chunks(self.cand)} chunks), 1024 threads")


def _limits(mutant: Optional[str]):
    c = source_constants()
    argmax_k = c["kF64ArgmaxK"] + (1 if mutant == "arg-max dispatch limit off by one" else 0)
    max_k = c["kF64MaxK"] + (1 if mutant == "1024 limit off by one" else 0)
    return c, argmax_k, max_k


def flat_plan(n: int, k: int, mutant: Optional[str] = None) -> Plan:
    """flat_plan and the launches of hmm_cosine_topk_f64, restated."""
    c, argmax_k, max_k = _limits(mutant)
    k_eff = min(k, n)
    by_slice = (n + c["kF64Slice"] - 1) // c["kF64Slice"]
    cap = c["kF64MaxGroups"] if k_eff <= argmax_k else c["kF64MaxGroupsSort"]
    groups = max(1, min(by_slice, cap))
    per = n // groups if mutant == "per by floor" else (n + groups - 1) // groups
    if k_eff > max_k:
        n_pad = 1
        while n_pad < n:
            n_pad <<= 1
        return Plan(n, k, k_eff, "sort", 0, 0, n_pad, 256, False, 0, 256, False, scan_grid(n))
    cand = groups * k_eff
    if k_eff <= argmax_k:
        t1, t2 = argmax_threads(per), argmax_threads(cand)
        return Plan(n, k, k_eff, "argmax", groups, per, 0, t1, per <= c["kF64Held"] * t1, cand, t2, cand <= c["kF64Held"] * t2,
                    scan_grid(n))
    return Plan(n, k, k_eff, "lds", groups, per, 0, 1024, False, cand, 1024, False, scan_grid(n))


def segment_plan(n_e: int, k: int, mutant: Optional[str] = None) -> Tuple[str, int, bool]:
    """(path, threads, held) of one event's workgroup in hmm_cosine_topk_segmented_f64."""
    c, argmax_k, _ = _limits(mutant)
    if k <= argmax_k:
        return "argmax", c["argmax_small"], n_e <= c["kF64Held"] * c["argmax_small"]
    return "lds", 1024, False


# ---- keys and the selection model -------------------------------------------------------------------------------------------------
def order_keys(sims, nan_last: bool = False) -> np.ndarray:
    """order_bits64 on an array: a monotone double -> uint64 map, -0.0 == +0.0, NaN -> all ones.  Key 0 belongs to no double."""
    s = np.asarray(sims, dtype=np.float64) + 0.0
    b = s.view(np.uint64)
    key = np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))
    key[np.isnan(s)] = np.uint64(1) if nan_last else ~np.uint64(0)
    return key


def rank_fast(sims) -> np.ndarray:
    """``exact64_cases.rank`` as one np.lexsort: NaN first, similarity descending, -0 == +0, higher index first."""
    keys = order_keys(sims)
    return np.lexsort((np.arange(len(keys)), keys))[::-1].astype(np.int64)


def _best(keys, pos, k, tie_low=False):
    """The k best valid (key != 0) pairs, best first; ties by higher position (by LOWER position under ``tie_low``)."""
    valid = keys != 0
    keys, pos = keys[valid], pos[valid]
    second = (np.int64(NOPOS) - pos.astype(np.int64)) if tie_low else pos.astype(np.int64)
    o = np.lexsort((second, keys))[::-1][:max(k, 0)]
    return keys[o], pos[o]


def _padded(keys, pos, k):
    out_k, out_p = np.zeros(k, np.uint64), np.full(k, NOPOS, np.uint64)
    out_k[:len(keys)], out_p[:len(pos)] = keys, pos
    return out_k, out_p


def _argmax_level(keys, pos, k, threads, mutant, tie_low=False):
    c = source_constants()
    held = len(keys) <= c["kF64Held"] * threads
    if held and mutant == "register slot kF64Held - 1 not loaded":
        keys = keys.copy()
        keys[(c["kF64Held"] - 1) * threads:] = 0          # thread t holds elements t + j * threads: slot j = i // threads
    return _best(keys, pos, k, tie_low)


def _lds_level(keys, pos, k, mutant, tie_low=False):
    """Keep the best 1024, merge the next 1024; the first k of what is left."""
    chunk = source_constants()["lds_chunk"]
    kept_k, kept_p = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    for c0 in range(0, len(keys), chunk):
        ck, cp = keys[c0:c0 + chunk].copy(), pos[c0:c0 + chunk]
        if mutant == "chunk offset 1023 dropped in a merge" and len(ck) == chunk:
            ck[chunk - 1] = 0
        both_k, both_p = np.concatenate([kept_k, ck]), np.concatenate([kept_p, cp])
        if mutant == "tie rule reversed between LDS chunks":
            both_k, both_p = _best(both_k, both_p, chunk, tie_low=True)      # who survives the cut; their order is the right one
        kept_k, kept_p = _best(both_k, both_p, chunk, tie_low)
    return kept_k[:k], kept_p[:k]


def model_flat(sims, k: int, mutant: Optional[str] = None) -> np.ndarray:
    """The int64 indices hmm_cosine_topk_f64 returns for the doubles ``sims``, by the kernel's own structure.  Under a mutant the
    list may be shorter than min(k, n) or hold NOPOS (a pad that was emitted)."""
    assert mutant is None or mutant in MUTANTS, mutant
    sims = np.asarray(sims, dtype=np.float64)
    n = len(sims)
    p = flat_plan(n, k, mutant)
    keys = order_keys(sims, nan_last=mutant == "NaN ranked last")
    pos = np.arange(n, dtype=np.uint64)
    if p.path == "sort":
        pad_key = order_keys(np.zeros(1))[0] if mutant == "padding counted as a hit in the full sort" else np.uint64(0)
        all_k = np.concatenate([keys, np.full(p.n_pad - n, pad_key, np.uint64)])
        all_p = np.concatenate([pos, np.full(p.n_pad - n, NOPOS, np.uint64)])
        o = np.lexsort((all_p, all_k))[::-1][:p.k_eff]
        return all_p[o].astype(np.int64)
    k1 = p.k_eff - 1 if mutant == "first level keeps k - 1" else p.k_eff
    cand_k, cand_p = [], []
    for lo, hi in p.slices():
        if p.path == "argmax":
            sk, sp = _argmax_level(keys[lo:hi], pos[lo:hi], k1, p.threads1, mutant)
        else:
            sk, sp = _lds_level(keys[lo:hi], pos[lo:hi], k1, mutant)
        sk, sp = _padded(sk, sp, p.k_eff)
        cand_k.append(sk)
        cand_p.append(sp)
    cand_k, cand_p = np.concatenate(cand_k), np.concatenate(cand_p)
    tie_low = mutant == "tie rule reversed in the second level"
    if p.path == "argmax":
        out = _argmax_level(cand_k, cand_p, p.k_eff, p.threads2, mutant, tie_low)[1]
    else:
        out = _lds_level(cand_k, cand_p, p.k_eff, mutant, tie_low)[1]
    return out.astype(np.int64)


def model_segment(sims, k: int, mutant: Optional[str] = None) -> np.ndarray:
    """One event's slot of hmm_cosine_topk_segmented_f64: positions within the event, best first, min(k, n_e) of them."""
    sims = np.asarray(sims, dtype=np.float64)
    keys = order_keys(sims, nan_last=mutant == "NaN ranked last")
    pos = np.arange(len(sims), dtype=np.uint64)
    path, threads, _ = segment_plan(len(sims), k, mutant)
    if path == "argmax":
        return _argmax_level(keys, pos, k, threads, mutant)[1].astype(np.int64)
    return _lds_level(keys, pos, k, mutant)[1].astype(np.int64)


def clamped_segments(offsets: Sequence[int], n_rows: int) -> List[Tuple[int, int]]:
    """The header's clamping rule for a per-event offsets table: lo into [0, n_rows], hi into [lo, n_rows]."""
    out = []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        lo = min(max(int(lo), 0), n_rows)
        out.append((lo, min(max(int(hi), lo), n_rows)))
    return out


# ---- the query ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query(kind: str = "float32") -> np.ndarray:
    """The one query of every case.  "float32"; "float64": the same values widened (fp32-valued); "double": a genuine double."""
    rng = np.random.default_rng(64)
    q = (COLD_MAG * rng.choice([-1.0, 1.0], DIM)).astype(np.float32)
    q[_HOT] = HOT_MAG * np.array([1, -1, 1, -1, -1, 1, -1, 1], dtype=np.float32)
    q[_ZERO] = 0.0
    assert cases.norm_is_unambiguous(q)
    if kind == "float32":
        return q
    if kind == "float64":
        return q.astype(np.float64)
    assert kind == "double"
    q64 = q.astype(np.float64) * (1.0 + rng.uniform(-1e-9, 1e-9, DIM))
    assert not cases.is_f32_valued(q64)
    return q64


# ---- the store ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Store:
    label: str
    xc: np.ndarray              # float32[n]
    xd: np.ndarray              # float32[n]
    c: np.ndarray               # int64[n]
    d: np.ndarray               # int64[n]
    tie: np.ndarray             # int32[n]: the tie group of a row, -1 for none
    background: bool

    @property
    def n(self) -> int:
        return len(self.xc)

    def closed_form(self, q=None, A: Optional[float] = None) -> np.ndarray:
        q = query() if q is None else np.asarray(q)
        A = cases.host_query_norm(q) if A is None else A
        xc, xd = self.xc.astype(np.float64), self.xd.astype(np.float64)
        qc, qd = q[self.c].astype(np.float64), q[self.d].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (xc * qc + xd * qd) / (np.sqrt(xc * xc + xd * xd) * np.float64(A))

    def dense(self, rows) -> np.ndarray:
        rows = np.asarray(rows, dtype=np.int64)
        out = np.zeros((len(rows), DIM), np.float32)
        out[np.arange(len(rows)), self.c[rows]] = self.xc[rows]
        out[np.arange(len(rows)), self.d[rows]] = self.xd[rows]
        return out

    def nan_rows(self) -> np.ndarray:
        return np.flatnonzero((self.xc == 0) & (self.xd == 0))

    def violations(self, sims=None) -> np.ndarray:
        """Rows next to a neighbour of the full order that is closer than GAP without being an intended tie."""
        sims = self.closed_form() if sims is None else sims
        order = rank_fast(sims)
        order = order[~np.isnan(sims[order])]
        v = sims[order]
        gap = -np.diff(v)
        same = (self.tie[order[:-1]] >= 0) & (self.tie[order[:-1]] == self.tie[order[1:]])
        bad = (gap < GAP) & ~(same & (gap == 0))
        return np.unique(np.concatenate([order[:-1][bad], order[1:][bad]]))

    def check(self) -> "Store":
        """The generators' conditions; an input that does not meet them is an error."""
        assert self.xc.dtype == np.float32 and self.xd.dtype == np.float32            # the rows are fp32 values
        assert (self.c != self.d).all() and self.c.min() >= 0 and self.d.min() >= 0 and max(self.c.max(), self.d.max()) < DIM
        sims = self.closed_form()
        assert len(self.violations(sims)) == 0, f"{self.label}: neighbours closer than GAP that are no intended tie"
        bits = sims.view(np.uint64)
        for g in np.unique(self.tie[self.tie >= 0]):                                    # intended ties are bit-equal
            assert len(set(bits[self.tie == g].tolist())) == 1, f"{self.label}: tie group {g} is not bit-equal"
        assert np.isnan(sims).sum() == len(self.nan_rows())
        return self


class _Builder:
    def __init__(self, n: int, label: str, seed: int, background: bool = True):
        self.n, self.label, self.background = n, label, background
        self.rng = np.random.default_rng(6400 + seed)
        i = np.arange(n)
        self.q = query()
        self.c = _HOT[i % len(_HOT)].copy()
        self.d = _NONHOT[(i + i // len(_NONHOT)) % len(_NONHOT)].copy()
        self.xc, self.xd = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.tie = np.full(n, -1, np.int32)
        self.special = np.zeros(n, bool)
        self.groups = 0
        if background:
            self._draw(i)

    def _draw(self, rows):
        m = len(rows)
        a = self.rng.uniform(0.05, 0.5, m) * self.rng.choice([-1.0, 1.0], m)
        self.xc[rows] = a.astype(np.float32)
        self.xd[rows] = (np.abs(a) * self.rng.uniform(1.5, 6.0, m) * self.rng.choice([-1.0, 1.0], m)).astype(np.float32)

    def _mark(self, rows):
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        assert rows.size == 0 or (rows.min() >= 0 and rows.max() < self.n), (self.label, rows)
        assert not self.special[rows].any() and len(np.unique(rows)) == len(rows), f"{self.label}: a row is planted twice"
        self.special[rows] = True
        return rows

    def level(self, rows, j, above_background=True):
        """Rows at level(s) j (a number for all of them: an exact tie; an array: one level each)."""
        rows = self._mark(rows)
        j = np.broadcast_to(np.asarray(j, dtype=np.float64), rows.shape)
        assert j.size == 0 or (j.min() >= 0 and (j.max() <= MAX_LEVEL or not above_background))
        self.d[rows] = _COLD[rows % len(_COLD)]
        self.xc[rows] = np.float32(0.5) * np.sign(self.q[self.c[rows]])
        self.xd[rows] = (0.5 * (0.05 + j * LEVEL_STEP)).astype(np.float32) * np.sign(self.q[self.d[rows]])
        return rows

    def ranked(self, items):
        """items: rows (or tuples of rows: exact ties) in the order of the expected list; levels 0, 1, 2, ..."""
        for j, item in enumerate(items):
            if isinstance(item, tuple):
                self.ties(item, j)
            else:
                self.level([item], j)

    def ties(self, rows, j):
        rows = self.level(rows, j)
        self.tie[rows] = self.groups
        self.groups += 1

    def nan(self, rows):
        rows = self._mark(rows)
        self.xc[rows] = 0.0
        self.xd[rows] = 0.0

    def zeros(self, rows):
        """Similarity exactly +0.0: xc = +0.0, the other element on a column where the query is 0.  One tie group."""
        rows = self._mark(rows)
        self.xc[rows] = 0.0
        self.d[rows] = _ZERO[rows % len(_ZERO)]
        self.xd[rows] = 1.0
        self.tie[rows] = self.groups
        self.groups += 1

    def eps(self, row, sign):
        rows = self._mark([row])
        self.d[rows] = _ZERO[rows % len(_ZERO)]
        self.xc[rows] = np.float32(sign) * EPS * np.sign(self.q[self.c[rows]])
        self.xd[rows] = 1.0

    def finish(self) -> Store:
        st = Store(self.label, self.xc, self.xd, self.c, self.d, self.tie, self.background)
        for _ in range(20):
            bad = st.violations()
            if len(bad) == 0:
                break
            again = bad[~self.special[bad]]
            assert len(again), f"{self.label}: planted rows collide with each other"
            self._draw(again)
        return st.check()


def around(points: Sequence[int], n: int, count: int) -> List[int]:
    """``count`` distinct rows alternating below and above each point: p - 1, p, p - 2, p + 1, ... round robin over the points."""
    out, seen, step = [], set(), 0
    while len(out) < count:
        for p in points:
            for r in (p - 1 - step, p + step):
                if 0 <= r < n and r not in seen and len(out) < count:
                    seen.add(r)
                    out.append(r)
        step += 1
        assert step <= n
    return out


def seams(n: int, ks: Sequence[int]) -> List[int]:
    """The first rows of the slices 1 .. G-1 of every plan the ks take on n rows."""
    out = []
    for k in ks:
        for lo, _ in flat_plan(n, k).slices()[1:]:
            if lo not in out and lo < n:
                out.append(lo)
    return out


def spread(n: int, count: int) -> List[int]:
    """``count`` distinct rows over the whole store, both ends included."""
    return sorted(set(np.linspace(0, n - 1, count).round().astype(int).tolist()))


# ---- layouts -----------------------------------------------------------------------------------------------------------------------
def _straddle(n, ks, seed):
    b = _Builder(n, f"straddle n={n}", seed)
    b.ranked(around(seams(n, ks), n, 80))
    return b.finish()


def _last_slice(n, ks, seed):
    b = _Builder(n, f"last slice n={n}", seed)
    b.ranked(list(range(n - 1, n - 1031, -1)))
    return b.finish()


def _first_slice(n, ks, seed):
    b = _Builder(n, f"first slice n={n}", seed)
    b.ranked(list(range(1030)))
    return b.finish()


def _one_group(n, ks, seed):
    c = source_constants()
    held = c["kF64Held"] * c["argmax_small"]
    assert n == held
    b = _Builder(n, "one group", seed)
    b.ranked([n - 1, 0] + list(range(held - c["argmax_small"], n - 1, 4)))          # the last register slot: 3840 .. 4095
    return b.finish()


def _chunk_seams(n, ks, seed):
    b = _Builder(n, "chunk seams", seed)
    items: list = []
    for lo, hi in flat_plan(n, ks[0]).slices():
        for off in (1023, 1024, 2047, 2048):
            if lo + off < hi:
                items.append(lo + off)
        items.append((lo + 1022, lo + 1025))                                          # an exact tie across the chunk seam
    b.ranked(items)
    return b.finish()


def _mixed(n, ks, seed):
    """Winners and exact ties around every seam (or the middle), NaN rows at both ends, at the seam and in the middle."""
    b = _Builder(n, f"mixed n={n}", seed)
    points = seams(n, [k for k in ks if flat_plan(n, k).path != "sort"] or [1]) or [n // 2]
    rows = around(points, n, 24)
    items: list = []
    for i in range(0, 24, 3):
        items += [rows[i], (rows[i + 1], rows[i + 2])]
    free = [r for r in (0, 1, n // 3, n - 2, n - 1, points[0] + 40, points[0] - 40) if r not in rows]
    b.ranked(items)
    b.nan(free[:5])
    b.ties(free[5:7], 30)
    return b.finish()


def _sort_cap(n, ks, seed):
    b = _Builder(n, "sort-path cap", seed)
    sa, sl = seams(n, [k for k in ks if flat_plan(n, k).path == "argmax"]), seams(n, [k for k in ks if flat_plan(n, k).path == "lds"])
    at = [p for pair in zip(sa, sl) for p in pair] + sa[len(sl):] + sl[len(sa):]    # the seams of both plans, taking turns
    b.ranked([n - 1, n - 2] + around(at, n, 2 * len(at)) + list(range(n - 3, n - 903, -1)))
    return b.finish()


def _second_level_1024(n, ks, seed):
    """One winner per first-level group of the k = 64 plan; the best ones in the groups whose candidates land in register slots
    4 and 0 of the second level's 1024 threads (candidate g * 64 is element g * 64: slot (g * 64) // 1024)."""
    p = flat_plan(n, ks[0])
    sl = p.slices()
    slot = lambda g: (g * p.k_eff) // p.threads2
    groups = [g for g in range(p.groups) if slot(g) == 4] + [g for g in range(p.groups) if slot(g) == 0]
    groups += [g for g in range(p.groups) if g not in groups]
    b = _Builder(n, "1024-thread second level", seed)
    b.ranked([sl[g][0] + (g * 61) % (sl[g][1] - sl[g][0]) for g in groups])
    return b.finish()


def _argmax_cap(n, ks, seed):
    """One winner per group in a quarter of the groups -- the last group (slot 15 of the second level) first --, each in another
    register slot of its first-level workgroup, then a run at the very end of the last, short slice."""
    p = flat_plan(n, max(ks))
    sl = p.slices()
    groups = [p.groups - 1] + list(range(0, p.groups - 1, 4))
    rows = []
    for i, g in enumerate(groups):
        lo, hi = sl[g]
        rows.append(min(lo + (i % 5) * p.threads1 + (i * 37) % p.threads1, hi - 1 - (i % 3)))
    b = _Builder(n, "arg-max cap", seed)
    b.ranked(rows + [r for r in range(n - 1, n - 40, -1) if r not in rows])
    return b.finish()


# order layouts
def _identical(n, k, seed):
    b = _Builder(n, f"identical n={n}", seed, background=False)
    b.ties(np.arange(n), 0)
    return b.finish()


def _zeros(n, k, seed):
    b = _Builder(n, f"zeros n={n}", seed, background=False)
    plus, minus = n // 2 + 1, n - 1
    b.eps(plus, +1)
    b.eps(minus, -1)
    b.zeros(np.array([r for r in range(n) if r not in (plus, minus)]))
    return b.finish()


def _ties_for_first(n, k, seed):
    b = _Builder(n, f"{k + 3} ties for first n={n}", seed)
    b.ties(spread(n, k + 3), 0)
    return b.finish()


def _many_nan(n, k, seed):
    b = _Builder(n, f"{k + 3} NaN rows n={n}", seed)
    b.nan(spread(n, k + 3))
    return b.finish()


def _nan_at_seams(n, k, seed):
    b = _Builder(n, f"NaN at the seams n={n}", seed)
    points = seams(n, [k]) or [n // 2]
    rows = around(points, n, 4 * len(points))
    b.nan(rows[: 2 * len(points)])
    b.ranked([tuple(rows[2 * len(points):])])                                          # an exact tie just outside the NaN rows
    return b.finish()


def _monotone(n, k, seed, falling):
    b = _Builder(n, f"{'descending' if falling else 'ascending'} n={n}", seed, background=False)
    rows = np.arange(n)
    b.level(rows, (rows if falling else rows[::-1]) * (8.0 * MAX_LEVEL / n), above_background=False)      # r from 0.05 to 7.25
    return b.finish()


# ---- case tables -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    n: int
    ks: Tuple[int, ...]
    make: Callable
    reaches: Dict[int, dict]            # k -> the fields of Plan the case claims (the CPU file compares them with flat_plan)
    seed: int = 0
    double_query: bool = False          # also run with the genuine-double query (TOL)
    large: bool = False                 # built alone on the device, freed before the next

    @property
    def id(self) -> str:
        return f"{self.name}-n{self.n}"

    def store(self) -> Store:
        if self.id not in _STORES:
            _STORES[self.id] = self.make(self.n, self.ks, self.seed)
        return _STORES[self.id]

    def forget(self) -> None:
        _STORES.pop(self.id, None)


_STORES: Dict[str, Store] = {}


def _two(groups, per, **more):
    """The claims of the four standard ks on a store of ``groups`` slices of ``per`` rows."""
    return {5: dict(path="argmax", groups=groups, per=per, threads1=256, held1=True, threads2=256, held2=True, **more),
            64: dict(path="argmax", groups=groups, per=per, threads1=256, held1=True, threads2=256, held2=True, **more),
            65: dict(path="lds", groups=groups, per=per), 1024: dict(path="lds", groups=groups, per=per)}


KS4 = (5, 64, 65, 1024)
FLAT: List[Case] = [
    Case("one group", 4096, (1, 64), _one_group,
         {1: dict(path="argmax", groups=1, per=4096, threads1=256, held1=True), 64: dict(path="argmax", groups=1, per=4096, held1=True)}),
]
for _n, _g, _per in ((4097, 2, 2049), (8192, 2, 4096), (8193, 3, 2731)):
    FLAT += [Case("straddle", _n, KS4, _straddle, _two(_g, _per), 1, double_query=_n == 4097),
             Case("last slice", _n, KS4, _last_slice, _two(_g, _per), 2),
             Case("first slice", _n, KS4, _first_slice, _two(_g, _per), 3)]
FLAT += [
    Case("chunk seams", 4097, (65, 1024), _chunk_seams, {65: dict(path="lds", groups=2, per=2049), 1024: dict(path="lds", groups=2, per=2049)}, 4),
    Case("k boundaries", 4097, (64, 65, 1024, 1025, 4097, 4100), _mixed,
         {64: dict(path="argmax"), 65: dict(path="lds"), 1024: dict(path="lds"), 1025: dict(path="sort", n_pad=8192),
          4097: dict(path="sort", k_eff=4097), 4100: dict(path="sort", k_eff=4097)}, 5),
    Case("full sort", 2048, (1025,), _mixed, {1025: dict(path="sort", n_pad=2048)}, 6),
    Case("full sort", 2049, (1025,), _mixed, {1025: dict(path="sort", n_pad=4096)}, 7),
    Case("full sort", 1025, (1025,), _mixed, {1025: dict(path="sort", n_pad=2048, k_eff=1025)}, 8),
    Case("sort-path cap", 32 * 4096 + 1, (64, 65, 1024), _sort_cap,
         {64: dict(path="argmax", groups=33, per=3972, threads1=256, held1=True, cand=2112, threads2=256),
          65: dict(path="lds", groups=32, per=4097, cand=2080), 1024: dict(path="lds", groups=32, per=4097, cand=32 * 1024)}, 9, large=True),
    Case("1024-thread second level", 64 * 4096 + 1, (64, 63), _second_level_1024,
         {64: dict(path="argmax", groups=65, cand=4160, threads2=1024, held2=True),
          63: dict(path="argmax", groups=65, cand=4095, threads2=256, held2=True)}, 10, large=True),
    Case("arg-max cap", 256 * 4096 + 1, (5, 64), _argmax_cap,
         {5: dict(path="argmax", groups=256, per=4097, threads1=1024, held1=True, cand=1280, threads2=256, held2=True),
          64: dict(path="argmax", groups=256, per=4097, threads1=1024, held1=True, cand=16384, threads2=1024, held2=True)}, 11, large=True),
]

ORDER_KINDS = {
    "identical": _identical, "zeros": _zeros, "ties for first": _ties_for_first, "many NaN": _many_nan, "NaN at seams": _nan_at_seams,
    "ascending": lambda n, k, seed: _monotone(n, k, seed, False), "descending": lambda n, k, seed: _monotone(n, k, seed, True),
}
ORDER_SHAPES = [(4097, k) for k in KS4] + [(8193, k) for k in KS4] + [(2049, 1025)]
_PER_K = ("ties for first", "many NaN")


@functools.lru_cache(maxsize=None)
def order_store(kind: str, n: int, k: int) -> Store:
    """The store of an order case; only the two kinds that count k + 3 rows depend on k."""
    return ORDER_KINDS[kind](n, k, 20 + list(ORDER_KINDS).index(kind))


def order_cases() -> List[Tuple[str, int, Tuple[int, ...]]]:
    """(kind, n, ks): one store each."""
    out = []
    for kind in ORDER_KINDS:
        for n in (4097, 8193, 2049):
            ks = [k for m, k in ORDER_SHAPES if m == n]
            out += [(kind, n, (k,)) for k in ks] if kind in _PER_K else [(kind, n, tuple(ks))]
    return out


def get_order_store(kind, n, ks) -> Store:
    return order_store(kind, n, ks[0] if kind in _PER_K else 0)


# ---- segmented -------------------------------------------------------------------------------------------------------------------
SEG_N = 8200
SEG_KS = KS4
# The nine sizes 0, 1, 1023, 1024, 1025, 2048, 2049, 4096, 4097 add up to more than 8,200 rows, so they take two tables over the
# one store (a call per table and k); every table ends at n_rows and has events that start at odd rows.
SEG_TABLES = {
    "small": [0, 0, 1, 1024, 2048, 3073, 5121, 7170, 8200],           # 0, 1, 1023, 1024, 1025, 2048, 2049, (1030)
    "large": [0, 3, 4099, 8196, 8200],                                 # (3), 4096, 4097, (4)
}
SEG_SIZES = (0, 1, 1023, 1024, 1025, 2048, 2049, 4096, 4097)


@functools.lru_cache(maxsize=None)
def segmented_store() -> Store:
    b = _Builder(SEG_N, "segmented", 40)
    level = 0
    for table in SEG_TABLES.values():
        for lo, hi in zip(table[:-1], table[1:]):
            rows = [r for r in (lo, hi - 1) if lo <= r < hi and not b.special[r]]
            for r in dict.fromkeys(rows):                          # winners at the event's first and last row
                b.level([r], level)
                level += 1
            for seam in range(lo + 1024, hi, 1024):                # an exact tie across every 1024-pair seam of the event
                pair = [r for r in (seam - 1, seam) if not b.special[r]]
                if len(pair) == 2:
                    b.ties(pair, level)
                    level += 1
    b.nan([r for r in (5000, 7171) if not b.special[r]])
    return b.finish()


CLAMP_TABLES = {
    "negative first offset": [-5, 10, 20],
    "offset beyond n_rows": [0, 100, SEG_N + 50],
    "descending pair": [0, 500, 300, 800],
}


# ---- eligibility -----------------------------------------------------------------------------------------------------------------
ELIG_ROWS = 8200


def eligibility_offenders() -> Dict[str, int]:
    """Flat offsets in a (8200, 1024) float64 source, from the kernel's grid rule: workgroup b, step s reads offsets
    s * grid * 256 + b * 256 + thread."""
    c = source_constants()
    n_values = ELIG_ROWS * DIM
    grid = eligibility_grid(n_values)
    step = grid * c["elig_threads"]
    steps = (n_values + step - 1) // step
    return {"last": n_values - 1,
            "high workgroup, first step": (grid - 1) * c["elig_threads"] + 5,
            "low workgroup, late step": (steps - 2) * step + 3}


def eligibility_source(seed: int = 0) -> np.ndarray:
    """(8200, 1024) float64, every value an fp32 value."""
    rng = np.random.default_rng(6500 + seed)
    return rng.standard_normal((ELIG_ROWS, DIM), dtype=np.float32).astype(np.float64)


def f32_specials() -> np.ndarray:
    """fp32 values a careless check trips over: +-0.0, fp32 subnormals, +-inf, +-FLT_MAX, a NaN whose payload narrows exactly."""
    f = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, np.inf, -np.inf, np.finfo(np.float32).max, -np.finfo(np.float32).max],
                 dtype=np.float32)
    nan = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)
    return np.concatenate([f, nan]).astype(np.float64)


def not_f32_values() -> Dict[str, float]:
    """Doubles that are no fp32 value.  The last one is the smallest deviation there is: the double right after an fp32 value
    (2^-52 of it).  Adding 2^-60 of x to float(np.float32(x)) is lost in the rounding of the sum -- the result IS the fp32 value
    (the CPU file asserts that) -- so the next double stands in for it."""
    return {"1e300": 1e300, "double subnormal": 5e-324, "the double after an fp32 value": float(np.nextafter(float(np.float32(0.7314)), 1.0))}
