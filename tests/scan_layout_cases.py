"""Adversarial row layouts for the retrieval kernels: the dealing restated in Python, a store recipe whose similarities are planted
exactly, the layouts, the case tables and the references.  Shared by tests/test_cpu_scan_layouts.py (which proves, without a GPU,
that every layout puts its rows where it says and that the winners are separated) and tests/test_gpu_scan_layouts.py.

Nothing here is a number copied from the kernels: every ROWS / WAVES pair, grid cap, list capacity and dispatch limit is read out
of hippomm_amd/csrc (``SRC``), so a change there moves the layouts -- or fails the CPU file -- instead of leaving them beside
the point.

The store.  With orthonormal u_0 .. u_{Q-1} and v,  row_i = (sum_q c[q, i] u_q + sqrt(1 - sum_q c[q, i]^2) v) * scale_i  in fp32,
question q = u_q * qscale_q: the cosine similarity of row i to question q is c[q, i] up to fp32 rounding (~1e-7).  Winner j of a
question is planted at 0.9 - 1e-3 j, decoys in [0.6, 0.7], background within +-0.5 (times ``bg_scale(Q)`` for a batch, so that
sum_q c^2 < 1); a row is a winner or a decoy of at most one question (``taken``)."""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "hippomm_amd" / "csrc"
_FILES = ("hmm_common.h", "cosine_topk_shared.h", "topk_select.h", "cosine_topk.hip", "cosine_topk_prefilter.hip",
          "cosine_topk_multi.hip")

SIM_ATOL = 2e-6                  # tests/test_gpu_scan.py: the fp32 scan against a high-precision similarity
WINNER_TOP, WINNER_STEP, WINNER_FLOOR = 0.9, 1e-3, 0.773
DECOY_LO, DECOY_HI = 0.6, 0.7
MIN_WINNER_GAP, MIN_WINNER_MARGIN = 5e-4, 5e-2       # the separation condition of the zero-exemption tests


# ---- constants out of the sources ------------------------------------------------------------------------------------------------
def _source_text() -> str:
    """The kernels' sources without their probe-only parts (#ifdef HMM_PROBE ... #endif: never in the shipped library)."""
    text = "\n".join((CSRC / f).read_text() for f in _FILES)
    return re.sub(r"#ifdef HMM_PROBE\b.*?#endif", "", text, flags=re.S)


def _evaluate(exprs: dict) -> dict:
    """name -> int for every expression made of integers, + - * / ( ) and names that resolve the same way."""
    known: dict = {}
    progress = True
    while progress:
        progress = False
        for name, expr in exprs.items():
            if name in known or not re.fullmatch(r"[\w\s+\-*/()]+", expr):
                continue
            names = set(re.findall(r"[A-Za-z_]\w*", expr))
            if names <= set(known):
                known[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(known)))
                progress = True
    return known


@functools.lru_cache(maxsize=None)
def source_constants() -> dict:
    text = _source_text()
    exprs = {m.group(1): m.group(2).strip() for m in re.finditer(r"constexpr\s+int\s+(\w+)\s*=\s*([^;,]+);", text)}
    exprs.update({m.group(1): m.group(2).strip() for m in re.finditer(r"HMM_TUNABLE\(\s*int\s*,\s*(\w+)\s*,\s*([^)]+)\)", text)})
    c = _evaluate(exprs)
    # the flat shadow route's dispatch limit is written into its launcher (hmm_cosine_topk_prefilter)
    m = re.search(r"k > kPrefilterMaxK \|\| n_rows < \(int64_t\)(kChunk \* \d+)", text)
    c["kPrefilterMinRows"] = _evaluate({**{k: str(v) for k, v in c.items()}, "x": m.group(1)})["x"]
    # prefilter_list_len(k): max(2 k, floor) capped at kListMaxK
    m = re.search(r"const int kk = 2 \* k < (\d+) \? (\d+) : 2 \* k;\s*return kk > kListMaxK \? kListMaxK : kk;", text)
    assert m and m.group(1) == m.group(2), "prefilter_list_len changed its form"
    c["kPrefilterListFloor"] = int(m.group(1))
    # the loops' own compaction rule, and the quick route's limit of select_ranked_hits
    assert "(kFusedCap - k) / ScanDealing::kBlockRows" in text and "(kFusedCap - k) / PrefilterDealing::kBlockRows" in text
    m = re.search(r"total <= \(int64_t\)(\d+) \* \(kChunk / (\d+)\)", text)
    c["kRankQuickMax"] = int(m.group(1)) * (c["kChunk"] // int(m.group(2)))
    c["kRankThreads"] = int(m.group(1))
    c["kPrefilterEps"] = float(re.search(r"constexpr float kPrefilterEps = ([\d.]+)f;", text).group(1))
    return c


def prefilter_list_len(k: int) -> int:
    c = source_constants()
    return min(max(2 * k, c["kPrefilterListFloor"]), c["kListMaxK"])


class Dealing:
    """RowDealing<ROWS, WAVES> of topk_select.h with the grid cap of the kernel that names it."""

    def __init__(self, name: str, rows: int, waves: int, cap: int):
        self.name, self.rows, self.waves, self.cap = name, rows, waves, cap
        self.block_rows = rows * waves

    def __repr__(self):
        return f"{self.name}<{self.rows},{self.waves}>"

    def grid(self, n: int) -> int:
        return min(-(-n // self.block_rows), self.cap)

    def rows_per_iteration(self, n_blocks: int) -> int:
        return n_blocks * self.block_rows

    def iterations(self, n: int, n_blocks: int) -> int:
        return -(-n // self.rows_per_iteration(n_blocks))

    def block_of_row(self, row, n_blocks: int):
        """The inverse, as the finish kernels compute it (also on numpy arrays)."""
        return ((row // self.rows) % (n_blocks * self.waves)) // self.waves

    def iteration_of_row(self, row, n_blocks: int):
        return (row // self.rows) // (n_blocks * self.waves)

    def rows_by_iteration(self, b: int, n: int, n_blocks: int) -> list:
        """The forward direction, as the streaming loop walks it: wave w of workgroup b takes group w + it * n_waves."""
        n_waves = n_blocks * self.waves
        out = []
        for it in range(self.iterations(n, n_blocks)):
            groups = b * self.waves + np.arange(self.waves, dtype=np.int64) + it * n_waves
            rows = (groups[:, None] * self.rows + np.arange(self.rows, dtype=np.int64)[None, :]).reshape(-1)
            out.append(rows[rows < n])
        return out

    def rows_of_block(self, b: int, n: int, n_blocks: int) -> np.ndarray:
        return np.concatenate(self.rows_by_iteration(b, n, n_blocks) or [np.zeros(0, np.int64)])


@functools.lru_cache(maxsize=None)
def dealings() -> dict:
    """name -> Dealing for the four descriptors, plus ``ChunkDealing``: the routes that sort similarities chunk by chunk
    (topk_chunk_kernel: n <= kChunk, k > kFusedK) have one workgroup per kChunk consecutive rows and a single iteration."""
    text, c = _source_text(), source_constants()
    caps: dict = {}
    for m in re.finditer(r"(\w+Dealing)::grid\(\s*\w+\s*,\s*(\w+)\s*\)", text):
        caps.setdefault(m.group(1), set()).add(c[m.group(2)])
    out = {}
    for m in re.finditer(r"using\s+(\w+)\s*=\s*RowDealing<\s*([^,>]+?)\s*,\s*([^>]+?)\s*>", text):
        name = m.group(1)
        assert len(caps[name]) == 1, (name, caps[name])
        out[name] = Dealing(name, c.get(m.group(2)) or int(m.group(2)), c.get(m.group(3)) or int(m.group(3)), next(iter(caps[name])))
    out["ChunkDealing"] = Dealing("ChunkDealing", c["kChunk"], 1, 1 << 30)
    return out


def compact_every(dealing: Dealing, list_len: int) -> int:
    """Iterations between two compact_block_list calls of a streaming loop that keeps ``list_len`` keys."""
    return (source_constants()["kFusedCap"] - list_len) // dealing.block_rows


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Plant:
    """Where one question's special rows sit.  ``winners`` in rank order (best first)."""
    layout: str
    block: int = -1
    winners: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    decoys: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    zero: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))      # all-zero rows: NaN similarity
    ties: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))      # bit-identical rows, copies of ties[0]
    ramp: int = 0                                                                # +1 ascending / -1 descending background

    def special(self) -> np.ndarray:
        return np.concatenate([self.winners, self.decoys, self.zero, self.ties]).astype(np.int64)


def _free(rows: np.ndarray, taken) -> np.ndarray:
    return rows if taken is None or len(taken) == 0 else rows[~np.isin(rows, taken)]


def _block(which: float, n_blocks: int) -> int:
    return int(round(which * (n_blocks - 1)))


def _spread(rows: np.ndarray, count: int) -> np.ndarray:
    assert len(rows) >= count, (len(rows), count)
    return rows[np.round(np.linspace(0, len(rows) - 1, count)).astype(np.int64)] if count else rows[:0]


def _one_workgroup(where: str):
    def f(d, n, nb, k, window, taken, rng, which):
        b = _block(which, nb)
        rows = _free(d.rows_of_block(b, n, nb), taken)                # in the order the workgroup meets them
        assert len(rows) >= k, f"workgroup {b} has {len(rows)} free rows, needs {k}"
        sel = {"spread": _spread(rows, k), "first": rows[:k], "last": rows[len(rows) - k:]}[where]
        return Plant("one_workgroup" if where == "spread" else f"one_workgroup_{where}_iterations", b, winners=rng.permutation(sel))
    return f


def _one_per_workgroup(d, n, nb, k, window, taken, rng, which):
    assert nb >= k + 1, (nb, k)
    pick = []
    for j in range(k + 1):
        rows = _free(d.rows_of_block(j, n, nb), taken)
        pick.append(rows[(7 * j) % len(rows)])
    return Plant("one_per_workgroup", -1, winners=np.array(pick[:k], np.int64), decoys=np.array(pick[k:], np.int64))


def _head(d, n, nb, k, window, taken, rng, which):
    return Plant("head", -1, winners=rng.permutation(_free(np.arange(n, dtype=np.int64), taken)[:k]))


def _tail(d, n, nb, k, window, taken, rng, which):
    rows = _free(np.arange(n, dtype=np.int64), taken)
    return Plant("tail", -1, winners=rng.permutation(rows[len(rows) - k:]))


def _ascending(d, n, nb, k, window, taken, rng, which):
    rows = _free(np.arange(n, dtype=np.int64), taken)
    return Plant("ascending", -1, winners=rows[::-1][:k].copy(), ramp=+1)             # the last row is the best


def _descending(d, n, nb, k, window, taken, rng, which):
    return Plant("descending", -1, winners=_free(np.arange(n, dtype=np.int64), taken)[:k].copy(), ramp=-1)


def _windows(d, b, n, nb, window, taken) -> list:
    """The free rows of workgroup b per compaction window (one window when the loop never compacts before its end)."""
    its = [_free(r, taken) for r in d.rows_by_iteration(b, n, nb)]
    if not window or len(its) <= window:
        return [np.concatenate(its)]
    return [np.concatenate(its[s:s + window]) for s in range(0, len(its), window)]


def _decoys_then_winners(d, n, nb, k, window, taken, rng, which):
    b = _block(which, nb)
    wins = _windows(d, b, n, nb, window, taken)
    rows = np.concatenate(wins)
    assert len(rows) >= k + 1, (len(rows), k)
    winners = rows[len(rows) - k:]                                                    # the workgroup's last iterations
    decoys = [np.setdiff1d(w, winners, assume_unique=True)[:k] for w in wins]         # k per window, at its start
    return Plant("decoys_then_winners", b, winners=rng.permutation(winners), decoys=np.concatenate(decoys))


def _winners_then_decoys(d, n, nb, k, window, taken, rng, which):
    b = _block(which, nb)
    wins = _windows(d, b, n, nb, window, taken)
    rows = np.concatenate(wins)
    assert len(rows) >= k + 1, (len(rows), k)
    winners = rows[:k]                                                                # the workgroup's first iterations
    decoys = [np.setdiff1d(w, winners, assume_unique=True)[:k] for w in wins]         # k behind them, k more after every compaction
    return Plant("winners_then_decoys", b, winners=rng.permutation(winners), decoys=np.concatenate(decoys))


def _nan_block(d, n, nb, k, window, taken, rng, which):
    b = _block(which, nb)
    zero = _spread(_free(d.rows_of_block(b, n, nb), taken), k + 3)
    others = np.setdiff1d(np.arange(n, dtype=np.int64), zero, assume_unique=True)
    return Plant("nan_block", b, winners=rng.permutation(_spread(others, min(k, len(others)))), zero=zero)


def _tie_block(d, n, nb, k, window, taken, rng, which):
    b = _block(which, nb)
    ties = [_spread(_free(d.rows_of_block(b, n, nb), taken), k + 5)]
    for other in ((b + 1) % nb, (b + max(nb // 2, 1)) % nb):
        if other != b:
            rows = _free(d.rows_of_block(other, n, nb), taken)
            ties.append(rows[len(rows) // 2:len(rows) // 2 + 1])
    return Plant("tie_block", b, ties=np.concatenate(ties))


_LAYOUTS = {
    "one_workgroup": _one_workgroup("spread"),
    "one_workgroup_first_iterations": _one_workgroup("first"),
    "one_workgroup_last_iterations": _one_workgroup("last"),
    "one_per_workgroup": _one_per_workgroup, "head": _head, "tail": _tail, "ascending": _ascending, "descending": _descending,
    "decoys_then_winners": _decoys_then_winners, "winners_then_decoys": _winners_then_decoys,
    "nan_block": _nan_block, "tie_block": _tie_block,
}
_WHICH = {"first": 0.0, "mid": 0.5, "last": 1.0}
REQUIRED_LAYOUTS = ("one_workgroup", "ascending", "decoys_then_winners")


def layout_kind(name: str) -> str:
    return name.split("@")[0]


def make_plant(name: str, d: Dealing, n: int, n_blocks: int, k: int, window=None, taken=None, seed: int = 0) -> Plant:
    """``name`` is a layout, optionally with the workgroup it concentrates on: "one_workgroup@last", "tie_block@0.25"."""
    kind, _, which = name.partition("@")
    frac = _WHICH[which] if which in _WHICH else float(which or 0.5)
    rng = np.random.default_rng(seed * 7919 + k * 31 + n)
    return _LAYOUTS[kind](d, n, n_blocks, k, window, taken, rng, frac)


def winner_value(j, k: int):
    """0.9 - 1e-3 j (the lowest of 128 winners is 0.773); beyond 128 winners the same range in finer steps."""
    step = WINNER_STEP if k <= 128 else (WINNER_TOP - WINNER_FLOOR) / (k - 1)
    return WINNER_TOP - step * np.asarray(j, dtype=np.float64)


def bg_scale(n_questions: int) -> float:
    """Background amplitude of a batch: 17 x (0.5 x 0.2)^2 + 0.9^2 = 0.98 < 1."""
    return 1.0 if n_questions == 1 else 0.2


def planted_vector(p: Plant, n: int, k: int, scale: float = 1.0, seed: int = 0) -> np.ndarray:
    """c[0 .. n) of one question (fp64).  Zero rows keep a background value here: they are zeroed in the store."""
    rng = np.random.default_rng(seed * 104729 + n)
    if p.ramp:
        c = np.linspace(-0.5, 0.5, n)[::p.ramp].copy() * scale
    else:
        c = rng.uniform(-0.5, 0.5, n) * scale
    c[p.decoys] = rng.uniform(DECOY_LO, DECOY_HI, len(p.decoys))
    c[p.winners] = winner_value(np.arange(len(p.winners)), k)
    c[p.ties] = WINNER_TOP
    return c


def plant_questions(names, d: Dealing, n: int, n_blocks: int, k: int, window=None, seed: int = 0):
    """One layout per question on the same store: (plants, c (Q, n) fp64).  Question q never plants on a row another took."""
    taken = np.zeros(0, np.int64)
    plants = []
    for q, name in enumerate(names):
        p = make_plant(name, d, n, n_blocks, k, window, taken, seed + q)
        plants.append(p)
        taken = np.concatenate([taken, p.special()])
    scale = bg_scale(len(plants))
    c = np.stack([planted_vector(p, n, k, scale, seed + q) for q, p in enumerate(plants)])
    return plants, c


def batch_layouts(n_questions: int) -> list:
    """The layouts of a batched call: the first four are fixed, the others cycle through the rest."""
    fixed = ["ascending", "descending", "one_workgroup@last", "decoys_then_winners@last"]
    rest = ["one_workgroup@first", "one_workgroup@mid", "one_per_workgroup", "head", "tail", "winners_then_decoys@0.4",
            "one_workgroup_first_iterations@0.1", "one_workgroup_last_iterations@0.6", "decoys_then_winners@0.2",
            "one_workgroup@0.3", "one_workgroup_last_iterations@0.7", "decoys_then_winners@0.8"]
    return (fixed + [rest[i % len(rest)] for i in range(max(n_questions - 4, 0))])[:n_questions]


# ---- the store recipe (torch, on any device) -------------------------------------------------------------------------------------
def basis(n_questions: int, device, seed: int = 5):
    """(U (Q, 1024), v (1024,)) orthonormal, fp32."""
    import torch
    a = torch.randn(1024, n_questions + 1, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    q, _ = torch.linalg.qr(a)
    q = q.T.contiguous().to(torch.float32).to(device)
    return q[:n_questions].contiguous(), q[n_questions].contiguous()


def query_scales(n_questions: int):
    return [1.0 + 0.5 * q for q in range(n_questions)]


def queries_of(U):
    import torch
    return (U * torch.tensor(query_scales(U.shape[0]), dtype=torch.float32, device=U.device)[:, None]).contiguous()


def recipe_rows(cc, row_index, U, v, out=None):
    """The rows ``row_index`` of the store from their planted values cc (Q, m) fp32, in fp32 on cc's device."""
    import torch
    w = (1.0 - (cc * cc).sum(0)).clamp_min(0.0).sqrt()
    blk = torch.empty(cc.shape[1], 1024, dtype=torch.float32, device=cc.device) if out is None else out
    torch.mul(v[None, :], w[:, None], out=blk)
    for q in range(cc.shape[0]):
        blk.addcmul_(cc[q][:, None], U[q][None, :])
    scale = 0.5 + 2.5 * torch.frac(row_index.to(torch.float64) * 0.6180339887498949)  # per-row scale in [0.5, 3)
    return blk.mul_(scale.to(torch.float32)[:, None])


def fill_rows(out, c, U, v, zero=(), ties=(), chunk: int = 1 << 16):
    """out[0 .. n) (a (n, 1024) fp32 view of the module's buffer) from c (Q, n): built on out's device in row chunks."""
    import torch
    n = out.shape[0]
    c = torch.as_tensor(np.ascontiguousarray(c), dtype=torch.float32).to(out.device)
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        recipe_rows(c[:, s:e], torch.arange(s, e, device=out.device), U, v, out=out[s:e])
    if len(zero):
        out[torch.as_tensor(np.asarray(zero), device=out.device)] = 0.0
    if len(ties) > 1:
        out[torch.as_tensor(np.asarray(ties[1:]), device=out.device)] = out[int(ties[0])].clone()
    return out


def reference_sims(rows, queries, chunk: int = 1 << 15) -> np.ndarray:
    """The high-precision reference: fp64 cosine similarity of the fp32 rows, (Q, n), computed on the rows' device."""
    import torch
    qd = queries.double()
    qn = qd.norm(dim=1)
    out = torch.empty(queries.shape[0], rows.shape[0], dtype=torch.float64, device=rows.device)
    for s in range(0, rows.shape[0], chunk):
        r = rows[s:s + chunk].double()
        out[:, s:s + chunk] = ((r @ qd.T) / (r.norm(dim=1)[:, None] * qn[None, :])).T
    return out.cpu().numpy()


def separation(ref: np.ndarray, k: int):
    """(smallest gap between adjacent ranks among the best k, gap between rank k and rank k + 1) of one fp64 similarity vector."""
    s = np.sort(ref[~np.isnan(ref)])[::-1][:k + 1]
    gaps = s[:-1] - s[1:]
    kk = min(k, len(s))
    inner = float(gaps[:kk - 1].min()) if kk > 1 else np.inf
    outer = float(gaps[k - 1]) if len(s) > k else np.inf
    return inner, outer


# ---- shapes and case tables ------------------------------------------------------------------------------------------------------
def iterations_for(d: Dealing, k: int) -> int:
    """Iterations of the full grid after which one workgroup holds k decoys and k winners, three at least."""
    return max(3, -(-2 * k // d.block_rows) + 1)


def rows_for(d: Dealing, iterations: int) -> int:
    """``iterations`` whole iterations of the full grid and three rows: odd, no multiple of ROWS, a straggler row at the end."""
    return iterations * d.rows_per_iteration(d.cap) + 3


@dataclass(frozen=True)
class FlatCase:
    route: str            # see FLAT_ROUTES
    layout: str
    k: int
    n: int
    dealing: str
    list_len: int         # keys a workgroup keeps on this route

    @property
    def id(self):
        return f"{self.route}-{self.layout}-k{self.k}-n{self.n}"

    def geometry(self):
        d = dealings()[self.dealing]
        nb = d.grid(self.n)
        ce = compact_every(d, self.list_len) if self.dealing != "ChunkDealing" else None
        return d, nb, ce

    def plant(self):
        d, nb, ce = self.geometry()
        return make_plant(self.layout, d, self.n, nb, self.k, ce)


_ALL_FLAT = ["one_workgroup@first", "one_workgroup@mid", "one_workgroup@last", "one_workgroup_first_iterations@mid",
             "one_workgroup_last_iterations@mid", "one_per_workgroup", "head", "tail", "ascending", "descending",
             "decoys_then_winners@last", "winners_then_decoys@last", "nan_block@mid", "tie_block@last"]
_CORE = ["one_workgroup@last", "ascending", "decoys_then_winners@last"]
_COMPACT = ["decoys_then_winners@last", "winners_then_decoys@last", "ascending", "one_workgroup@last"]


@functools.lru_cache(maxsize=None)
def exact_cases() -> tuple:
    """(b): the exact single-question routes of hmm_cosine_topk, each at the smallest shape that reaches it."""
    c, ds = source_constants(), dealings()
    scan = ds["ScanDealing"]
    out = []

    def add(route, layouts, k, n, dealing="ScanDealing"):
        out.extend(FlatCase(route, lay, k, n, dealing, k) for lay in layouts)

    for k in (32, 100):                                                    # n <= kChunk: similarities, one chunk sort
        add("chunk", ["one_workgroup@first", "ascending", "decoys_then_winners@first", "tie_block@first"], k, c["kChunk"], "ChunkDealing")
    for k in (5, 64):                                                      # fused scan, one-kernel finish (k k <= kChunk)
        add("fused_final", _ALL_FLAT, k, rows_for(scan, iterations_for(scan, k)))
    for k in (1, 32):
        add("fused_final", _CORE + ["tie_block@last"], k, rows_for(scan, iterations_for(scan, k)))
    for k in (65, c["kFusedK"]):                                           # fused scan, chunk passes
        add("fused_chunks", _CORE + ["one_per_workgroup", "tail", "nan_block@mid", "tie_block@last"], k,
            rows_for(scan, iterations_for(scan, k)))
    for k in (64, c["kFusedK"]):                                           # compaction inside the streaming loop
        add("fused_compact", _COMPACT, k, rows_for(scan, compact_every(scan, k) + 2))
    for k in (c["kFusedK"] + 1, c["kFastK"]):                              # similarities to a buffer, chunk sorts
        add("sims_buffer", ["one_workgroup@first", "ascending", "decoys_then_winners@last", "descending"], k, 2 * c["kChunk"] + 1809,
            "ChunkDealing")
    add("full_sort", ["one_workgroup@first", "ascending", "decoys_then_winners@first"], c["kFastK"] + 1, c["kChunk"] + 1 + 2,
        "ChunkDealing")
    return tuple(out)


@functools.lru_cache(maxsize=None)
def shadow_cases() -> tuple:
    """(c): hmm_cosine_topk_prefilter at and above its dispatch limit, and one store above its in-loop compaction."""
    c, d = source_constants(), dealings()["PrefilterDealing"]
    out = []
    for k in (1, 5, 32, 64):
        n = max(rows_for(d, iterations_for(d, k)), c["kPrefilterMinRows"] + 3)
        lays = _CORE + ["one_per_workgroup", "winners_then_decoys@last", "tail"] + (["tie_block@last", "nan_block@mid"] if k in (5, 64) else [])
        out.extend(FlatCase("shadow", lay, k, n, "PrefilterDealing", prefilter_list_len(k)) for lay in lays)
    for k in (32, 64):                                                     # both keep 64-entry lists
        n = rows_for(d, compact_every(d, prefilter_list_len(k)) + 2)
        out.extend(FlatCase("shadow_compact", lay, k, n, "PrefilterDealing", prefilter_list_len(k)) for lay in _COMPACT)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fallback_cases() -> tuple:
    """(c), the conditional exact scan behind the shadow route (exact_scan_fallback_kernel and its last-ticket finish): layouts of
    ScanDealing -- the dealing of that kernel -- on a store whose shadow pass is made to give up by ``saturators``."""
    scan, pre = dealings()["ScanDealing"], dealings()["PrefilterDealing"]
    out = []
    for k, lays in ((5, None), (64, None), (1, ["one_workgroup@last"]), (32, ["one_workgroup@last"])):
        n = max(rows_for(scan, iterations_for(scan, k)), rows_for(pre, 5))
        lays = lays or ["one_workgroup@first", "one_workgroup@mid", "one_workgroup@last", "decoys_then_winners@last", "ascending",
                        "one_per_workgroup", "tie_block@last"]
        out.extend(FlatCase("shadow_fallback", lay, k, n, "ScanDealing", k) for lay in lays)
    return tuple(out)


def saturators(case: FlatCase, p: Plant):
    """(rows, planted values): more rows than a shadow list keeps, all dealt to ONE workgroup of the shadow pass and all within the
    shadow's error margin below the k-th best row: that list's last entry passes the threshold, the list counts as saturated and
    the call falls back to the exact scan.  They sit 2e-3 below the lowest winner, 1e-5 apart: never part of the answer."""
    pre = dealings()["PrefilterDealing"]
    nb = pre.grid(case.n)
    rows = _free(pre.rows_of_block(nb // 3, case.n, nb), p.special())[:prefilter_list_len(case.k) + 6]
    floor = WINNER_TOP if len(p.ties) else float(winner_value(case.k - 1, case.k))
    return rows, floor - 2e-3 - 1e-5 * np.arange(len(rows))


def max_flat_rows() -> int:
    return max(case.n for case in exact_cases() + shadow_cases() + fallback_cases())


@dataclass(frozen=True)
class BatchCase:
    route: str            # "multi" (MultiDealing) or "multi_prefilter" (ShadowMultiDealing; its fallback is "multi")
    n_questions: int
    k: int
    n: int

    @property
    def id(self):
        return f"{self.route}-q{self.n_questions}-k{self.k}-n{self.n}"

    def geometry(self):
        d = dealings()["MultiDealing" if self.route == "multi" else "ShadowMultiDealing"]
        return d, d.grid(self.n)

    def plant(self):
        d, nb = self.geometry()
        names = batch_layouts(self.n_questions)
        if nb < d.cap:                                                     # one round: a workgroup holds kBlockRows rows only
            names = ["ascending", "descending", "one_workgroup@0.6", "decoys_then_winners@0.4"][:self.n_questions]
        return plant_questions(names, d, self.n, nb, self.k)


@functools.lru_cache(maxsize=None)
def batch_cases() -> tuple:
    """(d): 16 questions in one pass, 17 in two, 3 (lanes without a question), and a grid below its cap."""
    c, ds = source_constants(), dealings()
    rounds = 4 * ds["MultiDealing"].rows_per_iteration(ds["MultiDealing"].cap) + 5             # 4 x 16 384 + 5
    assert rounds >= c["kMPMinRows"]
    out = []
    for route in ("multi", "multi_prefilter"):
        out += [BatchCase(route, c["kMQ"], k, rounds) for k in (1, 5, 63, 64)]
        out += [BatchCase(route, c["kMQ"] + 1, k, rounds) for k in (5, 64)]
        out += [BatchCase(route, 3, 64, rounds)]
    out += [BatchCase("multi", 3, 5, 100 * ds["MultiDealing"].block_rows + 5)]                 # 100 workgroups < kNumCU
    out += [BatchCase("multi_prefilter", 3, 5, c["kMPMinRows"] + 100 * ds["ShadowMultiDealing"].block_rows + 5)]
    return tuple(out)


# ---- per-event layouts -----------------------------------------------------------------------------------------------------------
EVENT_MODES = ("first_piece", "last_piece", "seam", "ascending", "descending")


def event_sizes(k: int, large: bool) -> list:
    c = source_constants()
    small, chunk = c["kSmallSegChunk"], c["kChunk"]
    if large:                                                              # mean above g_small_segment_rows: the 4096-key shape
        return [chunk, chunk + 1, 3 * chunk - k + 1]
    return [k, k + 1, small - 1, small, small + 1, 2 * small + 7, 1, 0]


def event_chunk(sizes, k: int) -> int:
    """The LDS chunk the per-event kernels fold an event through (segments_are_small)."""
    c = source_constants()
    small = k <= c["kListMaxK"] and len(sizes) >= 1 and sum(sizes) <= len(sizes) * c["g_small_segment_rows"]
    return c["kSmallSegChunk"] if small else c["kChunk"]


def fold_pieces(m: int, k: int, chunk: int) -> list:
    """[lo, hi) of the pieces fold_topk cuts a run of m keys into: the first fills the chunk, the others chunk - carry."""
    out, base, have = [], 0, 0
    while base < m:
        take = min(m - base, chunk - have)
        out.append((base, base + take))
        have = min(have + take, k)
        base += take
    return out


def plant_event(m: int, k: int, chunk: int, mode: str, taken, rng):
    """(winner rows inside the event in rank order, ramp) of one question in one event of m rows."""
    avail = _free(np.arange(m, dtype=np.int64), taken)
    kw = min(k, len(avail))
    pieces = fold_pieces(m, k, chunk)
    if kw == 0:
        return avail[:0], 0
    if mode == "ascending":
        return avail[::-1][:kw].copy(), +1
    if mode == "descending":
        return avail[:kw].copy(), -1
    if mode == "first_piece":
        cand = avail[avail < pieces[0][1]]
    elif mode == "last_piece":
        cand = avail[avail >= pieces[-1][0]]
    else:                                                                  # across the first seam (the middle of a one-piece event)
        centre = pieces[0][1] - 0.5 if len(pieces) > 1 else m / 2
        cand = np.sort(avail[np.argsort(np.abs(avail - centre), kind="stable")[:kw]])
    if len(cand) < kw:                                                     # a last piece shorter than k: the last kw rows
        cand = avail[len(avail) - kw:]
    return rng.permutation(_spread(cand, kw)), 0


def plant_events(sizes, k: int, n_questions: int, mode_shift: int, seed: int = 0):
    """c (Q, sum sizes) fp64 and the winners per (question, event).  Question q uses mode (mode_shift + q) % 5 in every event;
    the background of an event is a ramp (the two ramp modes) or a shuffled ladder: distinct levels 1 / m apart, so that an event
    too small to hold every question's winners still has separated similarities."""
    chunk = event_chunk(sizes, k)
    scale = bg_scale(n_questions)
    c = np.zeros((n_questions, int(sum(sizes))))
    winners = {}
    lo = 0
    for e, m in enumerate(sizes):
        taken = np.zeros(0, np.int64)
        for q in range(n_questions):
            rng = np.random.default_rng(seed + 1000 * e + q)
            mode = EVENT_MODES[(mode_shift + q) % len(EVENT_MODES)]
            w, ramp = plant_event(m, k, chunk, mode, taken, rng)
            level = (np.arange(m) + 0.5) / max(m, 1) - 0.5
            c[q, lo:lo + m] = scale * (level[::ramp] if ramp else rng.permutation(level))
            c[q, lo + w] = winner_value(np.arange(len(w)), k)
            winners[q, e] = w
            taken = np.concatenate([taken, w])
        lo += m
    return c, winners


@dataclass(frozen=True)
class EventCase:
    route: str            # "segmented", "segmented_prefilter", "segmented_multi", "segmented_multi_prefilter"
    large: bool
    k: int
    mode_shift: int

    @property
    def id(self):
        return f"{self.route}-{'large' if self.large else 'small'}-k{self.k}-{EVENT_MODES[self.mode_shift]}"

    @property
    def n_questions(self):
        return 3 if "multi" in self.route else 1

    def sizes(self):
        return event_sizes(self.k, self.large)

    def plant(self):
        return plant_events(self.sizes(), self.k, self.n_questions, self.mode_shift)


@functools.lru_cache(maxsize=None)
def event_cases() -> tuple:
    out = []
    for route in ("segmented", "segmented_prefilter", "segmented_multi", "segmented_multi_prefilter"):
        for large in (False, True):
            for k in (5, 64):
                out += [EventCase(route, large, k, shift) for shift in range(len(EVENT_MODES))]
    for large in (False, True):                                            # the exact route's ANY_K sort (k > 64)
        out += [EventCase("segmented", large, 65, shift) for shift in range(len(EVENT_MODES))]
    return tuple(out)


# ---- hmm_rank_segment_hits: hand-made (E, k) hits ----------------------------------------------------------------------------------
RANK_PATTERNS = ("one_thread", "one_per_thread", "equal_in_one_thread", "full_window")


def rank_hits_case(pattern: str, extra_events: int):
    """(sims (E, 4) fp32, counts (E,), keep): E x 4 = the quick route's limit (+ 4 per extra event: the fold route).  The 64 best
    hits sit at the positions = 7 (mod 1024) -- all in thread 7 of select_ranked_hits -- or one per thread, or are 64 EQUAL
    similarities in thread 7 (the stable event order decides).  "full_window": besides, every hit of threads 0 .. 62 beats every hit
    of the other threads and thread 63 holds 64 equal hits just below them: the bound M is thread 63's first hit and 63 x 64 + 1
    keys reach it -- the quick route's candidate window (kChunk keys) is all but full."""
    c = source_constants()
    k, keep, threads = 4, 64, c["kRankThreads"]
    base_events = c["kRankQuickMax"] // k
    E = base_events + extra_events
    rng = np.random.default_rng(len(pattern) + extra_events)
    sims = rng.uniform(-1.0, 0.5, (E, k)).astype(np.float32)
    if pattern == "one_per_thread":
        pos = np.array([threads * j + (37 * j) % threads for j in range(keep)])
    else:
        pos = 7 + threads * np.arange(keep)
    assert pos.max() < base_events * k and len(set((pos % threads).tolist())) == (keep if pattern == "one_per_thread" else 1)
    if pattern == "full_window":
        every = np.arange(base_events * k)
        strong = every[every % threads < keep - 1]
        sims.reshape(-1)[strong] = rng.uniform(0.62, 0.7, len(strong)).astype(np.float32)
        sims.reshape(-1)[every[every % threads == keep - 1]] = np.float32(0.61)
    best = winner_value(rng.permutation(keep), keep).astype(np.float32)
    sims.reshape(-1)[pos] = np.float32(0.875) if pattern == "equal_in_one_thread" else best
    return sims, np.full(E, k, np.int32), keep
