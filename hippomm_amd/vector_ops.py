"""feature_search scan on MI355X -- host-side mirror of hippomm/utils/vector_ops.py.

``top_k_cosine_similarity(a, b, k)`` keeps the reference signature and return types
(vector_ops.py:151-188) and runs on the HIP kernels behind ``hmm_cosine_topk``.

The reference re-reads ``event.features[...]`` from host memory on every query
(hippocampal_memory.py:3153, :3304).  To keep the store resident in HBM between queries wrap
it once in a :class:`FeatureStore` (or pass a CUDA tensor); a numpy ``b`` is uploaded on every
call, which is correct but PCIe-bound.
"""
from __future__ import annotations

import functools
import logging
import math
import threading
import weakref
import zlib
try:                                     # xxh3: ~17 GB/s on one core (2 MB event matrix: 0.1 ms); zlib's CRC-32 is the ~1 GB/s fallback
    from xxhash import xxh3_64_intdigest as _content_hash
    _CONTENT_HASH = "xxh3_64"
except ImportError:                      # pragma: no cover - the image ships xxhash
    _content_hash = zlib.crc32
    _CONTENT_HASH = "crc32"
from typing import List, Tuple, Union

import numpy as np
import torch

from . import _lib

logger = logging.getLogger(__name__)

FEATURE_DIM = 1024

# The scan routes: (shape, through the bf16 shadow) -> (C entry point, its workspace-size function, takes a stats pointer).
# FeatureStore._scan assembles every argument list from these, in the one order the entry points share:
#   store, [shadow,] n, dim, queries, [Q,] [seg_offsets, E,] k, outputs..., [stats,] workspace, workspace bytes, stream
# and sizes the workspace with (n, [E,] [Q,] k).  "keys" is the flat scan that returns packed order keys; it has no shadow variant.
_ROUTES = {
    ("flat", False): ("hmm_cosine_topk", "hmm_cosine_topk_workspace_bytes", False),
    ("flat", True): ("hmm_cosine_topk_prefilter", "hmm_cosine_topk_prefilter_workspace_bytes", True),
    ("keys", False): ("hmm_cosine_topk_keys", "hmm_cosine_topk_workspace_bytes", False),
    ("segmented", False): ("hmm_cosine_topk_segmented", "hmm_cosine_topk_segmented_workspace_bytes", False),
    ("segmented", True): ("hmm_cosine_topk_segmented_prefilter", "hmm_cosine_topk_segmented_prefilter_workspace_bytes", False),
    ("multi", False): ("hmm_cosine_topk_multi", "hmm_cosine_topk_multi_workspace_bytes", False),
    ("multi", True): ("hmm_cosine_topk_multi_prefilter", "hmm_cosine_topk_multi_prefilter_workspace_bytes", True),
    ("segmented_multi", False): ("hmm_cosine_topk_segmented_multi", "hmm_cosine_topk_segmented_multi_workspace_bytes", False),
    ("segmented_multi", True): ("hmm_cosine_topk_segmented_multi_prefilter",
                                "hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes", True),
}


# The float64 route (exact64=True; include/hippomm_hip.h, "float64-origin stores") has its own entry points and argument order:
#   store, n, dim, queries, query dtype, query norms, [Q,] [seg_offsets, E,] k, outputs..., workspace, workspace bytes, stream
# and sizes the workspace with (n, [E,] [Q,] k).  One host path, FeatureStore._scan_f64, serves both tables: a single query is a
# (1,1024) batch with one norm, sent to the entry points that take no Q; a batch goes to those that take it.
_F64_ROUTES = {
    "flat": ("hmm_cosine_topk_f64", "hmm_cosine_topk_f64_workspace_bytes"),
    "segmented": ("hmm_cosine_topk_segmented_f64", "hmm_cosine_topk_segmented_f64_workspace_bytes"),
}
_F64_MULTI_ROUTES = {
    "flat": ("hmm_cosine_topk_multi_f64", "hmm_cosine_topk_multi_f64_workspace_bytes"),
    "segmented": ("hmm_cosine_topk_segmented_multi_f64", "hmm_cosine_topk_segmented_multi_f64_workspace_bytes"),
}

_I64, _F32, _I32 = (torch.int64, np.int64, 8), (torch.float32, np.float32, 4), (torch.int32, np.int32, 4)
_F64 = (torch.float64, np.float64, 8)


class _Packed:
    """Arrays laid out back to back in one uint8 buffer, so that the device writes them through ``device_views`` and the host
    reads them through ``host_views`` after ONE copy -- the same offsets on both sides.  fields: ((torch dtype, numpy dtype,
    item size), shape)."""

    def __init__(self, *fields):
        self.fields, self.offsets, self.nbytes = [], [], 0
        for (torch_dtype, numpy_dtype, size), shape in fields:
            end = self.nbytes + size * math.prod(shape)
            self.fields.append((self.nbytes, end, torch_dtype, numpy_dtype, shape if len(shape) > 1 else None))
            self.offsets.append(self.nbytes)
            self.nbytes = end

    def device_views(self, packed: torch.Tensor):                # a typed slice is 1-D already: only the others are reshaped
        return [packed[a:b].view(dtype) if shape is None else packed[a:b].view(dtype).view(shape)
                for a, b, dtype, _, shape in self.fields]

    def host_views(self, raw: np.ndarray):
        return [raw[a:b].view(dtype) if shape is None else raw[a:b].view(dtype).reshape(shape)
                for a, b, _, dtype, shape in self.fields]


@functools.lru_cache(maxsize=64)                                 # a caller's shapes repeat from call to call
def _hits_layout(*shape, sims=_F32):
    """idx | sims | counts of a segmented scan; shape = (E, k) or (Q, E, k).  The 8-byte fields come first."""
    return _Packed((_I64, shape), (sims, shape), (_I32, shape[:-1]))


def _hits_layout_f64(*shape):
    """_hits_layout of a segmented float64 scan: sims float64."""
    return _hits_layout(*shape, sims=_F64)


@functools.lru_cache(maxsize=64)
def _ranking_layout(*shape):
    """event | row | sim | count of a ranking; shape = (keep,) or (Q, keep), one count per question."""
    return _Packed((_I64, shape), (_I64, shape), (_F32, shape), (_I32, shape[:-1] or (1,)))


@functools.lru_cache(maxsize=64)
def _relevant_layout(*shape):
    """A filtered ranking: event | row | sim | count, then deferred events | their number | their counts; shape = (E, keep) or
    (Q, E, keep).  Everything the host needs to decide whether the deferred events' hits have to be read at all."""
    lead, (E, keep) = shape[:-2], shape[-2:]
    return _Packed((_I64, lead + (keep,)), (_I64, lead + (keep,)), (_F32, lead + (keep,)), (_I32, lead + (1,)),
                   (_I32, lead + (E,)), (_I32, lead + (1,)), (_I32, lead + (E,)))


@functools.lru_cache(maxsize=64)
def _deferred_layout(n_queries, cells):
    """The deferred events' own hits, compacted per question: idx (Q, E * k) | sims (Q, E * k)."""
    return _Packed((_I64, (n_queries, cells)), (_F32, (n_queries, cells)))


def _queries_2d(queries, device=None) -> torch.Tensor:
    """queries (numpy or torch) as a (Q,1024) tensor with Q >= 1; with ``device``, contiguous fp32 on it."""
    q = queries if isinstance(queries, torch.Tensor) else torch.from_numpy(np.asarray(queries))
    if q.dim() != 2 or q.shape[1] != FEATURE_DIM:
        raise ValueError(f"queries must be (Q,{FEATURE_DIM}), got {tuple(q.shape)}")
    if q.shape[0] == 0:
        raise ValueError("no queries")
    return q if device is None else q.detach().to(device=device, dtype=torch.float32).contiguous()


# ---- the float64 route: opt-in ---------------------------------------------------------------------------------------------------
# load_theta_event hands the reference float64 matrices, so its scans run in float64 (hippocampal_memory.py:387-395,
# vector_ops.py:178-186).  Such a matrix holds the repr digits of fp32 tower outputs: every value is an fp32 value, the resident
# fp32 rows lose nothing, and only the arithmetic differs.  With ``exact64=True`` (or, for the unchanged reference loop, after
# ``enable_exact64()``) a scan widens the rows in registers and accumulates in fp64 (hmm_cosine_topk_f64): similarities within
# 2^-42 of the exact quotient, float64 out.  OFF by default: every call then returns today's bits through today's kernels.
_EXACT64 = False
_warned_not_exact = False
EXACT64_TOL = 2.0 ** -42


def enable_exact64():
    """Let ``top_k_cosine_similarity`` take the float64 route wherever its result is float64 anyway (a float64 store or a float64
    query) and the store is eligible (every source value an fp32 value).  A float64 store that is not eligible logs one warning
    and keeps today's route.  For the unchanged reference loop, which cannot pass ``exact64=True``."""
    global _EXACT64
    _EXACT64 = True


def disable_exact64():
    global _EXACT64
    _EXACT64 = False


def first_not_f32(a: np.ndarray):
    """The flat offset of the first value of a float64 array whose bits differ from ``(double)(float)v``'s, or None when every
    value is an fp32 value (a NaN whose payload narrows exactly and an fp32 subnormal are).  What hmm_rows_f64_are_f32 reports."""
    flat = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        back = flat.astype(np.float32).astype(np.float64)
    bad = np.flatnonzero(back.view(np.uint64) != flat.view(np.uint64))
    return int(bad[0]) if bad.size else None


def _exact64_query(a, dev):
    """One query of any shape with 1024 elements as a batch of one: what ``_exact64_queries`` returns for its (1,1024) view."""
    a = a if isinstance(a, torch.Tensor) else np.asarray(a)
    if math.prod(a.shape) != FEATURE_DIM:
        raise ValueError(f"query must have {FEATURE_DIM} elements, got {math.prod(a.shape)}")
    return _exact64_queries(a.reshape(1, FEATURE_DIM), dev)


def _exact64_queries(queries, dev):
    """(buffer, address of the (Q,1024) batch, dtype code, address of the Q norms or None, Q) for the float64 entry points.
    A host batch keeps its dtype (float32 or float64; anything else becomes float32) and travels with one norm per question in the
    same upload, each ``np.linalg.norm(row)`` of the contiguous 1-D row evaluated by numpy in that dtype -- the reference's own
    ``a_norm``; ``norm(q, axis=1)`` sums along another path and need not give its bits.  A device batch is used where it lies and
    the kernel forms the norms (include/hippomm_hip.h: the last fp32 bit of an fp32 query's norm may then differ from numpy's).
    The batch starts at a 16-byte boundary either way."""
    if isinstance(queries, torch.Tensor) and queries.is_cuda:
        q = queries.detach()
        if q.dim() != 2 or q.shape[1] != FEATURE_DIM:
            raise ValueError(f"queries must be (Q,{FEATURE_DIM}), got {tuple(q.shape)}")
        if q.shape[0] == 0:
            raise ValueError("no queries")
        if q.dtype not in (torch.float32, torch.float64):
            q = q.to(torch.float32)
        q = q.to(dev).contiguous()
        if q.data_ptr() % 16:
            q = q.clone()
        return q, q.data_ptr(), int(q.dtype == torch.float64), None, q.shape[0]
    host = queries.detach().numpy() if isinstance(queries, torch.Tensor) else np.asarray(queries)
    if host.ndim != 2 or host.shape[1] != FEATURE_DIM:
        raise ValueError(f"queries must be (Q,{FEATURE_DIM}), got {tuple(host.shape)}")
    if host.shape[0] == 0:
        raise ValueError("no queries")
    host = np.ascontiguousarray(host, dtype=host.dtype if host.dtype in (np.float32, np.float64) else np.float32)
    Q = host.shape[0]
    norms = np.zeros(Q + (Q & 1), dtype=np.float64)                       # an even number of doubles: the batch behind them stays 16-byte aligned
    norms[:Q] = [np.linalg.norm(row) for row in host]                     # each in the query's dtype, widened
    buf = torch.from_numpy(np.concatenate([norms.view(np.uint8), host.reshape(-1).view(np.uint8)])).to(dev)
    if buf.data_ptr() % 16:                                               # a host buffer (no GPU in the process) may lie anywhere
        spare = torch.empty(buf.numel() + 16, dtype=torch.uint8, device=buf.device)
        skew = (-spare.data_ptr()) % 16
        spare[skew: skew + buf.numel()].copy_(buf)
        buf = spare[skew: skew + buf.numel()]
    return buf, buf.data_ptr() + norms.nbytes, int(host.dtype == np.float64), buf.data_ptr(), Q


def rank_hits_exact64(idx, sims, counts, keep: int, row_limits=None, defer=None, min_similarity: float = 0.4):
    """The reference's two per-event rules and its stable descending sort on the (E, k) float64 hits of a segmented scan, in numpy
    on the host -- the reference's own operations: ``sims[e, 0] < float(min_similarity)`` on doubles (a NaN never defers), the row
    rule ``idx < row_limits[e]``, then Python's stable sort by similarity (NaN first, the library's rule).  -> (hits, deferred)
    as ``EventStore.relevant_hits`` returns them, similarities float64."""
    idx, sims, counts = np.asarray(idx), np.asarray(sims, dtype=np.float64), np.asarray(counts)
    E, k = idx.shape
    threshold = float(min_similarity)
    deferred = [e for e in range(E) if defer is not None and defer[e] and counts[e] > 0 and sims[e, 0] < threshold]
    valid = np.arange(k)[None, :] < counts[:, None]
    if deferred:
        valid[deferred] = False
    if row_limits is not None:
        valid &= idx < np.asarray(row_limits, dtype=np.int64)[:, None]
    key = np.where(np.isnan(sims), np.inf, sims)
    cells = np.flatnonzero(valid.reshape(-1))                             # event order, then slot order
    down = -key.reshape(-1)[cells]
    if cells.size > 4 * keep:                                             # only cells at or above the keep-th key can be kept (ties included)
        at_least = down <= np.partition(down, keep - 1)[keep - 1]
        cells, down = cells[at_least], down[at_least]
    order = cells[np.argsort(down, kind="stable")][:keep]
    hits = [(int(c // k), int(idx.reshape(-1)[c]), float(sims.reshape(-1)[c])) for c in order]
    return hits, [(int(e), idx[e, :counts[e]].astype(np.int64), sims[e, :counts[e]].copy()) for e in deferred]


class FeatureStore:
    """(N,1024) fp32 feature matrix resident in HBM (the ``memory_store`` vision/audio matrix
    of one event, or many events concatenated), plus the scan workspace.

    ``f64_exact``: None for an fp32 source; for a float64 source True when every value was an fp32 value (narrowing lost nothing:
    the store is eligible for the float64 route) and False otherwise.  Conservative: once False it stays False until the store
    is rebuilt."""

    def __init__(self, rows: Union[np.ndarray, torch.Tensor], device=None, shadow: bool = False):
        """``shadow=True`` also builds the bf16 shadow (+2048 B per row) and lets ``search`` / ``search_device`` -- and therefore
        ``top_k_cosine_similarity(q, store, k)`` -- go through it: the same results, bit for bit, for half the bytes streamed.
        The rows must stay unchanged while a shadow exists (see ``build_shadow``)."""
        dev = device or _lib.require_gpu()
        source64 = None                                  # a float64 source, as it was handed in: checked once the state exists
        if isinstance(rows, np.ndarray):
            source_dtype = rows.dtype
            host = np.ascontiguousarray(rows.reshape(1, -1) if rows.ndim == 1 else rows, dtype=np.float32)
            t = torch.from_numpy(host).to(dev)
            if source_dtype == np.float64:
                source64 = rows
        else:
            source_dtype = np.dtype(str(rows.dtype).replace("torch.", "")) if rows.dtype in (
                torch.float32, torch.float64) else np.dtype(np.float32)
            t = rows.reshape(1, -1) if rows.dim() == 1 else rows
            if rows.dtype == torch.float64:
                source64 = t
            t = t.to(device=dev, dtype=torch.float32).contiguous()
        if t.dim() != 2 or t.shape[1] != FEATURE_DIM:
            raise ValueError(f"store must be (N,{FEATURE_DIM}), got {tuple(t.shape)}")
        self._init_state(t, source_dtype)
        if source64 is not None:
            self._note_f64_source(source64, 0)
        if shadow and t.shape[0] > 0:
            self.build_shadow()
            self.use_shadow = True

    def _init_state(self, rows: torch.Tensor, source_dtype):
        """Every field of a store, in one place (EventStore adds ``lengths`` and ``offsets``)."""
        self.rows, self.source_dtype = rows, source_dtype
        self.use_shadow = False                          # search / search_device go through the shadow
        self._shadow, self._shadow_version = None, None  # the bf16 shadow of `rows` and the torch version of `rows` it was built at
        self._ws = None                                  # the scan workspace every route shares (_scratch)
        self._buf, self._shadow_buf = None, None         # the capacity-sized buffers of a store that has grown (EventStore)
        self._pinned = None                              # the read-back staging buffer (EventStore._read_back)
        self._pinned_rules = None                        # the upload staging buffer of row_limits | defer (EventStore._upload_rules)
        self._f64_exact = None                           # see the f64_exact property
        self._f64_first_bad = None                       # (row in the store at ingest, column) of the first value that is no fp32 value
        self._f64_pending = []                           # [(device report int64[2], first row)] of checks not read back yet

    def __len__(self):
        return self.rows.shape[0]

    # ---- eligibility for the float64 route ------------------------------------------------------------------------------------
    def _note_f64_source(self, source, first_row: int):
        """AND one float64 source (rows ``first_row`` .. of the store) into ``f64_exact``: a host array is checked with numpy here,
        a device tensor by hmm_rows_f64_are_f32 on the current stream, beside the ingest; its report is read when somebody asks."""
        if isinstance(source, torch.Tensor) and source.is_cuda:
            src = source.detach().contiguous().reshape(-1, FEATURE_DIM)
            report = torch.empty(2, dtype=torch.int64, device=src.device)
            _lib.check(_lib.load().hmm_rows_f64_are_f32(src.data_ptr() if src.shape[0] else None, src.shape[0], FEATURE_DIM,
                                                        report.data_ptr(), _lib.stream_ptr()), "hmm_rows_f64_are_f32")
            self._f64_pending.append((report, int(first_row)))
            return
        at = first_not_f32(source.detach().numpy() if isinstance(source, torch.Tensor) else source)
        self._and_f64(at is None, None if at is None else (int(first_row) + at // FEATURE_DIM, at % FEATURE_DIM))

    def _and_f64(self, clean: bool, first_bad):
        if not clean and self._f64_exact is not False:
            self._f64_first_bad = first_bad
        self._f64_exact = bool(clean) if self._f64_exact is None else (self._f64_exact and bool(clean))

    @property
    def f64_exact(self):
        """None: only fp32 sources so far.  True: float64 sources, every value an fp32 value.  False: some float64 value was
        narrowed with a rounding; it stays False until the store is rebuilt (also after the event is removed).  Reading it brings
        back the reports of device-side checks still in flight (one small copy each)."""
        pending, self._f64_pending = self._f64_pending, []
        for report, first_row in pending:
            count, at = (int(v) for v in report.cpu().numpy())
            self._and_f64(count == 0, None if count == 0 else (first_row + at // FEATURE_DIM, at % FEATURE_DIM))
        return self._f64_exact

    def _use_exact64(self, exact64: bool, what: str, prefilter: bool = False) -> bool:
        """The explicit request: refused (ValueError) together with the bf16 shadow route and on a store that is not eligible."""
        if not exact64:
            return False
        if prefilter:
            raise ValueError(f"{what}: exact64=True does not go through the bf16 shadow (prefilter=True)")
        if self.f64_exact is False:
            row, col = self._f64_first_bad
            raise ValueError(f"{what}: exact64=True needs a store whose float64 source held fp32 values only; the value at "
                             f"(row {row}, column {col}) was not one")
        return True

    def _scan_f64(self, shape: str, batch, k: int, outputs, seg_offsets: torch.Tensor = None, single: bool = False):
        """One call of the float64 route ``shape`` into ``outputs`` (inside it one pass over the store per 16 questions);
        ``batch`` is what _exact64_queries returned.  ``single``: the single-query entry point of _F64_ROUTES, which takes no Q,
        instead of the batched one of _F64_MULTI_ROUTES.  Does not synchronise."""
        name, size_name = (_F64_ROUTES if single else _F64_MULTI_ROUTES)[shape]
        lib = _lib.load()
        _, q_ptr, q_dtype, norms_ptr, Q = batch
        n, count = len(self), () if single else (Q,)
        segments = () if seg_offsets is None else (seg_offsets.data_ptr(), seg_offsets.numel() - 1)
        ws = self._scratch(getattr(lib, size_name)(n, *segments[1:], *count, k))
        _lib.check(getattr(lib, name)(self.rows.data_ptr(), n, FEATURE_DIM, q_ptr, q_dtype, norms_ptr, *count, *segments, k,
                                      *[t.data_ptr() for t in outputs], ws.data_ptr(), ws.numel(), _lib.stream_ptr()), name)

    def _search_flat_f64(self, queries, k: int, single: bool = False):
        """The float64 route of search_multi_device: (idx (Q,k') int64, sims (Q,k') float64), k' = min(k, N); ``single``: of
        search_device, without the leading Q.  An empty store launches nothing (and a single query is then not looked at)."""
        if int(k) < 1:
            raise ValueError("k must be >= 1")
        dev, k_out = self.rows.device, min(int(k), len(self))
        batch = None if single and k_out == 0 else (_exact64_query if single else _exact64_queries)(queries, dev)
        lead = () if single else (batch[-1],)
        idx = torch.empty(*lead, k_out, dtype=torch.int64, device=dev)
        sims = torch.empty(*lead, k_out, dtype=torch.float64, device=dev)
        n_out = torch.empty(*lead or (1,), dtype=torch.int32, device=dev)
        if k_out > 0:
            self._scan_f64("flat", batch, int(k), (idx, sims, n_out), single=single)
        return idx, sims

    def _scratch(self, need_bytes: int) -> torch.Tensor:
        """The workspace, reallocated only when it is too small.  No route reads what an earlier call left in it."""
        if self._ws is None or self._ws.numel() < need_bytes:
            self._ws = torch.empty(need_bytes, dtype=torch.uint8, device=self.rows.device)
        return self._ws

    def _scan(self, shape: str, prefilter: bool, queries: torch.Tensor, k: int, outputs, Q: int = None,
              seg_offsets: torch.Tensor = None, stats: torch.Tensor = None):
        """One launch of the route (shape, prefilter) of _ROUTES into ``outputs`` (the tensors the entry point fills, in its
        order).  Builds the shadow when the route streams it; does not synchronise."""
        name, size_name, takes_stats = _ROUTES[shape, prefilter]
        lib = _lib.load()
        if prefilter:
            self.build_shadow()
        n = len(self)
        batch = () if Q is None else (Q,)
        segments = () if seg_offsets is None else (seg_offsets.data_ptr(), seg_offsets.numel() - 1)
        ws = self._scratch(getattr(lib, size_name)(n, *segments[1:], *batch, k))
        store = (self.rows.data_ptr(), self._shadow.data_ptr()) if prefilter else (self.rows.data_ptr(),)
        tail = (stats.data_ptr() if stats is not None else None,) if takes_stats else ()
        _lib.check(getattr(lib, name)(*store, n, FEATURE_DIM, queries.data_ptr(), *batch, *segments, k,
                                      *[t.data_ptr() for t in outputs], *tail, ws.data_ptr(), ws.numel(), _lib.stream_ptr()), name)

    def _search_flat(self, query: torch.Tensor, k: int, prefilter: bool, stats: torch.Tensor = None):
        if k < 1:
            raise ValueError("k must be >= 1")
        dev, k_out = self.rows.device, min(k, len(self))
        idx = torch.empty(k_out, dtype=torch.int64, device=dev)
        sims = torch.empty(k_out, dtype=torch.float32, device=dev)
        n_out = torch.empty(1, dtype=torch.int32, device=dev)
        self._scan("flat", prefilter, query, k, (idx, sims, n_out), stats=stats)
        return idx, sims

    def search_device(self, query: torch.Tensor, k: int, exact64: bool = False):
        """query: (1024,) fp32 CUDA tensor.  Returns CUDA tensors (idx int64[k'], sims fp32[k'])
        without synchronising (k' = min(k, N)).  ``exact64=True``: the float64 route (hmm_cosine_topk_f64) -- the query may be
        fp32 or fp64, on the host or the device, sims are float64 within 2^-42 of the exact quotient; never through the shadow."""
        if self._use_exact64(exact64, "search_device"):
            return self._search_flat_f64(query, k, single=True)
        if self.use_shadow:
            return self.search_prefiltered_device(query, k)
        return self._search_flat(query, k, False)

    def _rows_version(self) -> int:
        try:
            return self.rows._version
        except (RuntimeError, AttributeError):       # an inference tensor tracks no version: a snapshot until invalidate_shadow()
            return 0

    def _shadow_is_current(self) -> bool:
        """True when a shadow exists and matches the rows.  A stale one (the rows were edited through torch since) is dropped:
        the next prefiltered search rebuilds it whole, as it would have anyway."""
        if self._shadow is not None and self._shadow_version != self._rows_version():
            self.invalidate_shadow()
        return self._shadow is not None

    def build_shadow(self, force: bool = False):
        """Build the bf16 shadow of the store (2048 B per row beside the 4096-B fp32 rows; hmm_shadow_store_build) that
        ``search_prefiltered_device`` streams.  Idempotent unless ``force``.

        The shadow is a SNAPSHOT: ``self.rows`` must not change while it exists (``FeatureStore`` / ``from_device_rows`` alias
        a caller's fp32 CUDA tensor without copying).  An in-place update made through torch bumps the tensor's version
        counter, which the searches check: the shadow is then rebuilt before it is used.  Writes that bypass torch (a raw
        kernel on ``rows.data_ptr()``) need ``invalidate_shadow()`` or ``build_shadow(force=True)``.  The build is enqueued
        on the current stream; searches on another stream must be ordered after it by the caller.

        On a store that owns its buffers (an EventStore that has grown) the shadow is built into the capacity-sized buffer, where
        later appends keep it current row by row (an append never rebuilds it).  The ingest and the gather write rows behind
        torch's back AND their shadow rows with them, so the version the shadow was built at stays the one it is checked
        against; edits of ``rows`` made through torch still bump it and cause a rebuild."""
        version = self._rows_version()
        if force or self._shadow is None or self._shadow_version != version:
            n, owned = len(self), self._buf is not None
            buf = self._shadow_buf if owned else self._shadow
            size = self._buf.shape[0] * 2048 if owned else _lib.load().hmm_shadow_store_bytes(n)
            if buf is None or buf.numel() != size:
                buf = torch.empty(size, dtype=torch.uint8, device=self.rows.device)
            if owned:
                self._shadow_buf = buf
            if n > 0 or not owned:                       # without rows an owned store launches nothing; an aliased one lets the library refuse
                _lib.check(_lib.load().hmm_shadow_store_build(self.rows.data_ptr(), n, FEATURE_DIM, buf.data_ptr(), n * 2048,
                                                              _lib.stream_ptr()), "hmm_shadow_store_build")
            self._shadow = buf[: n * 2048]
            self._shadow_version = version
        return self

    def invalidate_shadow(self):
        """Forget the bf16 shadow (after the fp32 rows were modified behind torch's back); the next prefiltered search
        rebuilds it."""
        self._shadow = None
        return self

    def search_prefiltered_device(self, query: torch.Tensor, k: int, stats: torch.Tensor = None):
        """``search_device`` through the bf16 shadow: candidates from one pass over 2048 B per row, re-scored exactly on the
        fp32 rows -- the same (idx, sims) as ``search_device``, bit for bit (hmm_cosine_topk_prefilter).  ``stats``: optional
        int32[2] CUDA tensor receiving (candidates re-scored, saturated lists)."""
        return self._search_flat(query, k, True, stats)

    def search_keys_device(self, query: torch.Tensor, k: int) -> torch.Tensor:
        """Local top-k as packed order keys (uint64 bit patterns in an int64 tensor, 0-padded to k)
        for the sharded scan (hippomm_amd.sharding.sharded_top_k)."""
        keys = torch.empty(k, dtype=torch.int64, device=self.rows.device)
        self._scan("keys", False, query, k, (keys,))
        return keys

    def search_segments_device(self, query: torch.Tensor, seg_offsets: torch.Tensor, k: int, prefilter: bool = False,
                               exact64: bool = False):
        """Per-event top-k in one pass.  seg_offsets: int64 CUDA tensor (E+1,), row offsets of the events inside
        this store.  Returns CUDA tensors idx (E,k) int64 rows within each event (-1 padded), sims (E,k) fp32,
        counts (E,) int32 = min(k, n_e).  ``prefilter``: stream the bf16 shadow (built on first use) and re-score each event's
        candidates on the fp32 rows -- the same outputs, bit for bit, for half the bytes (hmm_cosine_topk_segmented_prefilter).
        ``exact64=True``: the float64 route (hmm_cosine_topk_segmented_f64): sims (E,k) float64, every event's slice what the flat
        float64 call gives on its rows, bit for bit; not together with ``prefilter``."""
        exact64 = self._use_exact64(exact64, "search_segments_device", prefilter)
        return self._search_segments_packed(query, seg_offsets, k, prefilter, single=True, exact64=exact64)[1:]

    def _search_segments_packed(self, queries, seg_offsets: torch.Tensor, k: int, prefilter: bool = False, stats: torch.Tensor = None,
                                single: bool = False, exact64: bool = False):
        """search_segments_multi_device -- or, ``single``, search_segments_device for one query -- returning (packed, idx, sims,
        counts): the three outputs are views of ONE buffer (_hits_layout), so that a caller who wants them on the host reads them
        back with one copy.  Through the fp32 rows, the bf16 shadow (``prefilter``) or the float64 route (``exact64``: sims float64;
        the queries as _exact64_queries takes them, otherwise fp32 on the device for ``single``).  A batch without events or
        without rows launches nothing: the padding is the answer.  A single query always goes to its entry point, which refuses
        E == 0 and k < 1 itself (on the fp32 routes) and pads the events of a store without rows."""
        k, dev, E = int(k), self.rows.device, seg_offsets.numel() - 1
        batch = queries if single or exact64 else _queries_2d(queries, dev)
        if k < 1 and (exact64 or not single):
            raise ValueError("k must be >= 1")
        if exact64:
            batch = (_exact64_query if single else _exact64_queries)(queries, dev)
        Q = None if single else (batch[-1] if exact64 else batch.shape[0])
        layout = _hits_layout(*(() if single else (Q,)), E, k, sims=_F64 if exact64 else _F32)
        packed = torch.empty(layout.nbytes, dtype=torch.uint8, device=dev)
        idx, sims, counts = layout.device_views(packed)
        if not single and (E == 0 or len(self) == 0):
            idx.fill_(-1)
            sims.zero_()
            counts.zero_()
        elif exact64:
            self._scan_f64("segmented", batch, k, (idx, sims, counts), seg_offsets=seg_offsets, single=single)
        else:
            self._scan("segmented" if single else "segmented_multi", bool(prefilter and len(self) > 0), batch, k, (idx, sims, counts),
                       Q=Q, seg_offsets=seg_offsets, stats=stats)
        return packed, idx, sims, counts

    def search_segments_multi_device(self, queries, seg_offsets: torch.Tensor, k: int, prefilter: bool = False,
                                     stats: torch.Tensor = None, exact64: bool = False):
        """``search_segments_device`` for a batch of questions in one pass over the store per 16 of them
        (hmm_cosine_topk_segmented_multi).  queries: (Q,1024) numpy or torch, any device, fp32 or fp64.  Returns CUDA tensors
        idx (Q,E,k) int64 rows within each event (-1 padded), sims (Q,E,k) fp32, counts (Q,E) int32 = min(k, n_e), without
        synchronising.  ``prefilter``: stream the bf16 shadow (built on first use) and re-score each event's candidates on the
        fp32 rows -- the same outputs, bit for bit (hmm_cosine_topk_segmented_multi_prefilter); ``stats``: optional int32[2]
        CUDA tensor receiving ((event, question) pairs that re-scored the whole event, rows re-scored), -1 / -1 when the exact
        function was the whole call.  ``exact64=True``: the float64 route for the batch (hmm_cosine_topk_segmented_multi_f64): sims
        (Q,E,k) float64, slice q what ``search_segments_device(queries[q], ..., exact64=True)`` returns, bit for bit; the batch is
        all fp32 or all fp64; not together with ``prefilter``."""
        exact64 = self._use_exact64(exact64, "search_segments_multi_device", bool(prefilter))
        return self._search_segments_packed(queries, seg_offsets, k, prefilter, stats, exact64=exact64)[1:]

    def search_multi_device(self, queries: torch.Tensor, k: int, prefilter: bool = None, stats: torch.Tensor = None,
                            exact64: bool = False):
        """queries (Q,1024) fp32 on the store's device -> (idx (Q,k') int64, sims (Q,k') fp32) device tensors,
        k' = min(k, N).  One pass over the store per 16 queries (hmm_cosine_topk_multi).  ``prefilter=True``: one pass over the
        bf16 shadow instead, candidates re-scored on the fp32 rows -- the same outputs, bit for bit
        (hmm_cosine_topk_multi_prefilter).  ``None`` is the exact pass even on a store built with ``shadow=True``: the shadow
        route has not been timed against it yet, and the results are the same either way; ``stats``: optional int32 (Q,2) CUDA tensor receiving per
        question (candidates re-scored, saturated lists), -1 / -1 when the exact function was the whole call.
        ``exact64=True``: the float64 route for the batch (hmm_cosine_topk_multi_f64), one pass per 16 queries: sims (Q,k') float64,
        row q what ``search_device(queries[q], k, exact64=True)`` returns, bit for bit; the batch may be fp32 or fp64, on the host
        or the device; not together with ``prefilter``."""
        if self._use_exact64(exact64, "search_multi_device", bool(prefilter)):
            return self._search_flat_f64(queries, k)
        queries = _queries_2d(queries, self.rows.device)
        nq, n, dev = queries.shape[0], len(self), self.rows.device
        idx = torch.empty(nq, k, dtype=torch.int64, device=dev)
        sims = torch.empty(nq, k, dtype=torch.float32, device=dev)
        n_out = torch.empty(nq, dtype=torch.int32, device=dev)
        # prefilter None: not self.use_shadow until tools/multi_prefilter_probe.py has placed the limits
        self._scan("multi", bool(prefilter and n > 0), queries, k, (idx, sims, n_out), Q=nq, stats=stats)
        kk = min(k, n)
        return idx[:, :kk], sims[:, :kk]

    def search_multi(self, queries, k: int, prefilter: bool = None, exact64: bool = False) -> List[Tuple[np.ndarray, np.ndarray]]:
        """Per query the (indices int64, similarities) pair top_k_cosine_similarity would return.  ``prefilter``: see
        ``search_multi_device``.  ``exact64=True``: per query what ``search(query, k, exact64=True)`` returns, float64, from one
        pass over the store per 16 queries; a host batch is sent with numpy's own norm of every row."""
        if self._use_exact64(exact64, "search_multi", bool(prefilter)):
            idx, sims = (t.cpu().numpy() for t in self._search_flat_f64(queries, k))
            return [(idx[i], sims[i]) for i in range(idx.shape[0])]
        q = queries if isinstance(queries, torch.Tensor) else torch.from_numpy(np.asarray(queries, dtype=np.float32))
        idx, sims = self.search_multi_device(q.reshape(-1, FEATURE_DIM), k, prefilter)
        idx, sims = idx.cpu().numpy(), sims.cpu().numpy()
        return [(idx[i], sims[i]) for i in range(idx.shape[0])]

    def search(self, query, k: int, exact64: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """``search_device`` with the results on the host.  ``exact64=True``: float64 similarities from the float64 route; a
        host query is sent with numpy's own ``np.linalg.norm`` of it, the reference's ``a_norm``."""
        if self._use_exact64(exact64, "search"):
            idx, sims = self._search_flat_f64(query, k, single=True)
        else:
            idx, sims = self.search_device(_query_to_device(query, self.rows.device), k)
        return idx.cpu().numpy(), sims.cpu().numpy()


def merge_keys_device(keys: torch.Tensor, row_offsets: torch.Tensor, k: int):
    """keys: (n_shards, k) int64 CUDA (packed order keys); row_offsets: (n_shards,) int64 CUDA."""
    lib = _lib.load()
    n_shards = keys.shape[0]
    dev = keys.device
    idx = torch.empty(k, dtype=torch.int64, device=dev)
    sims = torch.empty(k, dtype=torch.float32, device=dev)
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.hmm_topk_merge_keys(keys.contiguous().data_ptr(), n_shards, k, row_offsets.data_ptr(),
                                       idx.data_ptr(), sims.data_ptr(), n_out.data_ptr(), _lib.stream_ptr()),
               "hmm_topk_merge_keys")
    n = int(n_out.item())
    return idx[:n], sims[:n]


# ---- optional residency for the UNCHANGED reference loop ----------------------------------------------------------------------
# The reference calls top_k_cosine_similarity(query, event.features['vision'], k=5) once per event and question with the event's
# host array (hippocampal_memory.py:3143-3153): as a drop-in that is a host-side fp32 conversion plus an upload per call (~1 ms
# per event).  With the cache enabled a numpy store seen before is served from its resident FeatureStore.  OFF by default.
# What it assumes: an array modified IN PLACE between two calls is noticed through a fingerprint of its contents -- a 64-bit
# hash of EVERY byte (xxh3, ~17 GB/s on one host core: 0.1 ms for a 500-frame event; CRC-32 when xxhash is absent) for arrays up
# to 64 MB (the reference's per-event matrices are 0.1-3 MB), and only a 64-row x 16-column sample (plus buffer address, shape,
# dtype, strides) above that, where a write to an unsampled element returns results from the stale HBM copy.
_STORE_CACHE = None
FULL_FINGERPRINT_BYTES = 64 << 20


class _StoreCache:
    def __init__(self, max_bytes: int, full_fingerprint_bytes: int = FULL_FINGERPRINT_BYTES):
        self.max_bytes, self.bytes, self.entries, self.hits, self.misses = int(max_bytes), 0, {}, 0, 0
        self.full_fingerprint_bytes = int(full_fingerprint_bytes)
        self._lock = threading.RLock()           # entries / bytes are also touched by weak-reference callbacks (any thread)

    def fingerprint(self, b: np.ndarray):
        head = (b.ctypes.data, b.shape, b.dtype.str, b.strides)
        if b.nbytes <= self.full_fingerprint_bytes:
            flat = b if b.flags.c_contiguous else np.ascontiguousarray(b)
            return head + (_CONTENT_HASH, _content_hash(memoryview(flat).cast("B")))
        rows = b.reshape(1, -1) if b.ndim == 1 else b
        pick = np.unique(np.linspace(0, rows.shape[0] - 1, num=min(rows.shape[0], 64)).astype(np.int64))
        return head + ("sampled", hash(np.ascontiguousarray(rows[pick][:, ::64]).tobytes()))

    def get(self, b: np.ndarray) -> "FeatureStore":
        key, fp = id(b), self.fingerprint(b)
        with self._lock:
            ent = self.entries.get(key)
            if ent is not None and ent[0]() is b and ent[2] == fp:
                self.hits += 1
                self.entries[key] = self.entries.pop(key)            # most recently used last
                return ent[1]
            if ent is not None:
                self._drop(key)
            self.misses += 1
        store = FeatureStore(b)
        size = store.rows.numel() * 4
        with self._lock:
            self._drop(key)                      # another thread may have inserted the same array while this one was uploading
            while self.entries and self.bytes + size > self.max_bytes:
                self._drop(next(iter(self.entries)))
            # the weak reference's callback releases the HBM copy when the host array dies
            self.entries[key] = (weakref.ref(b, lambda _r, k=key: self._drop(k)), store, fp, size)
            self.bytes += size
        return store

    def _drop(self, key):
        with self._lock:
            ent = self.entries.pop(key, None)
            if ent is not None:
                self.bytes -= ent[3]


def enable_store_cache(max_bytes: int = 8 << 30, full_fingerprint_bytes: int = FULL_FINGERPRINT_BYTES):
    """Keep the feature matrices that ``top_k_cosine_similarity`` receives as numpy arrays resident in HBM between calls (up to
    ``max_bytes`` of fp32 rows, least recently used first out): the reference's per-event loop then runs unchanged at the
    resident-store rate.

    Staleness: every call fingerprints the host array.  Arrays of at most ``full_fingerprint_bytes`` (default 64 MB; the
    reference's per-event matrices are 0.1-3 MB) are hashed WHOLE (xxh3 of every byte), so any in-place edit is a miss and
    the array is uploaded again.  Larger arrays are fingerprinted by a 64-row x 16-column sample plus address / shape / dtype /
    strides only: an in-place write to an unsampled element of such an array is NOT noticed and the answer comes from the
    stale resident copy -- wrap big stores in a ``FeatureStore`` yourself instead of relying on the cache."""
    global _STORE_CACHE
    _STORE_CACHE = _StoreCache(max_bytes, full_fingerprint_bytes)
    return _STORE_CACHE


def disable_store_cache():
    global _STORE_CACHE
    _STORE_CACHE = None


def _query_to_device(a, dev) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        q = a.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    else:
        q = torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.float32)).to(dev)
    if q.numel() != FEATURE_DIM:
        raise ValueError(f"query must have {FEATURE_DIM} elements, got {q.numel()}")
    return q


def top_k_cosine_similarity(
    a: Union[np.ndarray, torch.Tensor],
    b: Union[np.ndarray, torch.Tensor, FeatureStore],
    k: int,
    exact64: bool = False,
) -> Tuple[np.ndarray, np.ndarray]:
    """Top-k cosine similarities between one vector and many (reference vector_ops.py:151-188).

    a: (1024,) query (numpy or torch); b: (N,1024) store (numpy, torch, or a resident
    FeatureStore; a 1-D b is one row, as at :173-174).  Returns (indices int64[k'],
    similarities[k']), k' = min(k, N) (k = 0: all N rows, k < 0: N - |k| rows, as the reference's slice gives), best first;
    similarities are float64 when either input was
    float64 (numpy's promotion at :182) and float32 otherwise.  Ties: higher row index first; a zero-norm
    row yields NaN and ranks first, as in the reference.  (The reference leaves the order INSIDE a tie group to numpy's
    unstable argsort; this total order is the library's own rule, include/hippomm_hip.h.)

    By default a float64 result holds fp32 arithmetic widened.  ``exact64=True`` takes the float64 route instead: the resident
    fp32 rows widened in registers, sums in fp64, ``a_norm`` numpy's own for a host query -- similarities within 2^-42 of the exact
    quotient and float64 whatever the inputs' dtypes, hence the reference's ranking of near-ties.  It needs a store whose float64
    source held fp32 values only (``FeatureStore.f64_exact``; a reloaded event does): otherwise ValueError naming the first
    offending (row, column).  ``enable_exact64()`` makes the same choice for every call whose result is float64 anyway, falling
    back to today's route, with one logged warning, for a store that is not eligible.
    """
    a_is64 = (isinstance(a, np.ndarray) and a.dtype == np.float64) or (
        isinstance(a, torch.Tensor) and a.dtype == torch.float64)
    if not isinstance(b, FeatureStore) and getattr(b, "ndim", 2) == 2 and len(b) == 0:
        n, b_is64 = 0, str(getattr(b, "dtype", "")).endswith("float64")
    else:
        if isinstance(b, FeatureStore):
            store = b
        elif _STORE_CACHE is not None and isinstance(b, np.ndarray):
            store = _STORE_CACHE.get(b)
        else:
            store = FeatureStore(b)
        n, b_is64 = len(store), store.source_dtype == np.float64
    # the reference slices argsort(sims)[-k:][::-1] (:185): k = 0 keeps everything ([-0:]), k < 0 the best N - |k| rows
    k = int(k)
    k_eff = n if k == 0 else (max(n + k, 0) if k < 0 else min(k, n))
    out_dtype = np.float64 if (a_is64 or b_is64 or exact64) else np.float32
    if k_eff == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=out_dtype)
    if not exact64 and _EXACT64 and out_dtype == np.float64:     # the module-wide switch: only where the result is float64 anyway
        exact64 = store.f64_exact is not False
        if not exact64:
            global _warned_not_exact
            if not _warned_not_exact:
                _warned_not_exact = True
                logger.warning("top_k_cosine_similarity: a float64 store holds values that are not fp32 values (first at row %d, "
                               "column %d); it keeps the fp32 route", *store._f64_first_bad)
    if exact64:
        idx, sims = store.search(a, k_eff, exact64=True)
        return idx.astype(np.int64, copy=False), sims.astype(np.float64, copy=False)
    idx, sims = store.search(a, k_eff)
    return idx.astype(np.int64, copy=False), sims.astype(out_dtype, copy=False)


def _index_of(i, E: int) -> int:
    """Event index ``i`` (negative ones count from the end) as 0 <= j < E."""
    j = int(i)
    if j != i or not -E <= j < E:
        raise IndexError(f"event index {i!r} out of range for {E} events")
    return j + E if j < 0 else j


class EventStore(FeatureStore):
    """All events' feature matrices of one modality concatenated in HBM, with their row offsets: what
    ``QARecallSystem._find_relevant_*_segments`` iterates over (hippocampal_memory.py:3143, :3294)."""

    def __init__(self, event_features, device=None):
        event_features = list(event_features)
        mats =[np.ascontiguousarray(np.asarray(f).reshape(-1, FEATURE_DIM), dtype=np.float32) for f in event_features]
        lengths = [m.shape[0] for m in mats]
        super().__init__(np.concatenate(mats, axis=0) if sum(lengths) else np.zeros((0, FEATURE_DIM), np.float32), device)
        self._set_events(lengths)
        at = 0
        for f, n in zip(event_features, lengths):                # the float64 events, as they were handed in (host arrays: numpy)
            if getattr(f, "dtype", None) in (np.float64, torch.float64) and n > 0:
                self._note_f64_source(f.detach().cpu() if isinstance(f, torch.Tensor) else np.asarray(f), at)
            at += n

    @classmethod
    def from_device_rows(cls, rows: torch.Tensor, lengths) -> "EventStore":
        """An EventStore over a (N,1024) fp32 matrix that is already resident (events = consecutive row ranges of the
        given lengths); nothing is copied."""
        if rows.dim() != 2 or rows.shape[1] != FEATURE_DIM or rows.dtype != torch.float32 or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous (N,1024) fp32 tensor")
        lengths = [int(n) for n in lengths]
        if sum(lengths) != rows.shape[0]:
            raise ValueError(f"event lengths sum to {sum(lengths)}, store has {rows.shape[0]} rows")
        self = cls.__new__(cls)
        self._init_state(rows, np.dtype(np.float32))
        self._set_events(lengths)
        return self

    def _set_events(self, lengths):
        self.lengths = lengths
        self.offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=self.rows.device)

    def _hits_exact64(self, queries, k: int, single: bool = False):
        """The per-event float64 top-k on the device and ONE packed read-back -> host (idx (Q,E,k) int64, sims (Q,E,k) float64,
        counts (Q,E) int32), copies; ``single``: of one query, without the leading Q."""
        packed, idx, _, _ = self._search_segments_packed(queries, self.offsets, k, single=single, exact64=True)
        idx_h, sims_h, counts_h = _hits_layout_f64(*idx.shape).host_views(self._read_back(packed))
        return idx_h.copy(), sims_h.copy(), counts_h.copy()

    def top_hits(self, query, k: int = 5, keep: int = 5, prefilter: bool = False, exact64: bool = False):
        """The caller's whole step in one go (hippocampal_memory.py:3143-3153 + :3275-3277): top-k per event, then every hit of
        every event ranked by similarity and the best `keep` returned as [(event index, row inside the event, similarity)].
        The ranking runs on the device (a stable descending sort of the (E, k) similarities in event order, i.e. what Python's
        stable ``sorted(..., reverse=True)`` does to the list the reference builds event by event); only `keep` hits are read
        back.  NaN similarities (zero-norm rows) rank first, as they do per event.  This IS the reference's answer only on a store
        where every row of every event is a kept row and no event has captions / a transcription: the reference drops hits of
        rows that were not kept and defers low-similarity events to the LLM BEFORE its sort -- ``relevant_hits`` applies both.

        ``exact64=True``: the per-event top-k runs on the device in float64 (hmm_cosine_topk_segmented_f64), one packed read-back
        brings (idx, sims float64, counts), and the stable descending sort runs on the host in numpy (``rank_hits_exact64``) --
        the reference's own operation on doubles.  Ranking doubles on the device is a follow-up, not part of this route."""
        if self._use_exact64(exact64, "top_hits", prefilter):
            if not self.lengths or int(keep) < 1:
                return []
            return rank_hits_exact64(*self._hits_exact64(query, k, single=True), int(keep))[0]
        q = _query_to_device(query, self.rows.device)
        idx, sims, counts = self.search_segments_device(q, self.offsets, int(k), prefilter)
        E, keep = idx.shape[0], int(keep)
        if E == 0 or keep < 1:
            return []
        if keep > 64:                                           # beyond the ranking kernel's tournament width: torch's stable sort
            slot = torch.arange(idx.shape[1], device=idx.device).unsqueeze(0)
            valid = slot < counts.unsqueeze(1)
            key = torch.where(valid, torch.nan_to_num(sims, nan=float("inf")), torch.full_like(sims, float("-inf"))).reshape(-1)
            order = torch.sort(key, descending=True, stable=True).indices[:keep]
            order = order[valid.reshape(-1)[order]]
            flat_idx, flat_sims = idx.reshape(-1)[order], sims.reshape(-1)[order]
            hits = torch.stack([(order // idx.shape[1]).double(), flat_idx.double(), flat_sims.double()]).cpu().numpy()
            return [(int(e), int(r), float(np.float32(v))) for e, r, v in zip(hits[0], hits[1], hits[2])]
        # one launch ranks the (E, k) hits (hmm_rank_segment_hits), one copy brings the `keep` best back (_ranking_layout)
        layout = _ranking_layout(keep)
        packed = torch.empty(layout.nbytes, dtype=torch.uint8, device=idx.device)
        _lib.check(_lib.load().hmm_rank_segment_hits(idx.data_ptr(), sims.data_ptr(), counts.data_ptr(), E, idx.shape[1], keep,
                                                     *[t.data_ptr() for t in layout.device_views(packed)], _lib.stream_ptr()),
                   "hmm_rank_segment_hits")
        ev_h, row_h, val_h, n = layout.host_views(packed.cpu().numpy())
        return [(int(ev_h[t]), int(row_h[t]), float(val_h[t])) for t in range(int(n[0]))]

    def top_k_per_event(self, query, k: int = 5, prefilter: bool = False, exact64: bool = False):
        """[(indices int64[k_e], sims float32[k_e]) for every event], each exactly what
        ``top_k_cosine_similarity(query, event_features, k)`` returns for that event.  ``exact64=True``: sims float64, what
        ``top_k_cosine_similarity(query, event_features, k, exact64=True)`` returns for it, bit for bit."""
        if self._use_exact64(exact64, "top_k_per_event", prefilter):
            if not self.lengths:
                return []
            idx_h, sims_h, counts_h = self._hits_exact64(query, k, single=True)
            return [(idx_h[e, :counts_h[e]], sims_h[e, :counts_h[e]]) for e in range(len(self.lengths))]
        q = _query_to_device(query, self.rows.device)
        packed, idx, _, _ = self._search_segments_packed(q, self.offsets, k, prefilter, single=True)
        E, k = idx.shape
        if E == 0:
            return []
        # one copy of the packed (idx | sims | counts) buffer into pinned memory instead of three synchronising .cpu() calls
        idx_h, sims_h, counts_h = _hits_layout(E, k).host_views(self._read_back(packed))
        idx_h, sims_h = idx_h.copy(), sims_h.copy()
        if int(counts_h.min()) == k:                             # every event has k rows: plain row views, no slicing
            return list(zip(idx_h, sims_h))
        return [(idx_h[e, :counts_h[e]], sims_h[e, :counts_h[e]]) for e in range(E)]

    def _read_back(self, packed: torch.Tensor, *more: torch.Tensor) -> np.ndarray:
        """One copy of a packed device buffer into pinned memory; the bytes are valid until the next read-back.  With ``more``:
        every part (any dtype, possibly a strided slice) is copied behind the one before it, then ONE synchronisation."""
        parts = (packed,) + more
        sizes = [p.numel() * p.element_size() for p in parts]
        nbytes = sum(sizes)
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=packed.is_cuda)
        host, at = self._pinned[:nbytes], 0
        for part, size in zip(parts, sizes):
            host[at: at + size].view(part.dtype).view(part.shape).copy_(part, non_blocking=True)
            at += size
        if packed.is_cuda:
            torch.cuda.current_stream(packed.device).synchronize()
        return host.numpy()

    def top_k_per_event_multi(self, queries, k: int = 5, prefilter: bool = False, exact64: bool = False):
        """``top_k_per_event`` for a batch of questions: per query the list that ``top_k_per_event(query, k)`` returns, from one
        pass over the store per 16 questions and one read-back.  ``prefilter``: through the bf16 shadow, the same results
        (``search_segments_multi_device``).  ``exact64=True``: per query what ``top_k_per_event(query, k, exact64=True)`` returns,
        sims float64, bit for bit."""
        q = _queries_2d(queries)
        Q, E, k = q.shape[0], len(self.lengths), int(k)
        if self._use_exact64(exact64, "top_k_per_event_multi", prefilter):
            if E == 0 or len(self) == 0:
                return [[(np.zeros(0, np.int64), np.zeros(0, np.float64)) for _ in range(E)] for _ in range(Q)]
            idx_h, sims_h, counts_h = self._hits_exact64(queries, k)
            return [[(idx_h[qi, e, :counts_h[qi, e]], sims_h[qi, e, :counts_h[qi, e]]) for e in range(E)] for qi in range(Q)]
        if E == 0 or len(self) == 0:
            return [[(np.zeros(0, np.int64), np.zeros(0, np.float32)) for _ in range(E)] for _ in range(Q)]
        packed = self._search_segments_packed(q, self.offsets, k, prefilter)[0]
        idx_h, sims_h, counts_h = _hits_layout(Q, E, k).host_views(self._read_back(packed))
        idx_h, sims_h, counts_h = idx_h.copy(), sims_h.copy(), counts_h[0].copy()      # counts = min(k, n_e): the same for every query
        if int(counts_h.min()) == k:
            return [list(zip(idx_h[qi], sims_h[qi])) for qi in range(Q)]
        return [[(idx_h[qi, e, :counts_h[e]], sims_h[qi, e, :counts_h[e]]) for e in range(E)] for qi in range(Q)]

    def top_hits_multi(self, queries, k: int = 5, keep: int = 5, prefilter: bool = False, exact64: bool = False):
        """``top_hits`` for a batch of questions: per query the list that ``top_hits(query, k, keep)`` returns.  One pass over the
        store per 16 questions, one ranking launch for all of them (hmm_rank_segment_hits_multi), one read-back of Q x `keep`
        hits.  keep > 64 is served by ``top_hits`` per query.  ``prefilter``: the pass streams the bf16 shadow, the same results
        (``search_segments_multi_device``).  ``exact64=True``: per query what ``top_hits(query, k, keep, exact64=True)`` returns:
        the float64 per-event top-k of the whole batch, one packed read-back of (idx, sims float64, counts), and
        ``rank_hits_exact64`` per question on the host."""
        q = _queries_2d(queries)
        Q, E, k, keep = q.shape[0], len(self.lengths), int(k), int(keep)
        exact64 = self._use_exact64(exact64, "top_hits_multi", prefilter)
        if E == 0 or len(self) == 0 or keep < 1:
            return [[] for _ in range(Q)]
        if exact64:
            idx_h, sims_h, counts_h = self._hits_exact64(queries, k)
            return [rank_hits_exact64(idx_h[qi], sims_h[qi], counts_h[qi], keep)[0] for qi in range(Q)]
        if keep > 64:
            return [self.top_hits(q[qi], k, keep, prefilter) for qi in range(Q)]
        idx, sims, counts = self.search_segments_multi_device(q, self.offsets, k, prefilter)
        layout = _ranking_layout(Q, keep)
        packed = torch.empty(layout.nbytes, dtype=torch.uint8, device=idx.device)
        _lib.check(_lib.load().hmm_rank_segment_hits_multi(idx.data_ptr(), sims.data_ptr(), counts.data_ptr(), Q, E, k, keep,
                                                           *[t.data_ptr() for t in layout.device_views(packed)], _lib.stream_ptr()),
                   "hmm_rank_segment_hits_multi")
        ev_h, row_h, val_h, n_h = layout.host_views(self._read_back(packed))
        return [[(int(ev_h[qi, t]), int(row_h[qi, t]), float(val_h[qi, t])) for t in range(int(n_h[qi]))] for qi in range(Q)]

    # ---- the reference's own selection: row rule and fallback rule ahead of the ranking -----------------------------------------
    # _find_relevant_video_segments / _find_relevant_audio_segments (hippocampal_memory.py:3143-3277, :3294-3381) do not rank every
    # hit: a hit counts only when its row is below the event's number of KEPT rows (`idx < len(event.frame_times)`), and an event
    # whose best similarity is below 0.4 and that has captions / a transcription is answered by the LLM instead.  top_hits ranks
    # every hit, so its `keep` hits are in general not the reference's; these two methods apply both rules on the device
    # (hmm_rank_segment_hits_filtered[_multi]) and hand the deferred events back with their own hits.

    def relevant_hits(self, query, k: int = 5, keep: int = 5, *, row_limits=None, defer=None, min_similarity: float = 0.4,
                      prefilter: bool = False, exact64: bool = False):
        """(hits, deferred).  hits: [(event, row inside the event, similarity)], best first, the best `keep` of the hits that
        pass the row rule (``row < row_limits[event]``) in events that are not deferred.  deferred: [(event, idx int64[k_e],
        sims float32[k_e])] in event order -- the events with ``defer[event]`` set whose best similarity is below
        ``np.float32(min_similarity)``, each with exactly what ``top_k_per_event`` returns for it.  ``row_limits`` / ``defer``: one
        entry per event, or None (no row rule / nothing deferred).  Same order rules as ``top_hits`` (stable, NaN first; a NaN best
        similarity never defers, as ``max(...) < 0.4`` is False).  keep <= 1024.  One scan, one ranking launch, one packed read-back,
        and -- only when events were deferred -- a second one of their hits alone.

        ``exact64=True`` (a store whose float64 source held fp32 values; not with ``prefilter``): the per-event top-k runs on the
        device in float64, one packed read-back brings (idx, sims float64, counts), and the two rules and the stable descending
        sort run on the host in numpy (``rank_hits_exact64``): the reference's own operations, ``<`` on doubles against
        ``float(min_similarity)``.  Similarities (hits and deferred) are float64.  Ranking doubles on the device is a follow-up,
        not part of this route."""
        rules = self._relevance_rules("relevant_hits", k, keep, row_limits, defer, min_similarity)
        if self._use_exact64(exact64, "relevant_hits", prefilter):
            if not self.lengths:
                return [], []
            return rank_hits_exact64(*self._hits_exact64(query, k, single=True), int(keep), rules[0], rules[1], min_similarity)
        q = _query_to_device(query, self.rows.device)
        if not self.lengths:
            return [], []
        packed = self._search_segments_packed(q, self.offsets, k, prefilter, single=True)
        return self._rank_relevant(packed[1:], None, int(keep), rules)[0]

    def relevant_hits_multi(self, queries, k: int = 5, keep: int = 5, *, row_limits=None, defer=None, min_similarity: float = 0.4,
                            prefilter: bool = False, exact64: bool = False):
        """``relevant_hits`` for a batch of questions: per query the (hits, deferred) pair, from one pass over the store per 16
        questions, one ranking launch for all of them (hmm_rank_segment_hits_filtered_multi) and the same one or two read-backs.
        The similarities are those of ``top_k_per_event_multi``.  ``exact64=True``: per query what ``relevant_hits(query, ...,
        exact64=True)`` returns: the float64 per-event top-k of the whole batch, one packed read-back, then both rules and the
        stable sort per question on the host (``rank_hits_exact64``)."""
        rules = self._relevance_rules("relevant_hits_multi", k, keep, row_limits, defer, min_similarity)
        q = _queries_2d(queries)
        exact64 = self._use_exact64(exact64, "relevant_hits_multi", prefilter)
        if not self.lengths:
            return [([], []) for _ in range(q.shape[0])]
        if exact64:
            idx_h, sims_h, counts_h = self._hits_exact64(queries, k)
            return [rank_hits_exact64(idx_h[qi], sims_h[qi], counts_h[qi], int(keep), rules[0], rules[1], min_similarity)
                    for qi in range(q.shape[0])]
        packed = self._search_segments_packed(q, self.offsets, k, prefilter)
        return self._rank_relevant(packed[1:], q.shape[0], int(keep), rules)

    def _relevance_rules(self, what: str, k, keep, row_limits, defer, min_similarity):
        """The host-side checks of relevant_hits[_multi], before anything is launched -> (limits int64[E] or None, flags uint8[E]
        or None, the threshold as fp32)."""
        E = len(self.lengths)
        if int(k) < 1:
            raise ValueError(f"{what}: k must be >= 1")
        if not 1 <= int(keep) <= 1024:
            raise ValueError(f"{what}: keep must be between 1 and 1024, got {keep}")
        if E and min(self.lengths) == 0:                         # the reference's np.max / max of an empty array raises there
            raise ValueError(f"{what}: event {list(self.lengths).index(0)} has no rows")
        limits = flags = None
        if row_limits is not None:
            limits = np.asarray(row_limits).reshape(-1)
            if limits.size and limits.dtype.kind not in "iu":
                raise ValueError(f"{what}: row_limits must be integers, got {limits.dtype}")
            limits = np.ascontiguousarray(limits, dtype=np.int64)
            if limits.shape[0] != E:
                raise ValueError(f"{what}: row_limits has {limits.shape[0]} entries for {E} events")
            if E and int(limits.min()) < 0:
                raise ValueError(f"{what}: row_limits must be >= 0")
        if defer is not None:
            flags = np.asarray(defer).reshape(-1)
            if flags.shape[0] != E:
                raise ValueError(f"{what}: defer has {flags.shape[0]} entries for {E} events")
            flags = np.ascontiguousarray(flags.astype(bool).astype(np.uint8))
        return limits, flags, np.float32(min_similarity)

    def _upload_rules(self, limits, flags):
        """row_limits | defer in one pinned buffer, one asynchronous copy -> their device addresses (None where not given)."""
        parts = [a.view(np.uint8) for a in (limits, flags) if a is not None]
        if not parts:
            return None, None, None
        host = torch.from_numpy(np.concatenate(parts))
        if self.rows.is_cuda:
            # one pinned staging buffer per store.  A call that returns has synchronised on its read-back, so its copy has landed
            # before the next call overwrites the buffer; a call that RAISED after queueing the copy has not, and the next call
            # may overwrite bytes still in flight -- of an upload whose result nobody reads any more.
            if self._pinned_rules is None or self._pinned_rules.numel() < host.numel():
                self._pinned_rules = torch.empty(max(host.numel(), 1 << 12), dtype=torch.uint8, pin_memory=True)
            staged = self._pinned_rules[: host.numel()]
            staged.copy_(host)
            dev = staged.to(self.rows.device, non_blocking=True)
        else:
            dev = host
        base, at = dev.data_ptr(), (limits.nbytes if limits is not None else 0)
        return dev, (base if limits is not None else None), (base + at if flags is not None else None)

    def _rank_relevant(self, hits, Q, keep: int, rules):
        """The filtered ranking of the (idx, sims, counts) of a segmented scan and its read-backs; Q None: one question."""
        idx, sims, counts = hits
        lead = () if Q is None else (Q,)
        n_q, (E, k) = Q or 1, idx.shape[-2:]
        limits, flags, threshold = rules
        layout = _relevant_layout(*lead, E, keep)
        packed = torch.empty(layout.nbytes, dtype=torch.uint8, device=idx.device)
        outputs = layout.device_views(packed)
        if flags is not None:
            d_idx, d_sims = _deferred_layout(n_q, E * k).device_views(
                torch.empty(_deferred_layout(n_q, E * k).nbytes, dtype=torch.uint8, device=idx.device))
            d_ptrs = (d_idx.data_ptr(), d_sims.data_ptr())
        else:                                                     # nothing can be deferred: the two arrays are never written, any
            d_ptrs = (packed.data_ptr(), packed.data_ptr())       # non-null address satisfies the argument check
        keepalive, limits_ptr, flags_ptr = self._upload_rules(limits, flags)
        name = "hmm_rank_segment_hits_filtered" if Q is None else "hmm_rank_segment_hits_filtered_multi"
        ev, row, val, n, d_ev, n_d, d_cnt = outputs
        _lib.check(getattr(_lib.load(), name)(idx.data_ptr(), sims.data_ptr(), counts.data_ptr(), *lead, E, k, keep, limits_ptr,
                                              flags_ptr, float(threshold), ev.data_ptr(), row.data_ptr(), val.data_ptr(), n.data_ptr(),
                                              d_ev.data_ptr(), n_d.data_ptr(), *d_ptrs, d_cnt.data_ptr(),
                                              _lib.stream_ptr()), name)
        ev_h, row_h, val_h, n_h, d_ev_h, n_d_h, d_cnt_h = [v.reshape((n_q,) + v.shape[len(lead):]) for v in
                                                           layout.host_views(self._read_back(packed))]
        found = [[(int(ev_h[qi, t]), int(row_h[qi, t]), float(val_h[qi, t])) for t in range(int(n_h[qi, 0]))] for qi in range(n_q)]
        n_def = [int(n_d_h[qi, 0]) for qi in range(n_q)]
        if max(n_def) == 0:
            return [(found[qi], []) for qi in range(n_q)]
        d_ev_h, d_cnt_h = d_ev_h.copy(), d_cnt_h.copy()           # the staging buffer is rewritten by the second read-back
        # per question the compacted front of both arrays, n_deferred * k entries: contiguous pieces, copied as they lie (two
        # per question that deferred anything; every idx piece, then every sims piece), one synchronisation
        asked = [qi for qi in range(n_q) if n_def[qi]]
        raw = self._read_back(*[a[qi, : n_def[qi] * k] for a in (d_idx, d_sims) for qi in asked]).copy()
        out, at, sims_at = [(found[qi], []) for qi in range(n_q)], 0, sum(n_def) * k * 8
        for qi in asked:
            cells = n_def[qi] * k
            idx_h, sims_h = raw[at: at + cells * 8].view(np.int64), raw[sims_at: sims_at + cells * 4].view(np.float32)
            at, sims_at = at + cells * 8, sims_at + cells * 4
            out[qi][1].extend((int(d_ev_h[qi, j]), idx_h[j * k: j * k + d_cnt_h[qi, j]], sims_h[j * k: j * k + d_cnt_h[qi, j]])
                              for j in range(n_def[qi]))
        return out

    # ---- a store that grows: append, replace and drop events on the device ----------------------------------------------------
    # The constructor and from_device_rows leave `rows` as they always did (an exact-size upload, or the caller's tensor).  The
    # first mutating call moves the store into buffers it owns: `_buf`, (capacity, 1024) fp32, and -- once a shadow exists --
    # `_shadow_buf`, capacity * 2048 bytes.  `rows` stays a contiguous view of the first n rows and `_shadow` of the first
    # n * 2048 bytes, `offsets` and `lengths` keep their meaning, so every search method above works unchanged on a grown store and
    # returns what a fresh EventStore of the same events returns, bit for bit.  New rows are written by hmm_store_ingest_rows
    # (fp32 rows and their shadow rows in one launch), events are moved by hmm_store_gather_segments.  Everything is enqueued on
    # the current stream and nothing synchronises the device; a mutating call makes one small host-to-device copy (the offsets,
    # from pinned memory) plus the upload of a source that lives on the host.  Single-threaded use, like the rest of the class.

    @property
    def capacity(self) -> int:
        """Rows the store holds without moving (its row count while it still aliases the tensor it was built from)."""
        return len(self) if self._buf is None else self._buf.shape[0]

    def _set_buffers(self, buf: torch.Tensor, shadow_buf, n: int, shadow: bool):
        self._buf, self._shadow_buf = buf, shadow_buf
        self.rows = buf[:n]
        self._shadow = shadow_buf[: n * 2048] if shadow else None
        if shadow:
            self._shadow_version = self._rows_version()

    def _new_buffers(self, capacity: int, shadow: bool):
        dev = self.rows.device
        return (torch.empty(capacity, FEATURE_DIM, dtype=torch.float32, device=dev),
                torch.empty(capacity * 2048, dtype=torch.uint8, device=dev) if shadow else None)

    def _move_to(self, capacity: int, shadow: bool):
        """Owned buffers of `capacity` rows holding the present rows (and shadow): two device-to-device copies."""
        n = len(self)
        buf, shadow_buf = self._new_buffers(capacity, shadow)
        if n > 0:
            buf[:n].copy_(self.rows)
            if shadow:
                shadow_buf[: n * 2048].copy_(self._shadow[: n * 2048])
        self._set_buffers(buf, shadow_buf, n, shadow)

    def _grown(self, needed: int) -> int:
        return max(int(needed), 2 * self.capacity, 1)

    def reserve(self, rows: int):
        """Grow the capacity to at least `rows` rows now (existing rows and shadow are copied device to device; both buffers exist
        side by side until the old one is released), so that later appends up to that size write nothing but their own rows and
        ``rows.data_ptr()`` stays put.  A store built by the constructor or by ``from_device_rows`` moves into buffers of its own."""
        rows = int(rows)
        if rows < 0:
            raise ValueError("rows must be >= 0")
        if rows > self.capacity:
            self._move_to(rows, self._shadow_is_current())
        return self

    def _source_rows(self, features) -> torch.Tensor:
        """The rows of one event as a contiguous (n,1024) fp32 or fp64 tensor on the store's device: a device tensor stays where
        it lies, a host array is uploaded as it is (fp64 is narrowed by the ingest kernel, not by numpy), any other dtype is
        converted to fp32 first, as the constructor converts it."""
        if isinstance(features, torch.Tensor):
            t = features.detach()
            if t.dtype not in (torch.float32, torch.float64):
                t = t.to(torch.float32)
        else:
            a = np.asarray(features)
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float32)
            t = torch.from_numpy(np.ascontiguousarray(a))
        if t.numel() == 0:
            return torch.empty(0, FEATURE_DIM, dtype=torch.float32, device=self.rows.device)
        if t.dim() == 1 and t.shape[0] == FEATURE_DIM:
            t = t.reshape(1, FEATURE_DIM)
        if t.dim() != 2 or t.shape[1] != FEATURE_DIM:
            raise ValueError(f"event features must be (n,{FEATURE_DIM}) or ({FEATURE_DIM},), got {tuple(t.shape)}")
        t = t.to(self.rows.device).contiguous()
        for mine in (self.rows if self._buf is None else self._buf, self._shadow_buf):
            if mine is not None and mine.numel() > 0:
                a0, b0 = t.data_ptr(), mine.data_ptr()
                if a0 < b0 + mine.numel() * mine.element_size() and b0 < a0 + t.numel() * t.element_size():
                    raise ValueError("the source overlaps the store's own buffer: clone it first")
        return t

    def _upload_tables(self, lengths, src_segment=None):
        """offsets (int64, E + 1) and, for a gather, the source segment of every destination segment (int32, E): one pinned
        buffer, one asynchronous copy."""
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        seg = np.asarray(src_segment if src_segment is not None else [], dtype=np.int32)
        host = torch.from_numpy(np.concatenate([off.view(np.uint8), seg.view(np.uint8)])).pin_memory()
        dev = host.to(self.rows.device, non_blocking=True)
        return dev[: off.nbytes].view(torch.int64), dev[off.nbytes:].view(torch.int32)

    def _ingest(self, src: torch.Tensor, at: int, shadow: bool):
        if src.shape[0] == 0:
            return
        _lib.check(_lib.load().hmm_store_ingest_rows(src.data_ptr(), 1 if src.dtype == torch.float64 else 0, src.shape[0], FEATURE_DIM,
                                                     self._buf.data_ptr(), self._shadow_buf.data_ptr() if shadow else None,
                                                     self._buf.shape[0], at, _lib.stream_ptr()), "hmm_store_ingest_rows")

    def _note_ingested(self, features, src: torch.Tensor, at: int):
        """AND a float64 event that was just ingested at row ``at`` into ``f64_exact``: a host source is checked with numpy, a
        device tensor by hmm_rows_f64_are_f32 beside the ingest."""
        if src.dtype != torch.float64 or src.shape[0] == 0:
            return
        if isinstance(features, torch.Tensor):
            self._note_f64_source(src if features.is_cuda else features.detach(), at)
        else:
            self._note_f64_source(np.asarray(features), at)

    def append_event(self, features) -> int:
        """Append one event and return its index.  ``features``: numpy or torch, host or device, (n,1024), a 1-D (1024,) row or
        an empty matrix, float32 or float64 (another dtype is converted to float32 first; another width is a ValueError).  A
        device tensor is ingested where it lies -- no host trip -- and float64 is narrowed on the device, to the bits
        ``astype(np.float32)`` gives.  While the rows fit the capacity nothing but the new rows (and their shadow rows, when the
        store has a shadow) is written and ``rows.data_ptr()`` does not change; otherwise the capacity becomes
        max(needed, 2 x capacity) and the store moves (see ``reserve``).  The result is the store -- rows, offsets, shadow --
        that ``EventStore(all events)`` builds."""
        return self.extend([features])[0]

    def extend(self, list_of_features):
        """``append_event`` for several events: at most one move, one ingest launch per event, one offsets update.  Returns the
        new events' indices."""
        list_of_features = list(list_of_features)
        srcs = [self._source_rows(f) for f in list_of_features]
        first = len(self.lengths)
        if not srcs:
            return []
        n = len(self)
        needed = n + sum(s.shape[0] for s in srcs)
        shadow = self._shadow_is_current()
        if self._buf is None or needed > self._buf.shape[0]:
            self._move_to(self._grown(needed), shadow)
        at = n
        for f, s in zip(list_of_features, srcs):
            self._ingest(s, at, shadow)
            self._note_ingested(f, s, at)
            at += s.shape[0]
        self.lengths = list(self.lengths) + [int(s.shape[0]) for s in srcs]
        self.offsets = self._upload_tables(self.lengths)[0]
        self._set_buffers(self._buf, self._shadow_buf, needed, shadow)
        return list(range(first, first + len(srcs)))

    def _regather(self, src_segment, new_lengths):
        """Rebuild the store out of place: destination event j takes the rows of present event src_segment[j], or stays a hole
        of new_lengths[j] rows (-1)."""
        needed = int(sum(new_lengths))
        shadow = self._shadow_is_current()
        owned = self._buf is not None
        capacity = max(self.capacity, 1) if needed <= self.capacity else self._grown(needed)
        offsets, seg = self._upload_tables(new_lengths, src_segment)
        copies = any(s >= 0 and n > 0 for s, n in zip(src_segment, new_lengths))
        if copies or not owned or capacity != self.capacity:
            buf, shadow_buf = self._new_buffers(capacity, shadow)
        else:                                                    # nothing survives and the buffers fit: they are reused
            buf, shadow_buf = self._buf, self._shadow_buf
        if copies:
            _lib.check(_lib.load().hmm_store_gather_segments(
                self.rows.data_ptr(), self._shadow.data_ptr() if shadow else None, len(self), self.offsets.data_ptr(),
                len(self.lengths), seg.data_ptr(), offsets.data_ptr(), len(new_lengths), FEATURE_DIM, buf.data_ptr(),
                shadow_buf.data_ptr() if shadow else None, needed, capacity, _lib.stream_ptr()), "hmm_store_gather_segments")
        self.lengths = [int(n) for n in new_lengths]
        self.offsets = offsets
        self._set_buffers(buf, shadow_buf, needed, shadow)

    def remove_events(self, indices):
        """Drop the events at ``indices`` (negative ones count from the end); later events shift down, as ``del`` on the list
        would.  The survivors are gathered out of place into a second buffer of the same capacity and the old one is released,
        so for the length of the call the store takes twice its memory (no workgroup ever waits for another one's copy).  An
        index out of range (IndexError) or named twice (ValueError) raises before anything is launched."""
        E = len(self.lengths)
        drop = set()
        for i in indices:
            j = _index_of(i, E)
            if j in drop:
                raise ValueError(f"event {j} is named twice")
            drop.add(j)
        if not drop:
            return self
        keep = [j for j in range(E) if j not in drop]
        self._regather(keep, [self.lengths[j] for j in keep])
        return self

    def replace_event(self, i: int, features):
        """Event ``i`` gets new rows, of any length, and keeps its index: a gather with a hole at ``i`` (out of place, transient
        2 x memory as in ``remove_events``), then an ingest into the hole."""
        E = len(self.lengths)
        j = _index_of(i, E)
        src = self._source_rows(features)
        lengths = list(self.lengths)
        lengths[j] = int(src.shape[0])
        self._regather([-1 if e == j else e for e in range(E)], lengths)
        self._ingest(src, int(sum(lengths[:j])), self._shadow is not None)
        self._note_ingested(features, src, int(sum(lengths[:j])))
        return self
