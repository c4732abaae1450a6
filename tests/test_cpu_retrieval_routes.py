"""CPU: which C entry point every retrieval route of hippomm_amd.vector_ops calls, and with which arguments.

The library is replaced by a recorder (every ``hmm_*_workspace_bytes`` answers a fixed number, ``hmm_shadow_store_bytes(n)`` answers
n * 2048, every other entry point records its name and arguments and returns 0) and the stores live on the CPU, so the test pins
the host layer alone: entry point, integer arguments in order, store / shadow / output / stats / workspace pointers, the shadow's
bookkeeping, and the two packed read-back layouts (idx | sims | counts and event | row | sim | count).  What the kernels compute is
the GPU suites' business."""
import ctypes

import numpy as np
import pytest
import torch

from hippomm_amd import _lib
from hippomm_amd import vector_ops as vo

CPU = torch.device("cpu")
LENGTHS, N, E, Q, K, DIM = [10, 0, 30], 40, 3, 17, 5, 1024

# every size function answers its own number; the segmented pair answers one number, as the C side defines the two equal
SIZES = {"hmm_cosine_topk_workspace_bytes": 1008,
         "hmm_cosine_topk_prefilter_workspace_bytes": 2016,
         "hmm_cosine_topk_segmented_workspace_bytes": 3024,
         "hmm_cosine_topk_segmented_prefilter_workspace_bytes": 3024,
         "hmm_cosine_topk_multi_workspace_bytes": 4032,
         "hmm_cosine_topk_multi_prefilter_workspace_bytes": 5040,
         "hmm_cosine_topk_segmented_multi_workspace_bytes": 6048,
         "hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes": 7056}
SEGMENTED_SIZES = ("hmm_cosine_topk_segmented_workspace_bytes", "hmm_cosine_topk_segmented_prefilter_workspace_bytes")


class _Recorder:
    def __init__(self):
        self.calls, self.sized = [], []

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            def size(*args):
                self.sized.append((name, args))
                return SIZES[name]
            return size
        if name == "hmm_shadow_store_bytes":
            return lambda n: n * 2048

        def entry(*args):
            self.calls.append((name, args))
            if name == "hmm_rank_segment_hits":                 # its caller reads the hit count back: no hits
                ctypes.memset(args[9], 0, 4)
            return 0
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls

    def only(self):
        calls = self.take()
        assert len(calls) == 1, [c[0] for c in calls]
        return calls[0]


class _Ptr:
    """Equals any non-null pointer."""

    def __eq__(self, other):
        return isinstance(other, int) and other != 0

    def __repr__(self):
        return "<non-null>"


PTR = _Ptr()


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    return rec


def _events(lengths=LENGTHS):
    rng = np.random.default_rng(3)
    return [rng.standard_normal((n, DIM)).astype(np.float32) for n in lengths]


def _event_store(lengths=LENGTHS):
    return vo.EventStore(_events(lengths), device=CPU)


def _feature_store(n=N, shadow=False):
    return vo.FeatureStore(np.concatenate(_events([n])), device=CPU, shadow=shadow)


def _query():
    return torch.linspace(-1, 1, DIM)


def _queries():
    return torch.linspace(-1, 1, Q * DIM).reshape(Q, DIM)


def _shadow_build(store):
    return ("hmm_shadow_store_build", (store.rows.data_ptr(), len(store), DIM, store._shadow.data_ptr(), len(store) * 2048, None))


# ---- the flat routes ----------------------------------------------------------------------------------------------------------
def test_flat_exact(lib):
    store, q = _feature_store(), _query()
    idx, sims = store.search_device(q, K)
    assert lib.only() == ("hmm_cosine_topk", (store.rows.data_ptr(), N, DIM, q.data_ptr(), K, idx.data_ptr(), sims.data_ptr(), PTR,
                                              PTR, SIZES["hmm_cosine_topk_workspace_bytes"], None))
    assert lib.sized == [("hmm_cosine_topk_workspace_bytes", (N, K))]
    assert idx.shape == (K,) and idx.dtype == torch.int64 and sims.shape == (K,) and sims.dtype == torch.float32
    assert store.search_device(q, 64)[0].shape == (N,)                        # k' = min(k, N)
    assert lib.only()[1][4] == 64
    with pytest.raises(ValueError, match="k must be >= 1"):
        store.search_device(q, 0)


@pytest.mark.parametrize("with_stats", [False, True])
def test_flat_prefilter(lib, with_stats):
    store, q = _feature_store(), _query()
    stats = torch.zeros(2, dtype=torch.int32) if with_stats else None
    idx, sims = store.search_prefiltered_device(q, K, stats)
    build, scan = lib.take()
    assert build == _shadow_build(store)
    assert scan == ("hmm_cosine_topk_prefilter", (store.rows.data_ptr(), store._shadow.data_ptr(), N, DIM, q.data_ptr(), K, idx.data_ptr(),
                                                  sims.data_ptr(), PTR, stats.data_ptr() if with_stats else None, PTR,
                                                  SIZES["hmm_cosine_topk_prefilter_workspace_bytes"], None))
    assert lib.sized == [("hmm_cosine_topk_prefilter_workspace_bytes", (N, K))]
    assert store._shadow.numel() == N * 2048 and idx.shape == sims.shape == (K,)
    with pytest.raises(ValueError, match="k must be >= 1"):
        store.search_prefiltered_device(q, 0)


def test_search_device_goes_through_the_shadow_only_on_a_shadow_store(lib):
    store, q = _feature_store(shadow=True), _query()
    assert store.use_shadow and lib.only() == _shadow_build(store)           # built by the constructor
    idx, sims = store.search_device(q, K)
    assert lib.only() == ("hmm_cosine_topk_prefilter", (store.rows.data_ptr(), store._shadow.data_ptr(), N, DIM, q.data_ptr(), K,
                                                        idx.data_ptr(), sims.data_ptr(), PTR, None, PTR,
                                                        SIZES["hmm_cosine_topk_prefilter_workspace_bytes"], None))
    plain = _feature_store()
    plain.build_shadow()                                                      # a shadow that merely exists does not reroute search_device
    lib.take()
    plain.search_device(q, K)
    assert not plain.use_shadow and lib.only()[0] == "hmm_cosine_topk"


def test_keys_has_no_shadow_variant(lib):
    for store in (_feature_store(), _feature_store(shadow=True)):
        lib.take()
        q = _query()
        keys = store.search_keys_device(q, K)
        assert lib.only() == ("hmm_cosine_topk_keys", (store.rows.data_ptr(), N, DIM, q.data_ptr(), K, keys.data_ptr(), PTR,
                                                       SIZES["hmm_cosine_topk_workspace_bytes"], None))
        assert keys.shape == (K,) and keys.dtype == torch.int64
    assert lib.sized == [("hmm_cosine_topk_workspace_bytes", (N, K))] * 2


# ---- the segmented routes -----------------------------------------------------------------------------------------------------
def _assert_hits_views(idx, sims, counts, lead):
    """idx | sims | counts back to back: sims at lead * k * 8, counts at lead * k * 12 from idx."""
    base = idx.data_ptr()
    assert (sims.data_ptr() - base, counts.data_ptr() - base) == (lead * K * 8, lead * K * 12)
    assert (idx.dtype, sims.dtype, counts.dtype) == (torch.int64, torch.float32, torch.int32)


def test_segmented_exact(lib):
    store, q = _event_store(), _query()
    idx, sims, counts = store.search_segments_device(q, store.offsets, K)
    assert lib.only() == ("hmm_cosine_topk_segmented", (store.rows.data_ptr(), N, DIM, q.data_ptr(), store.offsets.data_ptr(), E, K,
                                                        idx.data_ptr(), idx.data_ptr() + E * K * 8, idx.data_ptr() + E * K * 12, PTR,
                                                        SIZES["hmm_cosine_topk_segmented_workspace_bytes"], None))
    (size_fn, size_args), = lib.sized
    assert size_fn in SEGMENTED_SIZES and size_args == (N, E, K)
    assert idx.shape == sims.shape == (E, K) and counts.shape == (E,)
    _assert_hits_views(idx, sims, counts, E)


def test_segmented_prefilter(lib):
    store, q = _event_store(), _query()
    idx, sims, counts = store.search_segments_device(q, store.offsets, K, prefilter=True)
    build, scan = lib.take()
    assert build == _shadow_build(store)
    # no stats pointer on this entry point: the workspace follows the three outputs
    assert scan == ("hmm_cosine_topk_segmented_prefilter", (store.rows.data_ptr(), store._shadow.data_ptr(), N, DIM, q.data_ptr(),
                                                            store.offsets.data_ptr(), E, K, idx.data_ptr(), idx.data_ptr() + E * K * 8,
                                                            idx.data_ptr() + E * K * 12, PTR,
                                                            SIZES["hmm_cosine_topk_segmented_prefilter_workspace_bytes"], None))
    (size_fn, size_args), = lib.sized
    assert size_fn in SEGMENTED_SIZES and size_args == (N, E, K)
    _assert_hits_views(idx, sims, counts, E)


# ---- the batched routes -------------------------------------------------------------------------------------------------------
def _recorded_queries(call, shadow):
    return call[1][4 if shadow else 3]


def test_multi_exact_also_on_a_shadow_store(lib):
    for store, prefilter in ((_feature_store(), None), (_feature_store(), False), (_feature_store(shadow=True), None)):
        lib.take()
        q = _queries()
        idx, sims = store.search_multi_device(q, K, prefilter)
        name, args = lib.only()
        assert name == "hmm_cosine_topk_multi"
        assert args == (store.rows.data_ptr(), N, DIM, q.data_ptr(), Q, K, idx.data_ptr(), sims.data_ptr(), PTR, PTR,
                        SIZES["hmm_cosine_topk_multi_workspace_bytes"], None)
        assert idx.shape == sims.shape == (Q, K)
    assert lib.sized == [("hmm_cosine_topk_multi_workspace_bytes", (N, Q, K))] * 3
    wide = _feature_store().search_multi_device(_queries(), 64)[0]            # k' = min(k, N): a column slice of the (Q, k) output
    assert wide.shape == (Q, N) and wide.stride() == (64, 1)


@pytest.mark.parametrize("with_stats", [False, True])
def test_multi_prefilter(lib, with_stats):
    store, q = _feature_store(), _queries()
    stats = torch.zeros(Q, 2, dtype=torch.int32) if with_stats else None
    idx, sims = store.search_multi_device(q, K, prefilter=True, stats=stats)
    build, scan = lib.take()
    assert build == _shadow_build(store)
    assert scan == ("hmm_cosine_topk_multi_prefilter", (store.rows.data_ptr(), store._shadow.data_ptr(), N, DIM, q.data_ptr(), Q, K,
                                                        idx.data_ptr(), sims.data_ptr(), PTR, stats.data_ptr() if with_stats else None, PTR,
                                                        SIZES["hmm_cosine_topk_multi_prefilter_workspace_bytes"], None))
    assert lib.sized == [("hmm_cosine_topk_multi_prefilter_workspace_bytes", (N, Q, K))]


def test_multi_queries_are_validated_and_made_contiguous_fp32(lib):
    store = _feature_store()
    with pytest.raises(ValueError, match=r"queries must be \(Q,1024\), got \(1024,\)"):
        store.search_multi_device(_query(), K)
    with pytest.raises(ValueError, match="no queries"):
        store.search_multi_device(torch.zeros(0, DIM), K)
    with pytest.raises(ValueError, match=r"queries must be \(Q,1024\), got \(17, 8\)"):
        store.search_segments_multi_device(np.zeros((Q, 8)), torch.zeros(4, dtype=torch.int64), K)
    with pytest.raises(ValueError, match="no queries"):
        store.search_segments_multi_device(np.zeros((0, DIM)), torch.zeros(4, dtype=torch.int64), K)
    assert lib.take() == []
    q64 = _queries().double()                                                  # fp64: converted, so another buffer reaches the library
    store.search_multi_device(q64, K)
    assert _recorded_queries(lib.only(), False) != q64.data_ptr()


def test_segmented_multi_exact(lib):
    store, q = _event_store(), _queries()
    idx, sims, counts = store.search_segments_multi_device(q, store.offsets, K)
    assert lib.only() == ("hmm_cosine_topk_segmented_multi", (store.rows.data_ptr(), N, DIM, q.data_ptr(), Q, store.offsets.data_ptr(), E, K,
                                                              idx.data_ptr(), idx.data_ptr() + Q * E * K * 8, idx.data_ptr() + Q * E * K * 12,
                                                              PTR, SIZES["hmm_cosine_topk_segmented_multi_workspace_bytes"], None))
    assert lib.sized == [("hmm_cosine_topk_segmented_multi_workspace_bytes", (N, E, Q, K))]
    assert idx.shape == sims.shape == (Q, E, K) and counts.shape == (Q, E)
    _assert_hits_views(idx, sims, counts, Q * E)
    with pytest.raises(ValueError, match="k must be >= 1"):
        store.search_segments_multi_device(q, store.offsets, 0)


@pytest.mark.parametrize("with_stats", [False, True])
def test_segmented_multi_prefilter(lib, with_stats):
    store, q = _event_store(), _queries()
    stats = torch.zeros(2, dtype=torch.int32) if with_stats else None
    idx, sims, counts = store.search_segments_multi_device(q, store.offsets, K, prefilter=True, stats=stats)
    build, scan = lib.take()
    assert build == _shadow_build(store)
    assert scan == ("hmm_cosine_topk_segmented_multi_prefilter", (store.rows.data_ptr(), store._shadow.data_ptr(), N, DIM, q.data_ptr(), Q,
                                                                  store.offsets.data_ptr(), E, K, idx.data_ptr(),
                                                                  idx.data_ptr() + Q * E * K * 8, idx.data_ptr() + Q * E * K * 12,
                                                                  stats.data_ptr() if with_stats else None, PTR,
                                                                  SIZES["hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes"], None))
    assert lib.sized == [("hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes", (N, E, Q, K))]
    _assert_hits_views(idx, sims, counts, Q * E)


# ---- a store without rows, asked for the shadow route --------------------------------------------------------------------------
def test_prefilter_on_a_store_without_rows(lib):
    """What each route does today with prefilter=True and zero rows (the library refuses n == 0 where it is reached; the recorder
    does not).  Flat single query: no fallback, the shadow build and the prefilter entry are both called with n == 0.  search_device
    on FeatureStore(shadow=True): the constructor built no shadow, the exact entry.  Segmented and flat batched: the exact entry.
    Segmented batched: no entry at all, the padding is written by torch."""
    empty = np.zeros((0, DIM), np.float32)
    q, qs = _query(), _queries()

    flat = vo.FeatureStore(empty, device=CPU)
    idx, sims = flat.search_prefiltered_device(q, K)
    assert [c[0] for c in lib.take()] == ["hmm_shadow_store_build", "hmm_cosine_topk_prefilter"] and idx.shape == (0,)

    shadowed = vo.FeatureStore(empty, device=CPU, shadow=True)
    assert not shadowed.use_shadow and lib.take() == []
    shadowed.search_device(q, K)
    name, args = lib.only()
    assert name == "hmm_cosine_topk" and args[1] == 0

    events = vo.EventStore([empty, empty], device=CPU)
    idx, sims, counts = events.search_segments_device(q, events.offsets, K, prefilter=True)
    name, args = lib.only()
    assert name == "hmm_cosine_topk_segmented" and args[1] == 0 and args[5] == 2

    idx, sims = events.search_multi_device(qs, K, prefilter=True)
    name, args = lib.only()
    assert name == "hmm_cosine_topk_multi" and args[1] == 0 and idx.shape == (Q, 0)

    idx, sims, counts = events.search_segments_multi_device(qs, events.offsets, K, prefilter=True)
    assert lib.take() == [] and idx.shape == (Q, 2, K) and bool((idx == -1).all()) and not sims.any() and not counts.any()
    none = vo.EventStore([], device=CPU)
    idx, sims, counts = none.search_segments_multi_device(qs, none.offsets, K, prefilter=True)
    assert lib.take() == [] and idx.shape == (Q, 0, K) and counts.shape == (Q, 0)
    assert none.top_hits_multi(qs) == [[] for _ in range(Q)]
    assert none.top_k_per_event_multi(qs) == [[] for _ in range(Q)]
    assert lib.take() == []


# ---- the workspace -------------------------------------------------------------------------------------------------------------
def test_workspace_grows_only_when_too_small_and_by_exactly_what_was_asked(lib):
    store, q, qs = _event_store(), _query(), _queries()
    store.search_segments_device(q, store.offsets, K)                          # 3024
    first = lib.only()[1][-3:-1]
    assert first[1] == 3024
    store.search_keys_device(q, K)                                             # 1008: fits, the same buffer
    assert lib.only()[1][-3:-1] == first
    store.search_segments_multi_device(qs, store.offsets, K)                   # 6048: grown to exactly that
    grown = lib.only()[1][-3:-1]
    assert grown[1] == 6048
    store.search_multi_device(qs, K)                                           # 4032: fits
    assert lib.only()[1][-3:-1] == grown


# ---- the shadow's bookkeeping --------------------------------------------------------------------------------------------------
def test_shadow_is_a_snapshot_rebuilt_on_a_version_bump_or_after_invalidate(lib):
    store, q = _event_store(), _query()
    assert not store.use_shadow
    assert store.build_shadow() is store and lib.only() == _shadow_build(store)
    store.build_shadow()
    store.search_prefiltered_device(q, K)
    assert [c[0] for c in lib.take()] == ["hmm_cosine_topk_prefilter"]         # current: not built again
    store.build_shadow(force=True)
    assert lib.only() == _shadow_build(store)
    store.rows.mul_(2.0)                                                       # an edit through torch bumps the version
    store.search_segments_device(q, store.offsets, K, prefilter=True)
    assert [c[0] for c in lib.take()] == ["hmm_shadow_store_build", "hmm_cosine_topk_segmented_prefilter"]
    assert store.invalidate_shadow() is store and store._shadow is None
    store.search_multi_device(_queries(), K, prefilter=True)
    assert [c[0] for c in lib.take()] == ["hmm_shadow_store_build", "hmm_cosine_topk_multi_prefilter"]


def test_shadow_of_a_store_that_owns_its_buffers_lives_in_the_capacity_sized_buffer(lib):
    store = _event_store()
    assert store.capacity == N
    store.reserve(64)
    assert store.capacity == 64 and store._buf.shape == (64, DIM) and store.rows.data_ptr() == store._buf.data_ptr() and len(store) == N
    assert store._shadow is None and lib.take() == []
    store.build_shadow()
    assert lib.only() == ("hmm_shadow_store_build", (store._buf.data_ptr(), N, DIM, store._shadow_buf.data_ptr(), N * 2048, None))
    assert store._shadow_buf.numel() == 64 * 2048 and store._shadow.data_ptr() == store._shadow_buf.data_ptr()
    assert store._shadow.numel() == N * 2048
    store.reserve(128)                                                         # a current shadow travels with its rows
    assert store._shadow is not None and store._shadow_buf.numel() == 128 * 2048 and lib.take() == []
    store.rows.mul_(2.0)
    store.reserve(256)                                                         # a stale one does not
    assert store._shadow is None and lib.take() == []

    none = vo.EventStore([], device=CPU).reserve(8)                            # owned and empty: nothing is launched
    none.build_shadow()
    assert lib.take() == [] and none._shadow.numel() == 0 and none._shadow_buf.numel() == 8 * 2048


# ---- the ranking behind top_hits ------------------------------------------------------------------------------------------------
def test_top_hits_ranks_the_segmented_outputs_into_one_packed_buffer(lib):
    store, keep = _event_store(), 7
    assert store.top_hits(_query(), K, keep) == []                             # the recorder reports no hits
    scan, rank = lib.take()
    assert scan[0] == "hmm_cosine_topk_segmented" and rank[0] == "hmm_rank_segment_hits"
    idx, sims, counts = scan[1][7:10]
    ev = rank[1][6]
    assert rank[1] == (idx, sims, counts, E, K, keep, ev, ev + keep * 8, ev + keep * 16, ev + keep * 20, None)
    store.top_hits(_query(), K, keep, prefilter=True)
    assert [c[0] for c in lib.take()] == ["hmm_shadow_store_build", "hmm_cosine_topk_segmented_prefilter", "hmm_rank_segment_hits"]
    assert vo.EventStore([], device=CPU).top_hits(_query(), K, keep) == []     # no event: the scan is still called, nothing is ranked
    assert [c[0] for c in lib.take()] == ["hmm_cosine_topk_segmented"]


# ---- the packed layouts ---------------------------------------------------------------------------------------------------------
def _fill(layout):
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, layout.nbytes, dtype=np.uint8)
    return raw, torch.from_numpy(raw.copy())


@pytest.mark.parametrize("lead", [(3,), (17, 3)])
def test_hits_layout(lead):
    layout = vo._hits_layout(*lead, 5)
    cells = int(np.prod(lead)) * 5
    assert layout.offsets == [0, cells * 8, cells * 12] and layout.nbytes == cells * 12 + int(np.prod(lead)) * 4
    raw, dev = _fill(layout)
    d_idx, d_sims, d_counts = layout.device_views(dev)
    h_idx, h_sims, h_counts = layout.host_views(raw)
    assert (d_idx.dtype, d_sims.dtype, d_counts.dtype) == (torch.int64, torch.float32, torch.int32)
    assert (h_idx.dtype, h_sims.dtype, h_counts.dtype) == (np.int64, np.float32, np.int32)
    assert d_idx.shape == h_idx.shape == d_sims.shape == h_sims.shape == lead + (5,) and d_counts.shape == h_counts.shape == lead
    assert [v.data_ptr() - dev.data_ptr() for v in (d_idx, d_sims, d_counts)] == layout.offsets
    for d, h in zip((d_idx, d_sims, d_counts), (h_idx, h_sims, h_counts)):
        assert d.numpy().tobytes() == h.tobytes()                              # the same bits, NaN patterns included
    d_idx[-1, ..., -1] = -1                                                    # views, not copies
    assert dev[cells * 8 - 8: cells * 8].tolist() == [255] * 8


@pytest.mark.parametrize("lead", [(), (17,)])
def test_ranking_layout(lead):
    layout = vo._ranking_layout(*lead, 5)
    cells = int(np.prod(lead)) * 5
    assert layout.offsets == [0, cells * 8, cells * 16, cells * 20] and layout.nbytes == cells * 20 + int(np.prod(lead)) * 4
    raw, dev = _fill(layout)
    device, host = layout.device_views(dev), layout.host_views(raw)
    assert [v.dtype for v in device] == [torch.int64, torch.int64, torch.float32, torch.int32]
    assert [v.dtype for v in host] == [np.int64, np.int64, np.float32, np.int32]
    assert [tuple(v.shape) for v in device] == [v.shape for v in host] == [lead + (5,)] * 3 + [lead or (1,)]     # one count per question
    assert [v.data_ptr() - dev.data_ptr() for v in device] == layout.offsets
    for d, h in zip(device, host):
        assert d.numpy().tobytes() == h.tobytes()
