"""GPU: the store that grows on the device -- hmm_store_ingest_rows, hmm_store_gather_segments and the EventStore methods on top of
them (reserve / append_event / extend / remove_events / replace_event, event_store.refresh_event_store).

The yardstick throughout is the path that existed before: a fresh ``EventStore(list_of_events)`` and ``hmm_shadow_store_build`` on
the rows in question, compared byte for byte.  There are no tolerances.  Buffers of the raw calls are carved from a poisoned,
guarded arena (tests/arena.py) at exactly their capacity, so a byte written outside the rows a call owns is seen."""
import json

import numpy as np
import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 1024


def _lib():
    from hippomm_amd import _lib as L
    return L, L.load()


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _rows(n, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal((n, D))).astype(np.float32)


def shadow_rows_of(rows_dev):
    """hmm_shadow_store_build on an (n,1024) fp32 device matrix: (n, 2048) bytes."""
    L, lib = _lib()
    n = rows_dev.shape[0]
    out = torch.empty(n * 2048, dtype=torch.uint8, device=rows_dev.device)
    if n:
        L.check(lib.hmm_shadow_store_build(rows_dev.data_ptr(), n, D, out.data_ptr(), out.numel(), L.stream_ptr()), "hmm_shadow_store_build")
    return out.view(n, 2048)


def ingest(src_ptr, dtype, n, store_ptr, shadow_ptr, capacity, at):
    L, lib = _lib()
    L.check(lib.hmm_store_ingest_rows(src_ptr, dtype, n, D, store_ptr, shadow_ptr, capacity, at, L.stream_ptr()), "hmm_store_ingest_rows")
    torch.cuda.synchronize()


# ---- 1. ingest, fp32 --------------------------------------------------------------------------------------------------------
CAPACITY = 80


@pytest.mark.parametrize("n", [1, 3, 4, 5, 67])
def test_ingest_fp32_writes_its_rows_and_their_shadow_rows_and_nothing_else(n):
    src_host = _rows(n, 100 + n)
    src_host[-1, :4] = [-0.0, 1e-40, -3e-42, 0.0]                             # moved as bits, and harmless to the row's norm
    want_rows = _bytes(torch.from_numpy(src_host)).to(DEV)
    want_shadow = shadow_rows_of(torch.from_numpy(src_host).to(DEV)).reshape(-1)
    for pattern in ("ones", "big"):
        for at in sorted({0, 1, CAPACITY - n}):
            for with_shadow in (True, False):
                ar = A.GuardedArena(A.needed_bytes([n * 4096, CAPACITY * 4096, CAPACITY * 2048]), DEV, A.PATTERNS[pattern])
                src = ar.put(torch.from_numpy(src_host).to(DEV), "source")
                store = ar.carve(CAPACITY * 4096, "store")
                shadow = ar.carve(CAPACITY * 2048, "shadow")
                exp_store, exp_shadow = store.clone(), shadow.clone()
                exp_store[at * 4096: (at + n) * 4096] = want_rows
                if with_shadow:
                    exp_shadow[at * 2048: (at + n) * 2048] = want_shadow
                ingest(ar.address(src), 0, n, ar.address(store), ar.address(shadow) if with_shadow else None, CAPACITY, at)
                what = (pattern, at, with_shadow)
                assert torch.equal(store, exp_store), what                   # the rows, and every other byte unchanged
                assert torch.equal(shadow, exp_shadow), what
                assert torch.equal(src, want_rows), what
                ar.check_guards()


def test_ingest_fp32_keeps_every_bit_pattern():
    bits = np.random.default_rng(7).integers(0, 2 ** 32, size=(5, D), dtype=np.uint64).astype(np.uint32)
    bits[0, :6] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF]     # NaN payloads, a signalling NaN, -0.0, subnormals
    src = torch.from_numpy(bits.view(np.int32)).to(DEV)
    store = torch.zeros(9, D, dtype=torch.int32, device=DEV)
    ingest(src.data_ptr(), 0, 5, store.data_ptr(), None, 9, 2)
    assert torch.equal(store[2:7], src) and not store[:2].any() and not store[7:].any()


# ---- 2. ingest, fp64 --------------------------------------------------------------------------------------------------------
def _fp64_source():
    rng = np.random.default_rng(11)
    a = rng.standard_normal((4, D))                                           # random doubles that need rounding
    # exact ties: an fp32 value plus half an ulp, last bit even and odd -> round to nearest EVEN decides
    f = rng.standard_normal(256).astype(np.float32)
    even = (f.view(np.uint32) & np.uint32(0xFFFFFFFE)).view(np.float32)
    odd = (f.view(np.uint32) | np.uint32(1)).view(np.float32)
    for j, lo in enumerate((even, odd)):
        hi = np.nextafter(lo, np.where(lo > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        a[1, j * 256: (j + 1) * 256] = (lo.astype(np.float64) + hi.astype(np.float64)) / 2      # exact in double
    flt_max = float(np.finfo(np.float32).max)
    to_inf = flt_max + 2.0 ** 103                                             # the tie between FLT_MAX and 2^128: the smallest double that rounds to infinity
    special = [0.0, -0.0, 1e-40, -3e-42, 2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, np.nextafter(2.0 ** -150, 1.0),
               1e-320, 2.0 ** -126, np.nextafter(2.0 ** -126, 0.0), 1e39, -1e39, to_inf, -to_inf, np.nextafter(to_inf, 0.0),
               -np.nextafter(to_inf, 0.0), flt_max, np.inf, -np.inf, np.nan, 1e300, -1e300]
    a[2, : len(special)] = special                                            # row 2: holds a NaN and infinities
    a[3] *= 1e-3                                                              # a second ordinary row behind the special one
    return a


def test_ingest_fp64_narrows_as_numpy_astype_does():
    src_host = _fp64_source()
    with np.errstate(over="ignore"):
        want = src_host.astype(np.float32)
    n, cap, at = src_host.shape[0], 9, 3
    ar = A.GuardedArena(A.needed_bytes([n * 8192, cap * 4096, cap * 2048]), DEV, A.PATTERNS["big"])
    src = ar.put(torch.from_numpy(src_host).to(DEV), "source")
    store = ar.carve(cap * 4096, "store")
    shadow = ar.carve(cap * 2048, "shadow")
    before_store, before_shadow = store.clone(), shadow.clone()
    ingest(ar.address(src), 1, n, ar.address(store), ar.address(shadow), cap, at)
    got = store[at * 4096: (at + n) * 4096].view(torch.float32).view(n, D).cpu().numpy()
    nan = np.isnan(want)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.isinf(got[2]).sum() == 8 and (got[2] == 0).sum() >= 4           # the cases are what they claim to be
    # shadow rows: those of the narrowed rows (row 2 holds a NaN, whose payload in a product is not pinned: all of it is NaN)
    got_shadow = shadow[at * 2048: (at + n) * 2048].view(n, 2048)
    want_shadow = shadow_rows_of(torch.from_numpy(want).to(DEV))
    for r in (0, 1, 3):
        assert torch.equal(got_shadow[r], want_shadow[r]), r
    assert bool((got_shadow[2].view(torch.int16) & 0x7FFF > 0x7F80).all())
    assert torch.equal(store[: at * 4096], before_store[: at * 4096]) and torch.equal(store[(at + n) * 4096:], before_store[(at + n) * 4096:])
    assert torch.equal(shadow[: at * 2048], before_shadow[: at * 2048]) and torch.equal(shadow[(at + n) * 2048:], before_shadow[(at + n) * 2048:])
    ar.check_guards()


# ---- 3. special rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
def test_shadow_of_zero_infinite_and_overflowing_rows_is_the_builds(dtype):
    rows = _rows(5, 21)
    rows[0] = 0.0                                                             # zero norm
    rows[1, 77] = np.inf                                                      # a row with an inf
    rows[2] *= 1e20                                                           # finite entries, the squared norm overflows fp32
    rows[3] *= 1e-30                                                          # ... and one that underflows to zero
    want_shadow = shadow_rows_of(torch.from_numpy(rows).to(DEV))
    assert all(bool((want_shadow[r].view(torch.int16) & 0x7FFF > 0x7F80).all()) for r in range(4))          # the build's NaN rows
    src = torch.from_numpy(rows.astype(np.float64) if dtype else rows).to(DEV)
    store = torch.empty(5, D, dtype=torch.float32, device=DEV)
    shadow = torch.empty(5, 2048, dtype=torch.uint8, device=DEV)
    ingest(src.data_ptr(), dtype, 5, store.data_ptr(), shadow.data_ptr(), 5, 0)
    assert torch.equal(_bytes(store), _bytes(torch.from_numpy(rows).to(DEV)))
    assert torch.equal(shadow, want_shadow)


# ---- 4. gather ---------------------------------------------------------------------------------------------------------------
SRC_LENGTHS = [3, 0, 1, 17, 64, 65]


def _gather_case(pattern, src_segment, dst_lengths, dst_rows, dst_capacity, with_shadow=True):
    L, lib = _lib()
    src_host = _rows(sum(SRC_LENGTHS), 31)
    src_dev = torch.from_numpy(src_host).to(DEV)
    src_off = np.concatenate([[0], np.cumsum(SRC_LENGTHS)]).astype(np.int64)
    dst_off = np.concatenate([[0], np.cumsum(dst_lengths)]).astype(np.int64)
    ar = A.GuardedArena(A.needed_bytes([src_host.nbytes, src_host.nbytes // 2, dst_capacity * 4096, dst_capacity * 2048, 256, 256, 256]),
                        DEV, A.PATTERNS[pattern])
    src = ar.put(src_dev, "source rows")
    src_sh = ar.put(shadow_rows_of(src_dev), "source shadow")
    dst = ar.carve(dst_capacity * 4096, "destination rows")
    dst_sh = ar.carve(dst_capacity * 2048, "destination shadow")
    t_src_off = ar.put(torch.from_numpy(src_off).to(DEV), "source offsets")
    t_seg = ar.put(torch.tensor(src_segment, dtype=torch.int32, device=DEV), "segment table")
    t_dst_off = ar.put(torch.from_numpy(dst_off).to(DEV), "destination offsets")
    exp, exp_sh = dst.clone(), dst_sh.clone()
    for j, s in enumerate(src_segment):
        if s < 0 or s >= len(SRC_LENGTHS):
            continue
        rows = min(SRC_LENGTHS[s], dst_lengths[j], max(0, dst_rows - int(dst_off[j])))
        a, b = int(dst_off[j]), int(src_off[s])
        exp[a * 4096: (a + rows) * 4096] = src[b * 4096: (b + rows) * 4096]
        if with_shadow:
            exp_sh[a * 2048: (a + rows) * 2048] = src_sh[b * 2048: (b + rows) * 2048]
    L.check(lib.hmm_store_gather_segments(ar.address(src), ar.address(src_sh) if with_shadow else None, sum(SRC_LENGTHS),
                                          ar.address(t_src_off), len(SRC_LENGTHS), ar.address(t_seg), ar.address(t_dst_off),
                                          len(src_segment), D, ar.address(dst), ar.address(dst_sh) if with_shadow else None, dst_rows,
                                          dst_capacity, L.stream_ptr()), "hmm_store_gather_segments")
    torch.cuda.synchronize()
    assert torch.equal(dst, exp)                                              # rows where the table says; the hole and the spare capacity keep their poison
    assert torch.equal(dst_sh, exp_sh)
    ar.check_guards()
    return ar, dst, dst_sh


@pytest.mark.parametrize("pattern", ["ones", "big"])
def test_gather_moves_events_and_their_shadow_rows_where_the_table_says(pattern):
    ar, dst, dst_sh = _gather_case(pattern, [5, -1, 0, 3], [65, 4, 3, 17], 89, 100)
    assert ar.is_pattern(dst, 89 * 4096) and ar.is_pattern(dst_sh, 89 * 2048)             # at and beyond dst_rows
    _gather_case(pattern, [5, -1, 0, 3], [65, 4, 3, 17], 89, 100, with_shadow=False)      # both shadows null: the shadow keeps its poison


def test_gather_with_a_wrong_table_copies_less_never_elsewhere():
    _gather_case("ones", [0, 3], [5, 17], 22, 22)                             # destination segment longer than its source: 3 rows copied
    _gather_case("ones", [4, 2, 9, 5], [64, 1, 7, 65], 137, 140)              # a source segment that does not exist: skipped
    _gather_case("ones", [5, 4], [65, 64], 100, 129)                          # a table that runs past dst_rows: cut there
    _gather_case("ones", [1, 1, 2, 1], [0, 0, 1, 0], 1, 1)                    # empty segments around a single row


# ---- 5. / 6. a growing store equals a fresh one ------------------------------------------------------------------------------
QUERIES = _rows(3, 41)


def _bits_np(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_pairs(a, b):
    assert len(a) == len(b)
    for (ia, sa), (ib, sb) in zip(a, b):
        assert np.array_equal(ia, ib) and np.array_equal(_bits_np(sa), _bits_np(sb))


def _same_hits(a, b):
    assert [(e, r, np.float32(v).view(np.uint32)) for e, r, v in a] == [(e, r, np.float32(v).view(np.uint32)) for e, r, v in b]


def assert_equals_fresh(store, events, prefilter=False):
    """`store` against EventStore(events): rows, offsets, lengths and what every search returns, indices and similarity bits."""
    from hippomm_amd.vector_ops import EventStore
    fresh = EventStore(events)
    assert list(store.lengths) == list(fresh.lengths) and len(store) == len(fresh)
    assert store.offsets.dtype == fresh.offsets.dtype and torch.equal(store.offsets, fresh.offsets)
    assert store.rows.shape == fresh.rows.shape and store.rows.is_contiguous() and store.rows.dtype == torch.float32
    assert torch.equal(_bytes(store.rows), _bytes(fresh.rows))
    if getattr(store, "_shadow", None) is not None and len(store) > 0:
        fresh.build_shadow()
        assert torch.equal(store._shadow, fresh._shadow)
    _same_pairs(*[[p for per_query in s.top_k_per_event_multi(QUERIES, 5, prefilter) for p in per_query] for s in (store, fresh)])
    for a, b in zip(store.top_hits_multi(QUERIES, 5, 7, prefilter), fresh.top_hits_multi(QUERIES, 5, 7, prefilter)):
        _same_hits(a, b)
    if len(store) == 0:
        return fresh
    _same_pairs([store.search(QUERIES[0], 5)], [fresh.search(QUERIES[0], 5)])
    _same_pairs(store.top_k_per_event(QUERIES[1], 5, prefilter), fresh.top_k_per_event(QUERIES[1], 5, prefilter))
    _same_hits(store.top_hits(QUERIES[2], 5, 7, prefilter), fresh.top_hits(QUERIES[2], 5, 7, prefilter))
    return fresh


def _poison_spare_capacity(store):
    """NaN ranks first in this library's order: a scan that reads beyond the store's n rows shows up in every result.  Written
    through .data, which does not touch the version counter the shadow bookkeeping watches."""
    n = len(store)
    store._buf.data[n:].fill_(float("nan"))
    if getattr(store, "_shadow_buf", None) is not None:
        store._shadow_buf.data[n * 2048:].fill_(0xFF)


GROW_LENGTHS = [3, 0, 1, 17, 64, 65, 200]


def _grow_sources():
    """(what append_event is given, what the constructor is given) per event: numpy float32, numpy float64, a CUDA float32
    tensor, a CUDA float64 tensor and a 1-D row, in turn."""
    out = []
    for i, n in enumerate(GROW_LENGTHS):
        kind = i % 4 if n != 1 else 4
        host64 = np.random.default_rng(50 + i).standard_normal((n, D))
        host = host64.astype(np.float32) if kind in (0, 2, 4) else host64
        if kind == 4:
            host = host.reshape(D)
        given = torch.from_numpy(host).to(DEV) if kind in (2, 3) else host
        out.append((given, host))
    return out


def _grown_store(shadow_after=2):
    from hippomm_amd.vector_ops import EventStore
    store = EventStore([]).reserve(64)
    assert store.capacity == 64 and len(store) == 0
    events = []
    for i, (given, host) in enumerate(_grow_sources()):
        n_before, capacity, ptr = len(store), store.capacity, store.rows.data_ptr()
        assert store.append_event(given) == i
        events.append(host)
        needed = n_before + GROW_LENGTHS[i]
        if needed <= capacity:
            assert store.capacity == capacity
            assert n_before == 0 or store.rows.data_ptr() == ptr             # nothing moved while the capacity sufficed
        else:
            assert store.capacity == max(needed, 2 * capacity)
            assert store.rows.data_ptr() != ptr                              # ... and it moved exactly when it did not
        if i == shadow_after:
            store.build_shadow()
        _poison_spare_capacity(store)
        yield store, events


def test_a_growing_store_equals_a_fresh_one_after_every_append():
    steps = 0
    for store, events in _grown_store():
        assert_equals_fresh(store, events)
        steps += 1
    assert steps == len(GROW_LENGTHS) and store.capacity == 512 and len(store) == 350


@pytest.mark.parametrize("shadow", [False, True])
def test_remove_and_replace_equal_the_edited_list(shadow):
    for store, events in _grown_store(shadow_after=2 if shadow else -1):
        pass
    events = list(events)
    assert (store._shadow is not None) == shadow

    def check():
        assert (store._shadow is not None) == shadow                          # a shadow travels with its rows, none appears by itself
        _poison_spare_capacity(store)
        return assert_equals_fresh(store, events)

    big = torch.from_numpy(_rows(400, 61)).to(DEV)
    store.replace_event(6, big)                                               # beyond the capacity: 150 + 400 rows > 512
    events[6] = big.cpu().numpy()
    assert store.capacity == 1024
    check()
    longer, shorter = _rows(30, 62).astype(np.float64), torch.from_numpy(_rows(7, 63)).to(DEV)
    ptr = store._buf.data_ptr()
    store.replace_event(2, longer)
    events[2] = longer
    check()
    assert store._buf.data_ptr() != ptr and store.capacity == 1024             # out of place, the same capacity
    store.replace_event(-2, shorter)
    events[-2] = shorter.cpu().numpy()
    check()
    for drop in ([1], [0], [-1], [1]):                                        # the empty event, the first, the last, one in the middle
        store.remove_events(drop)
        for j in sorted((d % len(events) for d in drop), reverse=True):
            del events[j]
        check()
    assert [len(np.atleast_2d(e)) for e in events] == [30, 64, 7]
    before = (store._buf.data_ptr(), list(store.lengths), store.offsets.clone(), store.rows.clone())
    for bad, error in (([3], IndexError), ([-4], IndexError), ([0, 0], ValueError), ([0, -3], ValueError), ([1, 7], IndexError)):
        with pytest.raises(error):
            store.remove_events(bad)
    with pytest.raises(IndexError):
        store.replace_event(3, longer)
    with pytest.raises(ValueError):
        store.replace_event(0, _rows(2, 64)[:, :512])
    with pytest.raises(ValueError):
        store.append_event(store.rows[:2])                                    # a source inside the store's own buffer
    assert (store._buf.data_ptr(), list(store.lengths)) == before[:2] and torch.equal(store.offsets, before[2])
    assert torch.equal(store.rows, before[3])
    store.remove_events([0, 2])                                               # two at once
    del events[2], events[0]
    check()
    store.remove_events([0])                                                  # everything: behaves as EventStore([])
    events = []
    fresh = check()
    assert len(store) == 0 and store.lengths == [] and store.top_k_per_event_multi(QUERIES, 5) == fresh.top_k_per_event_multi(QUERIES, 5)
    assert store.append_event(_rows(4, 65)) == 0                              # ... and grows again
    events = [_rows(4, 65)]
    check()


# ---- 7. shadow kept current ------------------------------------------------------------------------------------------------
def test_appends_keep_the_shadow_current_without_rebuilding_it(monkeypatch):
    """33 events of 500 rows: 16 500 rows, above both dispatch limits of the shadow routes (16 384 rows; 128 rows per event)."""
    from hippomm_amd.vector_ops import EventStore
    L, lib = _lib()
    rng = np.random.default_rng(71)
    events = [rng.standard_normal((500, D), dtype=np.float32) for _ in range(33)]
    q = _rows(1, 72)[0]
    q_dev = torch.from_numpy(q).to(DEV)

    def answers(store):
        stats = torch.zeros(2, dtype=torch.int32, device=DEV)
        idx, sims = store.search_prefiltered_device(q_dev, 5, stats)
        return (idx.cpu(), _bytes(sims).cpu(), stats.cpu(), store.top_k_per_event(q, 5, prefilter=True),
                store.search_multi(QUERIES, 5, prefilter=True))

    fresh = EventStore(events).build_shadow()
    want = answers(fresh)

    store = EventStore([])
    store.extend([torch.from_numpy(e).to(DEV) for e in events[:11]])
    store.build_shadow()
    with monkeypatch.context() as m:
        def no_rebuild(*args):
            raise AssertionError("an append rebuilt the whole shadow")
        m.setattr(lib, "hmm_shadow_store_build", no_rebuild)
        store.extend(events[11:22])                                           # from the host
        store.extend([torch.from_numpy(e.astype(np.float64)).to(DEV) for e in events[22:]])       # fp32 values as doubles: the same rows
        got = answers(store)
    assert len(store) == 16500 and torch.equal(store.offsets, fresh.offsets)
    assert torch.equal(_bytes(store.rows), _bytes(fresh.rows))
    assert torch.equal(store._shadow, fresh._shadow)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[2], want[2]) and int(got[2][0]) != -1              # the shadow route answered
    _same_pairs(got[3], want[3])
    _same_pairs(got[4], want[4])


# ---- 8. aliased stores -------------------------------------------------------------------------------------------------------
def test_a_store_over_the_callers_tensor_moves_out_before_it_changes():
    from hippomm_amd.vector_ops import EventStore
    host = _rows(50, 81)
    extra = _rows(6, 82)
    for change in ("append", "remove", "replace", "reserve"):
        mine = torch.from_numpy(host).to(DEV)
        kept = mine.clone()
        store = EventStore.from_device_rows(mine, [20, 30])
        assert store.rows.data_ptr() == mine.data_ptr()
        events = [host[:20], host[20:]]
        if change == "append":
            store.append_event(extra)
            events.append(extra)
        elif change == "remove":
            store.remove_events([0])
            del events[0]
        elif change == "replace":
            with pytest.raises(ValueError):
                store.replace_event(1, mine[:6])                               # a source inside the rows the store still aliases
            store.replace_event(1, torch.from_numpy(extra).to(DEV))
            events[1] = extra
        else:
            store.reserve(64)
        torch.cuda.synchronize()
        assert torch.equal(_bytes(mine), _bytes(kept)), change                # the caller's tensor is never written
        assert store.rows.data_ptr() != mine.data_ptr(), change
        assert_equals_fresh(store, events)


# ---- 9. refresh_event_store --------------------------------------------------------------------------------------------------
def test_refresh_event_store_follows_the_index(tmp_path):
    import recipes
    from hippomm_amd import event_store as es
    base = tmp_path / "memory_store"
    index = {}

    def save(i, features):
        event = dict(recipes.event_case(), features=features)
        eid = f"vid_{i * 1000}"
        p = es.save_event(event, base / "events" / "vid" / f"{eid}.json", write_sidecars=(i != 1))
        index[eid] = {"video_id": "vid", "start_time": float(i), "end_time": float(i + 1), "file_path": str(p)}
        (base / "event_index.json").write_text(json.dumps(index, indent=2))

    def assert_fresh(store, ids):
        fresh, fresh_ids = es.build_event_store(base)
        assert ids == fresh_ids == list(index)
        assert list(store.lengths) == list(fresh.lengths) and torch.equal(store.offsets, fresh.offsets)
        assert torch.equal(_bytes(store.rows), _bytes(fresh.rows))
        _same_pairs(*[[p for per_query in s.top_k_per_event_multi(QUERIES, 5) for p in per_query] for s in (store, fresh)])

    save(0, {"vision": _rows(9, 91), "audio": _rows(2, 92)})
    save(1, {"vision": _rows(4, 93)})
    store, ids = es.build_event_store(base)
    assert ids == list(index) and store.lengths == [9, 4]
    assert es.refresh_event_store(store, ids, base) == ids and store.lengths == [9, 4]          # nothing new: nothing happens
    save(2, {"vision": _rows(6, 94)})
    save(3, {"audio": _rows(3, 95)})                                          # no vision: an empty segment
    save(4, {"vision": _rows(1, 96)[0]})                                      # a 1-D feature: one row
    save(5, {"vision": _rows(3, 97)[:, :512]})                                # a wrong width: an empty segment
    ids = es.refresh_event_store(store, ids, base)
    assert store.lengths == [9, 4, 6, 0, 1, 0]
    assert_fresh(store, ids)
    del index["vid_1000"], index["vid_3000"]
    (base / "event_index.json").write_text(json.dumps(index, indent=2))
    save(6, {"vision": _rows(5, 98)})
    ids = es.refresh_event_store(store, ids, base)
    assert store.lengths == [9, 6, 1, 0, 5]
    assert_fresh(store, ids)
    audio, audio_ids = es.build_event_store(base, "audio")
    assert audio.lengths == [2, 0, 0, 0, 0]
    save(7, {"vision": _rows(2, 99), "audio": _rows(8, 90)})
    assert es.refresh_event_store(audio, audio_ids, base, modality="audio") == list(index) and audio.lengths == [2, 0, 0, 0, 0, 8]


# ---- one scratch buffer for every scan route ----------------------------------------------------------------------------------
def _snapshot(out):
    """A result as bytes on the host: tensors and arrays as (dtype, shape, bytes), lists and tuples element by element."""
    if isinstance(out, torch.Tensor):
        return (str(out.dtype), tuple(out.shape), _bytes(out).cpu().numpy().tobytes())
    if isinstance(out, np.ndarray):
        return (str(out.dtype), out.shape, out.tobytes())
    if isinstance(out, (list, tuple)):
        return [_snapshot(o) for o in out]
    return out


def test_every_route_shares_one_scratch_and_answers_as_a_fresh_store_does():
    """The scan routes keep ONE workspace per store, grown when a route needs more and otherwise handed on as the last route left
    it.  16 640 rows (the smallest store on which the flat shadow route runs its own kernels: n >= 4 x 4096), 8 events with an
    empty one among them and 2080 rows on average (the segmented shadow routes run their own kernels from 128), 17 questions (two
    passes of the batched routes), k = 5: every route and every read-back method, smallest workspace first, then largest first on
    the same store, then largest first on a store whose scratch starts empty -- each result against the same call on a store that
    has made no other call, byte for byte."""
    from hippomm_amd.vector_ops import EventStore
    lengths = [3000, 0, 129, 2511, 4096, 1, 4903, 2000]
    assert sum(lengths) == 130 * 128 and len(lengths) == 8
    rng = np.random.default_rng(77)
    rows = torch.from_numpy(rng.standard_normal((sum(lengths), D), dtype=np.float32)).to(DEV)
    q = torch.from_numpy(rng.standard_normal(D, dtype=np.float32)).to(DEV)
    qs = torch.from_numpy(rng.standard_normal((17, D), dtype=np.float32)).to(DEV)

    def store():
        return EventStore.from_device_rows(rows, lengths).build_shadow()

    calls = [lambda s: s.search_device(q, 5),
             lambda s: s.search_prefiltered_device(q, 5),
             lambda s: s.search_keys_device(q, 5),
             lambda s: s.search_segments_device(q, s.offsets, 5),
             lambda s: s.search_segments_device(q, s.offsets, 5, prefilter=True),
             lambda s: s.top_hits(q, 5, 5),
             lambda s: s.top_hits(q, 5, 5, prefilter=True),
             lambda s: s.top_k_per_event(q, 5),
             lambda s: s.top_k_per_event(q, 5, prefilter=True),
             lambda s: s.search_multi_device(qs, 5),
             lambda s: s.search_multi_device(qs, 5, prefilter=True),
             lambda s: s.search_segments_multi_device(qs, s.offsets, 5),
             lambda s: s.search_segments_multi_device(qs, s.offsets, 5, prefilter=True),
             lambda s: s.top_hits_multi(qs, 5, 5),
             lambda s: s.top_hits_multi(qs, 5, 5, prefilter=True),
             lambda s: s.top_k_per_event_multi(qs, 5),
             lambda s: s.top_k_per_event_multi(qs, 5, prefilter=True)]
    want = [_snapshot(call(store())) for call in calls]
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    store().search_prefiltered_device(q, 5, stats)
    assert stats[0].item() >= 0                                               # the shadow route's own kernels, not the exact scan behind it
    order = list(range(len(calls)))
    one, other = store(), store()
    for name, s, sequence in (("ascending", one, order), ("descending on the same store", one, order[::-1]),
                              ("descending on a new store", other, order[::-1])):
        for i in sequence:
            assert _snapshot(calls[i](s)) == want[i], (name, i)
    per_event = one.top_k_per_event(q, 5)
    assert [len(idx) for idx, _ in per_event] == [min(5, n) for n in lengths]  # the empty event and the one-row event among them
