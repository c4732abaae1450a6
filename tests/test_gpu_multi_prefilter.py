"""GPU parity of the batched scans through the bf16 shadow (hmm_cosine_topk_multi_prefilter,
hmm_cosine_topk_segmented_multi_prefilter): each must return what its exact counterpart (hmm_cosine_topk_multi,
hmm_cosine_topk_segmented_multi) returns on the same inputs -- the same indices, the same similarity BITS, the same counts -- on
random stores on both sides of the dispatch limits, on stores where the bf16 error exceeds the rank gaps, on ties, NaN rows, zero
and NaN questions, and through the Python route; `stats` tells which route answered."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NQS = (1, 5, 16, 17, 33)


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cuda").manual_seed(seed), device="cuda")


def _dev(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def flat_both(fs, queries, k):
    """(exact idx, exact sims, shadow-route idx, shadow-route sims, stats (Q,2) list) for one FeatureStore."""
    q = _dev(queries)
    stats = torch.full((q.shape[0], 2), -7, dtype=torch.int32, device="cuda")
    i0, s0 = fs.search_multi_device(q, k, prefilter=False)
    i0, s0 = i0.clone(), s0.clone()
    i1, s1 = fs.search_multi_device(q, k, prefilter=True, stats=stats)
    return i0, s0, i1, s1, stats.cpu()


def assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        if x.dtype == torch.float32:
            assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))      # the same bits, NaN included
        else:
            assert torch.equal(x, y)


@pytest.mark.parametrize("n,k", [(1, 1), (63, 5), (16383, 32), (16384, 32), (16385, 1), (20000, 5), (20000, 64), (20000, 65),
                                 (70001, 32), (300001, 64)])
def test_equals_the_exact_batched_scan_on_random_stores(n, k):
    from hippomm_amd.vector_ops import FeatureStore
    fs = FeatureStore(_randn((n, 1024), n * 17 + k))
    queries = _randn((max(NQS), 1024), n + k)
    for nq in NQS:
        i0, s0, i1, s1, stats = flat_both(fs, queries[:nq], k)
        assert_same((i0, s0), (i1, s1))
        print(f"n={n} k={k} nq={nq} candidates {stats[:, 0].min().item()}..{stats[:, 0].max().item()} saturated {stats[:, 1].max().item()}")
        if n >= 16384 and k <= 64 and n > k:
            assert (stats[:, 1] == 0).all() and (stats[:, 0] >= k).all() and (stats[:, 0] <= 1024).all(), stats.tolist()
        else:
            assert (stats == -1).all(), stats.tolist()           # outside the limits the call IS the exact function


def _events(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, 1024), dtype=np.float32) for n in sizes]


def seg_both(es, queries, k):
    q = _dev(queries)
    stats = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    r0 = tuple(t.clone() for t in es.search_segments_multi_device(q, es.offsets, k))
    r1 = es.search_segments_multi_device(q, es.offsets, k, prefilter=True, stats=stats)
    return r0, r1, stats.cpu().tolist()


@pytest.mark.parametrize("sizes,k", [([300, 1, 0, 57, 5, 4096, 4097, 2], 5), ([9000, 3, 12000], 32), ([40] * 200, 5), ([500] * 64, 5),
                                     ([1500, 2, 0, 700, 1025, 64, 3000, 1], 5), ([200] * 50, 64),
                                     ([5000], 64), ([5000], 100), ([1019, 1020, 1024, 1025, 2039, 2044, 1, 0, 2, 3], 5)])
def test_per_event_equals_the_exact_batched_per_event_scan(sizes, k):
    """Empty and one-row events, events above one chunk, a tie and a zero row inside an event, k = 64 and k = 100, with 5 and with 17
    questions.  The last list crosses the SMALL chunk (1024 keys: its events average at most 1024 rows) with a carry of k = 5, see
    tests/test_gpu_scan_prefilter.py."""
    from hippomm_amd.vector_ops import EventStore
    events = _events(sizes, seed=len(sizes) * 7 + k)
    if len(events) > 3 and events[3].shape[0] > 10:
        events[3][7] = events[3][2]
        events[3][9] = 0.0
    es = EventStore(events)
    queries = _randn((17, 1024), 1)
    for nq in (5, 17):
        r0, r1, stats = seg_both(es, queries[:nq], k)
        assert_same(r0, r1)
        print(f"sizes={sizes[:4]}.. k={k} nq={nq} stats {stats}")
        if k <= 64 and sum(sizes) // len(sizes) >= 128:
            assert stats[0] == 0 and stats[1] >= nq * sum(min(k, n) for n in sizes), stats       # at least its k best per (event, question)
        else:
            assert stats == [-1, -1], stats


def test_scene_clusters_where_the_bf16_error_exceeds_the_rank_gaps():
    """600 scenes of 40 near-identical frames, 16 different questions, several aimed at different scenes: inside a winning scene the
    approximate order is wrong, only the margin and the exact re-score can be right."""
    from hippomm_amd.vector_ops import FeatureStore
    rng = np.random.default_rng(5)
    scenes = rng.standard_normal((600, 1024), dtype=np.float32)
    store = np.repeat(scenes, 40, axis=0) + 2e-3 * rng.standard_normal((24000, 1024), dtype=np.float32)
    queries = rng.standard_normal((16, 1024), dtype=np.float32)
    aimed = {0: 123, 3: 77, 7: 599, 12: 0, 15: 300}
    for slot, scene in aimed.items():
        queries[slot] = scenes[scene] + 0.5 * scenes[(scene + 41) % 600] + 0.05 * rng.standard_normal(1024, dtype=np.float32)
    fs = FeatureStore(store)
    for k in (5, 32, 64):
        i0, s0, i1, s1, stats = flat_both(fs, queries, k)
        assert_same((i0, s0), (i1, s1))
        for slot in aimed:
            assert stats[slot, 0] >= 40 or stats[slot, 1] > 0, stats.tolist()      # the whole winning scene had to be re-scored
    for slot, scene in aimed.items():
        rows = torch.from_numpy(store[scene * 40:(scene + 1) * 40]).cuda()
        q = torch.from_numpy(queries[slot]).cuda()
        approx = ((rows / rows.norm(dim=1, keepdim=True)).to(torch.bfloat16).float() @ q).cpu().numpy()
        exact = (rows.double() @ q.double() / rows.double().norm(dim=1)).cpu().numpy()
        assert np.argsort(-approx).tolist() != np.argsort(-exact).tolist()


@pytest.mark.parametrize("slot", [0, 15])
def test_question_aligned_with_the_rounding_error_of_its_best_row(slot):
    from hippomm_amd.vector_ops import FeatureStore
    rng = np.random.default_rng(9)
    store = rng.standard_normal((30000, 1024), dtype=np.float32)
    v = store[4321] / np.linalg.norm(store[4321])
    e = torch.from_numpy(v).to(torch.bfloat16).float().numpy() - v
    for j in range(64):                                          # decoys: a little further from v than v itself
        store[100 + 7 * j] = v + (0.02 + 0.0005 * j) * rng.standard_normal(1024).astype(np.float32) / 32
    queries = rng.standard_normal((16, 1024), dtype=np.float32)
    queries[slot] = (v - 0.6 * e / np.linalg.norm(e)).astype(np.float32)
    i0, s0, i1, s1, stats = flat_both(FeatureStore(store), queries, 32)
    assert_same((i0, s0), (i1, s1))
    assert 4321 in i1[slot].tolist()


def test_many_exact_ties_and_nan_rows_take_the_fallback():
    from hippomm_amd.vector_ops import FeatureStore
    rng = np.random.default_rng(11)
    base = rng.standard_normal((16, 1024), dtype=np.float32)
    store = base[rng.integers(0, 16, size=40000)]                # every row ~2500 times
    store[[17, 4000, 39999]] = 0.0                               # NaN rows rank first
    queries = rng.standard_normal((16, 1024), dtype=np.float32)
    fs = FeatureStore(store)
    for k in (3, 32):
        i0, s0, i1, s1, stats = flat_both(fs, queries, k)
        assert_same((i0, s0), (i1, s1))
        assert (i1[:, :3].cpu() == torch.tensor([39999, 4000, 17])).all() and torch.isnan(s1[:, :3]).all()
        if k == 3:                                               # the k best are the three NaN rows: a NaN threshold, only they pass, the shadow answers
            assert (stats[:, 0] == 3).all() and (stats[:, 1] == 0).all(), stats.tolist()
        else:                                                    # ~2500 equal best rows per question: the exact pass answered
            assert ((stats[:, 1] > 0) | (stats[:, 0] > 1024)).all(), stats.tolist()


def test_zero_and_nan_questions_among_normal_ones():
    from hippomm_amd.vector_ops import FeatureStore
    fs = FeatureStore(_randn((20000, 1024), 1))
    queries = _randn((16, 1024), 2)
    queries[4] = 0.0
    queries[11] = float("nan")
    i0, s0, i1, s1, stats = flat_both(fs, queries, 4)
    assert_same((i0, s0), (i1, s1))
    for bad in (4, 11):
        assert i1[bad].tolist() == [19999, 19998, 19997, 19996] and torch.isnan(s1[bad]).all()
        assert stats[bad, 1] > 0 or stats[bad, 0] > 1024, stats.tolist()
    good = [i for i in range(16) if i not in (4, 11)]
    ia, sa = fs.search_multi_device(queries[good], 4, prefilter=False)
    assert_same((ia, sa), (i1[good], s1[good]))                   # the others are what they are without the bad two


def test_events_of_near_identical_rows_are_rescored_whole():
    from hippomm_amd.vector_ops import EventStore
    rng = np.random.default_rng(3)
    sizes = [300, 2000, 40, 300]
    events = []
    for n in sizes:
        c = rng.standard_normal(1024).astype(np.float32)
        events.append(c + 1e-3 * rng.standard_normal((n, 1024), dtype=np.float32))
    es = EventStore(events)
    queries = rng.standard_normal((5, 1024)).astype(np.float32)
    queries[2] = events[1][5] + 0.3 * rng.standard_normal(1024)
    for k in (5, 32):
        r0, r1, stats = seg_both(es, queries, k)
        assert_same(r0, r1)
        assert stats[0] >= 5 and stats[1] >= 5 * 2000, stats       # the 2000-row event: every row, for every question
    assert es.top_hits_multi(queries, 5, 5, prefilter=True) == es.top_hits_multi(queries, 5, 5)
    a, b = es.top_k_per_event_multi(queries, 5, prefilter=True), es.top_k_per_event_multi(queries, 5)
    assert all(x[0].tolist() == y[0].tolist() and x[1].tobytes() == y[1].tobytes() for qa, qb in zip(a, b) for x, y in zip(qa, qb))


def test_per_event_slice_equals_the_flat_call_on_that_events_rows():
    """Slice (q, e) of the per-event result equals the flat prefiltered call on event e's rows alone: an event at the start, in the
    middle and at the end of the store (each large enough for the flat shadow route)."""
    from hippomm_amd.vector_ops import EventStore, FeatureStore
    sizes = [17000, 300, 16500, 129, 20001]
    rows = _randn((sum(sizes), 1024), 21)
    es = EventStore.from_device_rows(rows, sizes)
    queries = _randn((5, 1024), 22)
    k = 7
    idx, sims, counts = es.search_segments_multi_device(queries, es.offsets, k, prefilter=True)
    off = np.cumsum([0] + sizes)
    for e in (0, 2, 4):
        stats = torch.full((5, 2), -7, dtype=torch.int32, device="cuda")
        fi, fsim = FeatureStore(rows[off[e]:off[e + 1]]).search_multi_device(queries, k, prefilter=True, stats=stats)
        assert (stats[:, 0] >= k).all() and (stats[:, 1] == 0).all()
        assert_same((idx[:, e], sims[:, e]), (fi, fsim))
        assert (counts[:, e] == k).all()


def test_feature_store_with_shadow_serves_search_multi_identically():
    from hippomm_amd.vector_ops import FeatureStore
    rng = np.random.default_rng(77)
    for dtype in (np.float32, np.float64):
        store = rng.standard_normal((30000, 1024)).astype(np.float32).astype(dtype)
        queries = rng.standard_normal((7, 1024)).astype(np.float32)
        plain, shadowed = FeatureStore(store), FeatureStore(store, shadow=True)
        for k in (5, 32, 100):
            for (i0, s0), (i1, s1) in zip(plain.search_multi(queries, k), shadowed.search_multi(queries, k)):
                assert i0.tolist() == i1.tolist() and s0.dtype == s1.dtype and s0.tobytes() == s1.tobytes()
        stats = torch.full((7, 2), -7, dtype=torch.int32, device="cuda")
        for (i0, s0), (i1, s1) in zip(plain.search_multi(queries, 5), shadowed.search_multi(queries, 5, prefilter=True)):
            assert i0.tolist() == i1.tolist() and s0.tobytes() == s1.tobytes()
        shadowed.search_multi_device(torch.from_numpy(queries).cuda(), 5, prefilter=True, stats=stats)
        assert (stats[:, 0] >= 5).all() and (stats[:, 1] == 0).all()                         # asked for, the shadow answers


def test_shadow_follows_in_place_updates_of_the_rows():
    from hippomm_amd.vector_ops import FeatureStore
    rows = _randn((40000, 1024), 5)
    queries = _randn((5, 1024), 6)
    store = FeatureStore(rows, shadow=True)
    assert store.rows.data_ptr() == rows.data_ptr()
    i0, _ = store.search_multi_device(queries, 8, prefilter=True)
    target = int((torch.arange(40000, device="cuda")[~torch.isin(torch.arange(40000, device="cuda"), i0.reshape(-1))])[12345].item())
    rows[target] = queries[3] * 3.0                              # in place, through torch: the version counter moves
    stats = torch.full((5, 2), -7, dtype=torch.int32, device="cuda")
    i1, s1 = store.search_multi_device(queries, 8, prefilter=True, stats=stats)  # the shadow is rebuilt first
    ie, se = FeatureStore(rows).search_multi_device(queries, 8)
    assert int(i1[3, 0].item()) == target and (stats[:, 1] == 0).all() and (stats[:, 0] >= 8).all()
    assert_same((i1, s1), (ie, se))
