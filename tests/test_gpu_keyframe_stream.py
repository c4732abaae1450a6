"""GPU: hippomm_amd.consolidation.KeyFrameSelector (hmm_keyframe_extend) -- a selection grown batch by batch lists, after every
batch, what the one-shot selection lists for the rows seen so far: the golden vectors under the batch partitions, the in-band
fixtures under every two-batch split (each near-threshold pair decided once by the new x kept kernel and once by the new x new
kernel), random in-band pairs cut by batch boundaries, other thresholds, kept counts that cross a tile edge, NaN rows, capacity
growth, streams, reset and the input kinds."""
import numpy as np
import pytest
import torch

import keyframe_stream_cases as K
import recipes
from oracle.consolidation_oracle import select_key_frames_exact

pytestmark = pytest.mark.gpu


def _selector(**kw):
    from hippomm_amd.consolidation import KeyFrameSelector
    return KeyFrameSelector(**kw)


def _one_shot(f, thr=0.9):
    from hippomm_amd.consolidation import select_key_frames_device
    return select_key_frames_device(torch.from_numpy(np.ascontiguousarray(f, dtype=np.float32)).cuda(), thr).cpu().tolist()


def _feed(sel, f, part, want=None):
    """Feed f under the partition; with `want` (the one-shot list of all of f) check the prefix rule after every batch."""
    for a, b in part:
        sel.extend(f[a:b])
        assert sel.n_seen == b
        if want is not None:
            got = sel.kept()
            assert got.dtype == np.int64
            assert got.tolist() == K.expected_after(want, b), (a, b)
    return sel.kept().tolist()


@pytest.mark.parametrize("name", recipes.SELECT_CASES)
def test_golden_vectors_under_partitions(name):
    f, _ = recipes.select_case(name)
    assert recipes.sha256(f) == K.SHA[name]
    dev = torch.from_numpy(f).cuda()
    for label, part in K.partitions(name, f.shape[0]).items():
        assert _feed(_selector(), dev, part, K.GOLD[name]) == K.GOLD[name], label


@pytest.mark.parametrize("name", recipes.SELECT_INBAND_CASES)
def test_inband_fixtures_under_every_two_batch_split(name):
    f, _ = recipes.select_case(name)
    assert recipes.sha256(f) == K.SHA[name]
    dev, n = torch.from_numpy(f).cuda(), f.shape[0]
    for s in range(1, n):
        assert _feed(_selector(), dev, [(0, s), (s, n)], K.GOLD[name]) == K.GOLD[name], s


def test_random_inband_pairs_split_by_batch_boundaries():
    """The construction of test_gpu_select.py::test_inband_property_random_pairs: partners within +- 2e-7 of the threshold.
    Batches of 33: a pair (2j, 2j+1) lies in one batch (new x new decides it) or across a boundary (new x kept does)."""
    rng = np.random.default_rng(4242)
    n = 400
    f = rng.standard_normal((n, 1024)).astype(np.float32)
    thr = float(np.float32(0.9))
    for j in range(n // 2):
        u = f[2 * j].astype(np.float64)
        u /= np.linalg.norm(u)
        r = rng.standard_normal(1024)
        r -= r.dot(u) * u
        r /= np.linalg.norm(r)
        c = thr + rng.uniform(-2e-7, 2e-7)
        f[2 * j + 1] = ((c * u + np.sqrt(1 - c * c) * r) * rng.uniform(0.5, 3.0)).astype(np.float32)
    want = select_key_frames_exact(f).tolist()
    assert 0 < len(want) - n // 2 < n // 2, "both outcomes (kept / dropped partner) must occur"
    part = K.batches(n, [33])
    assert any(a % 2 == 1 for a, _ in part) and any(a % 2 == 0 for a, _ in part[1:])
    assert _feed(_selector(), f, part, want) == want
    assert _one_shot(f) == want


@pytest.mark.parametrize("n,clusters,sigma,thr", [(777, 90, 0.3, 0.9), (500, 60, 0.2, 0.5), (500, 60, 0.2, 0.97)])
def test_clustered_inputs_under_random_partitions(n, clusters, sigma, thr):
    f = recipes.clustered(n, clusters, sigma, seed=n + clusters)
    dev = torch.from_numpy(f).cuda()
    want = _one_shot(f, thr)
    assert 1 < len(want) <= n                               # (at 0.97 every row of this input is kept: no pair reaches it)
    for seed in range(3):
        sizes = np.random.default_rng(1000 * seed + n).integers(1, 131, size=n).tolist()
        assert _feed(_selector(similarity_threshold=thr), dev, K.batches(n, sizes), want) == want, seed


def test_kept_count_crosses_tile_edges():
    """130 unrelated rows are all kept (the kept rows fill two tiles and two rows of a third); copies of the rows on either side
    of each tile edge, fed one per batch, are dropped whichever tile holds their original; a fresh row is kept."""
    rng = np.random.default_rng(77)
    base = rng.standard_normal((130, 1024)).astype(np.float32)
    edge = [0, 63, 64, 127, 128, 129]
    copies = np.concatenate([base[edge], base[edge] * np.float32(2.5)])
    fresh = rng.standard_normal((1, 1024)).astype(np.float32)
    f = np.concatenate([base, copies, fresh])
    want = _one_shot(f)
    assert want == list(range(130)) + [142]
    sel = _selector()
    _feed(sel, f[:130], K.batches(130, K.CYCLE), want)
    for i in range(130, 142):
        sel.extend(f[i])                                     # a single (1024,) row
        assert sel.kept().tolist() == list(range(130)), i
    sel.extend(f[142:])
    assert sel.n_seen == 143 and sel.kept().tolist() == want


def test_nan_rows():
    f, _ = recipes.select_case("n12_zero_row")
    assert _feed(_selector(), f, [(0, 6), (6, 7), (7, 12)], K.GOLD["n12_zero_row"]) == K.GOLD["n12_zero_row"] == _one_shot(f)
    g = f.copy()
    g[0] = 0.0                                               # global row 0 is kept whatever it holds, and then blocks every row
    want = _one_shot(g)
    assert want == [0]
    for part in (K.batches(12, [1]), K.batches(12, [12]), [(0, 1), (1, 12)], [(0, 5), (5, 12)]):
        assert _feed(_selector(), g, part, want) == [0]


def test_capacity_grows_by_copying_the_live_rows():
    f, _ = recipes.select_case("n257_clusters40")
    sel = _selector(capacity=4)
    assert _feed(sel, f, K.batches(257, [7]), K.GOLD["n257_clusters40"]) == K.GOLD["n257_clusters40"]
    assert sel.capacity >= len(K.GOLD["n257_clusters40"]) > 4
    lazy = _selector(capacity=4)                             # no read-out in between: the class reads the count itself to grow
    for a, b in K.batches(257, [7]):
        lazy.extend(f[a:b])
    assert lazy.kept().tolist() == K.GOLD["n257_clusters40"]
    assert torch.equal(lazy.kept_device().cpu(), torch.tensor(K.GOLD["n257_clusters40"]))


def test_selectors_are_isolated_and_follow_the_current_stream():
    fa, _ = recipes.select_case("n257_clusters40")
    fb, _ = recipes.select_case("n64_revisit")
    da, db = torch.from_numpy(fa).cuda(), torch.from_numpy(fb).cuda()
    a, b = _selector(), _selector()
    pa, pb = K.batches(257, [33]), K.batches(64, [9])
    for i in range(max(len(pa), len(pb))):                   # in alternation on one stream, nothing read in between
        if i < len(pa):
            a.extend(da[pa[i][0]: pa[i][1]])
        if i < len(pb):
            b.extend(db[pb[i][0]: pb[i][1]])
    assert a.kept().tolist() == K.GOLD["n257_clusters40"] and b.kept().tolist() == K.GOLD["n64_revisit"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _selector()
        for s, e in pa:
            c.extend(da[s:e])
        got = c.kept().tolist()
    assert got == K.GOLD["n257_clusters40"]


def test_reset_and_input_kinds():
    f, _ = recipes.select_case("n257_clusters40")
    want, part = K.GOLD["n257_clusters40"], K.batches(257, K.CYCLE)
    sel = _selector()
    assert sel.kept().tolist() == [] and sel.n_seen == 0
    assert _feed(sel, torch.from_numpy(f).cuda(), part) == want
    sel.reset()
    assert sel.n_seen == 0 and sel.kept().tolist() == []
    assert _feed(sel, f, part) == want                                       # numpy float32, the same buffers
    assert _feed(_selector(), f.astype(np.float64), part) == want            # numpy float64
    assert _feed(_selector(), torch.from_numpy(f), part) == want             # a host tensor
    dev = sel.kept_device()
    assert dev.is_cuda and dev.dtype == torch.int64 and dev.cpu().tolist() == want
