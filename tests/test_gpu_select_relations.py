"""GPU: key-frame selection on inputs whose similarity relation is planted (select_relation_cases.py) -- hits between far tiles,
in bitmap columns beyond word 64, non-transitive triples and paths, a (kept tiles x new tiles) grid with a hit in every cell,
threshold and NaN-row edges.  hmm_gram_select and hmm_keyframe_extend must list exactly the closed-form kept rows (the margins
of test_cpu_select_relations.py rule rounding out), and the adjacency words hmm_gram_select leaves in its workspace must be the
modelled relation bit for bit: symmetric, diagonal included, nothing in a padding row or column."""
import ctypes as C

import numpy as np
import pytest
import torch

import keyframe_stream_cases as K
import select_relation_cases as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", R.CASES)
def test_one_shot_lists_the_planted_expectation(name):
    from hippomm_amd.consolidation import select_key_frames, select_key_frames_device
    f, thr, _, want = R.case(name)
    first = select_key_frames(f, None, thr)
    assert first.dtype == np.int64 and first.tolist() == want
    dev = torch.from_numpy(f).cuda()
    assert select_key_frames_device(dev, thr).cpu().tolist() == want
    assert select_key_frames(f, None, thr).tolist() == want                 # the same bytes again
    assert torch.equal(dev.cpu(), torch.from_numpy(f))


@pytest.mark.parametrize("name", R.CASES)
def test_grown_selection_lists_the_planted_prefix_after_every_batch(name):
    from hippomm_amd.consolidation import KeyFrameSelector
    f, thr, _, want = R.case(name)
    dev = torch.from_numpy(f).cuda()
    for label, part in R.partitions(name, f.shape[0]).items():
        sel = KeyFrameSelector(similarity_threshold=thr)
        for a, b in part:
            sel.extend(dev[a:b])
            assert sel.n_seen == b
            assert sel.kept().tolist() == K.expected_after(want, b), (label, a, b)
        assert sel.kept().tolist() == want, label


def _adjacency(f, thr):
    """hmm_gram_select through the C ABI on a workspace the test owns -> (kept list, adjacency bool (n_pad, n_pad)).  Layout
    (header of gram_select.hip): Fn (n_pad,1024) fp32, then, 256-byte aligned, n_pad x n_pad/32 uint32 words, bit b of word w
    of row r = column 32 w + b."""
    from hippomm_amd import _lib
    _lib.require_gpu()
    lib = _lib.load()
    n = f.shape[0]
    n_pad = (n + R.TILE - 1) // R.TILE * R.TILE
    words = n_pad // 32
    off_adj = (n_pad * 1024 * 4 + 255) // 256 * 256
    need = lib.hmm_gram_select_workspace_bytes(n)
    assert need >= off_adj + n_pad * words * 4
    dev = torch.from_numpy(f).cuda()
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")        # a word no block writes would show as this pattern
    kept = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    n_kept = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.hmm_gram_select(dev.data_ptr(), n, 1024, C.c_float(thr), kept.data_ptr(), n_kept.data_ptr(), ws.data_ptr(),
                                   need, _lib.stream_ptr()), "hmm_gram_select")
    torch.cuda.synchronize()
    raw = ws[off_adj: off_adj + n_pad * words * 4].cpu().numpy()
    bits = np.unpackbits(raw.reshape(n_pad, words * 4), axis=1, bitorder="little").astype(bool)     # little-endian words
    return kept[: int(n_kept.item())].cpu().tolist(), bits


@pytest.mark.parametrize("name", R.CASES)
def test_adjacency_words_are_the_modelled_relation(name):
    f, thr, planted, want = R.case(name)
    _, rel = R.case_model(name)
    n = f.shape[0]
    kept, bits = _adjacency(f, float(np.float32(thr)))
    assert kept == want
    assert bits.shape[0] == bits.shape[1] and bits.shape[0] % R.TILE == 0 and 0 <= bits.shape[0] - n < R.TILE
    wrong = np.argwhere(bits[:n, :n] != rel)
    assert wrong.size == 0, f"{len(wrong)} bits differ from the model, first (row, col) {wrong[:8].tolist()}"
    assert np.array_equal(rel, planted)
    assert np.array_equal(bits, bits.T)                                      # the mirror writes
    assert not bits[n:, :].any() and not bits[:, n:].any()                   # padding rows and columns are masked
