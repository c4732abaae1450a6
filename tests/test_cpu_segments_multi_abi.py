"""CPU: the C ABI of the batched per-event scan (hmm_cosine_topk_segmented_multi, its workspace query and
hmm_rank_segment_hits_multi) -- declared, exported and bound, a workspace query that does not grow with the number of questions,
and argument errors that are reported on a host without a GPU."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW = ["hmm_cosine_topk_segmented_multi", "hmm_cosine_topk_segmented_multi_workspace_bytes", "hmm_rank_segment_hits_multi"]
HMM_E_INVALID, HMM_E_WORKSPACE = -1, -2


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(build.build()))
    for name in NEW:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _lib._SIGNATURES, name
    assert _lib.load().hmm_abi_version() == 7


def test_workspace_query():
    q = _lib().hmm_cosine_topk_segmented_multi_workspace_bytes
    for args in [(0, 5, 3, 5), (-1, 5, 3, 5), (100, 0, 3, 5), (100, -2, 3, 5), (100, 5, 0, 5), (100, 5, -1, 5), (100, 5, 3, 0),
                 (100, 5, 3, -7)]:
        assert q(*args) == 0, args
    # one pass of 16 questions x 4 bytes per row at the least; bounded by what 16 questions need
    assert q(1_000_000, 2000, 16, 5) >= 16 * 4 * 1_000_000
    assert q(1_000_000, 2000, 16, 5) < 17 * 4 * 1_000_000
    for n, e, k in [(1, 1, 1), (1000, 7, 5), (1_000_000, 2000, 5), (4097, 3, 64), (4097, 3, 65), (20000, 9, 1024)]:
        assert q(n, e, 16, k) == q(n, e, 1000, k), (n, e, k)
    rows = [1, 2, 15, 16, 17, 63, 64, 65, 1000, 4096, 4097, 100_000, 1_000_000, 10_000_000]
    for a, b in zip(rows, rows[1:]):
        for k in (1, 5, 64, 65, 1024):
            assert q(a, 10, 3, k) <= q(b, 10, 3, k), (a, b, k)
    for n in (1, 500, 4097, 1_000_000):
        segs = [q(n, e, 3, 5) for e in (1, 2, 100, 2000, 100_000)]
        ks = [q(n, 10, 3, k) for k in (1, 5, 63, 64, 65, 128, 1024)]
        nqs = [q(n, 10, nq, 5) for nq in (1, 2, 15, 16, 17, 33, 1000)]
        assert segs == sorted(segs) and ks == sorted(ks) and nqs == sorted(nqs), n
    # the one-question scans behind k > 64 run in the same workspace
    seg = _lib().hmm_cosine_topk_segmented_workspace_bytes
    for n in (1, 500, 4097, 1_000_000):
        assert q(n, 10, 3, 100) >= seg(n, 10, 100)


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    one = 4096                                                   # a 16-byte aligned non-null dummy: nothing is dereferenced before the checks
    need = lib.hmm_cosine_topk_segmented_multi_workspace_bytes(100, 4, 3, 5)
    call = lib.hmm_cosine_topk_segmented_multi

    def err():
        return lib.hmm_last_error()

    assert call(one, 100, 512, one, 3, one, 4, 5, one, one, one, one, need, None) == HMM_E_INVALID
    assert b"cosine_topk_segmented_multi" in err() and b"dim must be 1024" in err()
    assert call(one, 100, 1024, one, 3, one, 4, 5, None, None, None, one, need, None) == HMM_E_INVALID
    assert b"cosine_topk_segmented_multi" in err() and b"null pointer" in err()
    assert call(one, 0, 1024, one, 3, one, 4, 5, one, one, one, one, need, None) == HMM_E_INVALID
    assert b"cosine_topk_segmented_multi" in err() and b"n_rows" in err()
    assert call(one, 0xFFFFFFFF, 1024, one, 3, one, 4, 5, one, one, one, one, 1 << 40, None) == HMM_E_INVALID
    assert b"n_rows" in err()
    assert call(one, 100, 1024, one, 0, one, 4, 5, one, one, one, one, need, None) == HMM_E_INVALID
    assert call(one, 100, 1024, one, 3, one, 4, 1025, one, one, one, one, need, None) == HMM_E_INVALID
    assert b"cosine_topk_segmented_multi" in err()
    assert call(one + 4, 100, 1024, one, 3, one, 4, 5, one, one, one, one, need, None) == HMM_E_INVALID
    assert b"16-byte aligned" in err()
    assert call(one, 100, 1024, one, 3, one, 4, 5, one, one, one, one + 8, need, None) == HMM_E_INVALID
    assert b"16-byte aligned" in err()
    assert call(one, 100, 1024, one, 3, one, 4, 5, one, one, one, one, need - 1, None) == HMM_E_WORKSPACE
    assert f"cosine_topk_segmented_multi: workspace {need - 1} < required {need}".encode() in err()
    assert call(one, 100, 1024, one, 3, one, 4, 100, one, one, one, one, need - 1, None) == HMM_E_WORKSPACE   # k > 64 too

    rank = lib.hmm_rank_segment_hits_multi
    assert rank(one, one, one, 3, 4, 5, 65, one, one, one, one, None) == HMM_E_INVALID
    assert b"rank_segment_hits_multi" in err() and b"keep" in err()
    assert rank(one, one, one, 3, 4, 5, 5, None, None, None, None, None) == HMM_E_INVALID
    assert b"rank_segment_hits_multi" in err() and b"null pointer" in err()
    assert rank(one, one, one, 0, 4, 5, 5, one, one, one, one, None) == HMM_E_INVALID
    assert b"rank_segment_hits_multi" in err()
