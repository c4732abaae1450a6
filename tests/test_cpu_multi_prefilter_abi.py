"""CPU: the C ABI of the batched scans through the bf16 shadow (hmm_cosine_topk_multi_prefilter,
hmm_cosine_topk_segmented_multi_prefilter and their workspace queries) -- declared, exported and bound, workspace queries that are
monotone and hold the exact function's workspace (the fallback runs inside it), and argument errors that are reported as status
codes on a host without a GPU."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW = ["hmm_cosine_topk_multi_prefilter", "hmm_cosine_topk_multi_prefilter_workspace_bytes",
       "hmm_cosine_topk_segmented_multi_prefilter", "hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes"]
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


def test_workspace_queries():
    lib = _lib()
    flat, seg = lib.hmm_cosine_topk_multi_prefilter_workspace_bytes, lib.hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes
    for args in [(0, 3, 5), (-1, 3, 5), (100, 0, 5), (100, -1, 5), (100, 3, 0), (100, 3, -7)]:
        assert flat(*args) == 0, args
    for args in [(0, 5, 3, 5), (-1, 5, 3, 5), (100, 0, 3, 5), (100, -2, 3, 5), (100, 5, 0, 5), (100, 5, -1, 5), (100, 5, 3, 0),
                 (100, 5, 3, -7)]:
        assert seg(*args) == 0, args
    rows = [1, 2, 15, 16, 17, 63, 64, 65, 1000, 4096, 4097, 16383, 16384, 16385, 100_000, 1_000_000, 10_000_000]
    ks = (1, 5, 32, 63, 64, 65, 128, 1024)
    for a, b in zip(rows, rows[1:]):
        for k in ks:
            assert flat(a, 3, k) <= flat(b, 3, k), (a, b, k)
            assert seg(a, 10, 3, k) <= seg(b, 10, 3, k), (a, b, k)
    for n in (1, 500, 4097, 20000, 1_000_000):
        by_k = [flat(n, 3, k) for k in ks]
        assert by_k == sorted(by_k), n
        by_k = [seg(n, 10, 3, k) for k in ks]
        by_e = [seg(n, e, 3, 5) for e in (1, 2, 100, 2000, 100_000)]
        assert by_k == sorted(by_k) and by_e == sorted(by_e), n
    # the fallback (and the call below the dispatch limits) runs inside the exact function's workspace
    for n in (1, 500, 4097, 16384, 20000, 1_000_000):
        for nq in (1, 16, 17, 33):
            for k in ks:
                assert flat(n, nq, k) >= lib.hmm_cosine_topk_multi_workspace_bytes(n, nq, k), (n, nq, k)
                assert seg(n, 10, nq, k) >= lib.hmm_cosine_topk_segmented_multi_workspace_bytes(n, 10, nq, k), (n, nq, k)


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    one = 4096                                                   # a 16-byte aligned non-null dummy: nothing is dereferenced before the checks

    def err():
        return lib.hmm_last_error()

    need = lib.hmm_cosine_topk_multi_prefilter_workspace_bytes(20000, 3, 5)
    call = lib.hmm_cosine_topk_multi_prefilter
    name = b"cosine_topk_multi_prefilter"
    assert call(one, one, 20000, 512, one, 3, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"dim must be 1024" in err()
    assert call(one, None, 20000, 1024, one, 3, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"null pointer" in err()
    assert call(one, one, 20000, 1024, one, 3, 5, None, None, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"null pointer" in err()
    assert call(one, one, 0, 1024, one, 3, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"n_rows" in err()
    assert call(one, one, 20000, 1024, one, 0, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"n_queries=0" in err()
    for bad in range(4):                                         # store, shadow, queries, workspace
        ptrs = [one + 4 if i == bad else one for i in range(4)]
        assert call(ptrs[0], ptrs[1], 20000, 1024, ptrs[2], 3, 5, one, one, one, None, ptrs[3], need, None) == HMM_E_INVALID
        assert name in err() and b"16-byte aligned" in err()
    assert call(one, one, 20000, 1024, one, 3, 5, one, one, one, None, one, need - 1, None) == HMM_E_WORKSPACE
    assert f"cosine_topk_multi_prefilter: workspace {need - 1} < required {need}".encode() in err()
    small = lib.hmm_cosine_topk_multi_prefilter_workspace_bytes(100, 3, 5)                 # below the dispatch limit, and k > 64, too
    assert call(one, one, 100, 1024, one, 3, 5, one, one, one, None, one, small - 1, None) == HMM_E_WORKSPACE
    big_k = lib.hmm_cosine_topk_multi_prefilter_workspace_bytes(20000, 3, 100)
    assert call(one, one, 20000, 1024, one, 3, 100, one, one, one, None, one, big_k - 1, None) == HMM_E_WORKSPACE

    need = lib.hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes(2000, 4, 3, 5)
    call = lib.hmm_cosine_topk_segmented_multi_prefilter
    name = b"cosine_topk_segmented_multi_prefilter"
    assert call(one, one, 2000, 512, one, 3, one, 4, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"dim must be 1024" in err()
    assert call(one, None, 2000, 1024, one, 3, one, 4, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"null pointer" in err()
    assert call(one, one, 2000, 1024, one, 3, None, 4, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"null pointer" in err()
    assert call(one, one, 0, 1024, one, 3, one, 4, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"n_rows" in err()
    assert call(one, one, 2000, 1024, one, 0, one, 4, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err() and b"n_queries >= 1" in err()
    assert call(one, one, 2000, 1024, one, 3, one, 0, 5, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert call(one, one, 2000, 1024, one, 3, one, 4, 1025, one, one, one, None, one, need, None) == HMM_E_INVALID
    assert name in err()
    for bad in range(4):
        ptrs = [one + 8 if i == bad else one for i in range(4)]
        assert call(ptrs[0], ptrs[1], 2000, 1024, ptrs[2], 3, one, 4, 5, one, one, one, None, ptrs[3], need, None) == HMM_E_INVALID
        assert name in err() and b"16-byte aligned" in err()
    assert call(one, one, 2000, 1024, one, 3, one, 4, 5, one, one, one, None, one, need - 1, None) == HMM_E_WORKSPACE
    assert f"cosine_topk_segmented_multi_prefilter: workspace {need - 1} < required {need}".encode() in err()
    assert call(one, one, 2000, 1024, one, 3, one, 4, 100, one, one, one, None, one, need - 1, None) == HMM_E_WORKSPACE   # k > 64 too
    assert call(one, one, 100, 1024, one, 3, one, 4, 5, one, one, one, None, one,
                lib.hmm_cosine_topk_segmented_multi_prefilter_workspace_bytes(100, 4, 3, 5) - 1, None) == HMM_E_WORKSPACE   # small events too
