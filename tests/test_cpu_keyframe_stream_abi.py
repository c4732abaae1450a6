"""CPU: the C ABI of the growing key-frame selection (hmm_keyframe_extend, hmm_keyframe_extend_workspace_bytes) -- declared,
exported and bound, the ABI version unchanged, every argument error reported as a status code with the function's name on a host
without a GPU (nothing is dereferenced or launched before the checks), m == 0 answered with HMM_OK, and no CPU fallback."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ["hmm_keyframe_extend_workspace_bytes", "hmm_keyframe_extend"]
HMM_OK, HMM_E_INVALID, HMM_E_WORKSPACE = 0, -1, -2
ONE = 1 << 20                                                    # a 16-byte aligned non-null dummy
FAR = 1 << 40                                                    # others, far from it and from each other
ROWS, IDX, CNT, WS = FAR, 2 * FAR, 3 * FAR, 4 * FAR
BIG = 1 << 62                                                    # "enough workspace"
TOP = 2 ** 63 - 1


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


def test_status_codes_are_the_headers():
    text = (ROOT / "include" / "hippomm_hip.h").read_text()
    for name, value in (("HMM_OK", HMM_OK), ("HMM_E_INVALID", HMM_E_INVALID), ("HMM_E_WORKSPACE", HMM_E_WORKSPACE)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call, name = lib.hmm_keyframe_extend, b"keyframe_extend"

    def refused(*args, say, code=HMM_E_INVALID):
        assert call(*args) == code, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg

    #      new, m, dim, thr, kept_rows, kept_idx, capacity, n_kept, n_seen_before, kept_bound, workspace, workspace_bytes, stream
    refused(ONE, 5, 512, 0.9, ROWS, IDX, 100, CNT, 10, 10, WS, BIG, None, say=b"dim must be 1024")
    refused(ONE, -5, 1024, 0.9, ROWS, IDX, 100, CNT, 10, 10, WS, BIG, None, say=b"negative")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, -100, CNT, 10, 10, WS, BIG, None, say=b"negative")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, 100, CNT, -10, 10, WS, BIG, None, say=b"negative")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 10, -1, WS, BIG, None, say=b"negative")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 10, 11, WS, BIG, None, say=b"rows seen")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 0, 1, WS, BIG, None, say=b"rows seen")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 200, 96, WS, BIG, None, say=b"exceed the capacity")
    refused(ONE, 101, 1024, 0.9, ROWS, IDX, 100, CNT, 0, 0, WS, BIG, None, say=b"exceed the capacity")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, TOP - 8, CNT, TOP - 8, TOP - 8, WS, BIG, None, say=b"exceed the capacity")   # no overflow
    refused(ONE, 1, 1024, 0.9, ROWS, IDX, TOP - 1, CNT, TOP - 1, TOP - 1, WS, BIG, None, say=b"exceed the capacity")   # in the sum
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, TOP, CNT, TOP, 0, WS, BIG, None, say=b"out of range")                        # nor in n_seen + m
    for missing in range(5):                                     # new rows, kept rows, kept indices, count, workspace
        p = [None if i == missing else v for i, v in enumerate((ONE, ROWS, IDX, CNT, WS))]
        refused(p[0], 5, 1024, 0.9, p[1], p[2], 100, p[3], 10, 10, p[4], BIG, None, say=b"null pointer")
    for bad in range(3):                                         # the row pointers and the workspace
        p = [v + 8 if i == bad else v for i, v in enumerate((ONE, ROWS, WS))]
        refused(p[0], 5, 1024, 0.9, p[1], IDX, 100, CNT, 10, 10, p[2], BIG, None, say=b"16-byte aligned")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX + 4, 100, CNT, 10, 10, WS, BIG, None, say=b"8-byte aligned")
    refused(ONE, 5, 1024, 0.9, ROWS, IDX, 100, CNT + 4, 10, 10, WS, BIG, None, say=b"8-byte aligned")
    # overlap, by plain pointer arithmetic on the bytes read (5 rows) and the state's whole extent (100 rows, 100 indices, 1 count)
    refused(ROWS, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 10, 10, WS, BIG, None, say=b"overlap")
    refused(ROWS + 100 * 4096 - 16, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 10, 10, WS, BIG, None, say=b"overlap")     # its last 16 bytes
    refused(ROWS - 5 * 4096 + 16, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 10, 10, WS, BIG, None, say=b"overlap")      # its first 16
    refused(IDX + 100 * 8 - 16, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 10, 10, WS, BIG, None, say=b"overlap")
    refused(CNT - 5 * 4096 + 16, 5, 1024, 0.9, ROWS, IDX, 100, CNT, 10, 10, WS, BIG, None, say=b"overlap")
    # an m whose bitmap exceeds LDS: hmm_gram_select's refusal (64 KiB of bits = 524288 rows)
    refused(ONE, 524289, 1024, 0.9, ROWS, IDX, 1 << 30, CNT, 0, 0, WS, BIG, None, say=b"too large for the LDS bitmap")
    # one byte short of the query
    for m in (1, 64, 65):
        need = lib.hmm_keyframe_extend_workspace_bytes(m)
        refused(ONE, m, 1024, 0.9, ROWS, IDX, 100, CNT, 10, 10, WS, need - 1, None, say=b"workspace", code=HMM_E_WORKSPACE)


def test_zero_rows_return_ok_without_a_launch():
    """No GPU on this host: a launch would fail, HMM_OK means none was tried -- and no pointer is looked at."""
    lib = _lib()
    assert lib.hmm_keyframe_extend(None, 0, 1024, 0.9, None, None, 0, None, 0, 0, None, 0, None) == HMM_OK
    assert lib.hmm_keyframe_extend(ONE, 0, 1024, 0.9, ROWS, IDX, 100, CNT, 50, 50, WS, 0, None) == HMM_OK
    assert lib.hmm_keyframe_extend(ONE + 4, 0, 1024, 0.9, ROWS, IDX, 100, CNT, 100, 100, None, 0, None) == HMM_OK


def test_workspace_query_is_positive_and_monotone():
    lib = _lib()
    sizes = [lib.hmm_keyframe_extend_workspace_bytes(m) for m in range(0, 400)] + \
            [lib.hmm_keyframe_extend_workspace_bytes(m) for m in (1000, 3600, 3632, 100000)]
    assert lib.hmm_keyframe_extend_workspace_bytes(1) > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] >= 64 * 4096                                 # at least the normalised rows of one tile


def test_selector_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from hippomm_amd import _lib
    from hippomm_amd.consolidation import KeyFrameSelector
    sel = KeyFrameSelector()
    with pytest.raises(_lib.HippoMMHipError, match="no CPU fallback"):
        sel.extend(np.ones((3, 1024), dtype=np.float32))
    with pytest.raises(_lib.HippoMMHipError, match="no CPU fallback"):
        sel.extend(torch.ones(1024))
    assert sel.n_seen == 0 and sel.kept().tolist() == []
