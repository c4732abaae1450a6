"""CPU: the C ABI of the frame-extraction walk (hmm_extract_walk, hmm_extract_walk_workspace_bytes, hmm_extract_carry) -- declared,
exported and bound with matching signatures, the public struct layouts mirrored by the Python layer, the ABI version unchanged,
and every argument error reported as a status code with the function's name on a host without a GPU (nothing is dereferenced on
the device or launched before the checks)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = {"hmm_extract_walk_workspace_bytes": 2, "hmm_extract_walk": 16, "hmm_extract_carry": 6}
HMM_E_INVALID, HMM_E_WORKSPACE = -1, -2
FAR = 1 << 40                                                    # non-null, aligned device dummies far from each other
GRAY, STATE, REC, WS = FAR, 2 * FAR, 3 * FAR, 4 * FAR
BIG = 1 << 62


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)


def test_symbols_are_declared_exported_and_bound_with_matching_signatures():
    from hippomm_amd import _lib, build
    text = _header()
    raw = ctypes.CDLL(str(build.build()))
    for name, n_args in NEW.items():
        m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == n_args, (name, params)
        assert hasattr(raw, name), name
        res, args = _lib._SIGNATURES[name]
        assert len(args) == n_args, name
        for p, a in zip(params, args):                           # pointers as addresses, scalars by their C type
            want = ctypes.c_void_p if "*" in p or p.startswith("hmm_stream_t") else \
                {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t}[p.split()[0]]
            assert a is want, (name, p, a)
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
    assert _lib.load().hmm_abi_version() == 7


def test_struct_layouts_are_the_python_layers():
    from hippomm_amd import frame_extraction as seg
    text = _header()
    for struct, dtype in (("hmm_extract_state", seg.EXTRACT_STATE), ("hmm_extract_record", seg.EXTRACT_RECORD)):
        body = re.search(rf"typedef struct \{{([^}}]*)\}}\s*{struct};", text).group(1)
        fields = [(t, n) for t, n in re.findall(r"\b(int32_t|double)\s+(\w+);", body)]
        assert [n for _, n in fields] == list(dtype.names), struct
        assert [dtype[n] for _, n in fields] == [np.dtype("<i4") if t == "int32_t" else np.dtype("<f8") for t, _ in fields]
    assert seg.EXTRACT_STATE.itemsize == 24 and seg.EXTRACT_RECORD.itemsize == 40          # no padding: what a C compiler lays out


def test_walk_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    times = (ctypes.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    flags = (ctypes.c_int32 * 4)(1, 1, 1, 1)
    none = (ctypes.c_int32 * 4)()
    T, C, D = (ctypes.addressof(x) for x in (times, flags, none))

    def refused(*args, say, code=HMM_E_INVALID):
        assert lib.hmm_extract_walk(*args) == code, args
        msg = lib.hmm_last_error()
        assert b"extract_walk" in msg and say in msg, msg

    #       gray, n_slots, H, W, first_slot, count, times, check, deny, threshold, min_gap, state, records, workspace, bytes, stream
    good = [GRAY, 5, 48, 64, 1, 4, T, C, D, 0.3, 1.0, STATE, REC, WS, BIG, None]
    for at in (0, 6, 7, 8, 11, 12, 13):
        refused(*[None if i == at else v for i, v in enumerate(good)], say=b"null pointer")
    for h, w in ((6, 64), (48, 6), (0, 0), (-3, 64)):
        refused(*[{2: h, 3: w}.get(i, v) for i, v in enumerate(good)], say=b"win_size exceeds image extent")
    for first, count, n_slots in ((0, 4, 5), (-1, 1, 5), (2, 4, 5), (1, 5, 5), (5, 1, 5), (1, 2 ** 31 - 1, 5)):
        refused(*[{1: n_slots, 4: first, 5: count}.get(i, v) for i, v in enumerate(good)], say=b"outside slots")
    refused(*[{5: 0}.get(i, v) for i, v in enumerate(good)], say=b"count")
    refused(*[{1: 1, 5: 1}.get(i, v) for i, v in enumerate(good)], say=b"n_slots")
    for at in (11, 12, 13):
        refused(*[v + 4 if i == at else v for i, v in enumerate(good)], say=b"8-byte aligned")
    for bad in (float("nan"), float("inf"), float("-inf")):
        worse = (ctypes.c_double * 4)(0.0, 1.0, bad, 3.0)
        refused(*[ctypes.addressof(worse) if i == 6 else v for i, v in enumerate(good)], say=b"not finite")
    refused(*[float("nan") if i == 9 else v for i, v in enumerate(good)], say=b"NaN")
    refused(*[float("nan") if i == 10 else v for i, v in enumerate(good)], say=b"NaN")
    for h, w in ((48, 64), (43, 263), (7, 7), (1080, 1920)):
        need = lib.hmm_extract_walk_workspace_bytes(h, w)
        assert need >= 8 * ((w - 6 + 255) // 256) * ((h - 6 + 35) // 36) and need % 256 == 0
        refused(*[{2: h, 3: w, 14: need - 1}.get(i, v) for i, v in enumerate(good)], say=b"workspace", code=HMM_E_WORKSPACE)
    assert lib.hmm_extract_walk_workspace_bytes(6, 64) == 0 and lib.hmm_extract_walk_workspace_bytes(48, 6) == 0
    assert lib.hmm_extract_walk_workspace_bytes(48, 64) == lib.hmm_ssim_pairs_workspace_bytes(48, 64, 1)


def test_carry_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    for args, say in (((None, 5, 48, 64, STATE, None), b"null pointer"), ((GRAY, 5, 48, 64, None, None), b"null pointer"),
                      ((GRAY, 0, 48, 64, STATE, None), b"bad shape"), ((GRAY, 5, 0, 64, STATE, None), b"bad shape"),
                      ((GRAY, 5, 48, 64, STATE + 4, None), b"8-byte aligned")):
        assert lib.hmm_extract_carry(*args) == HMM_E_INVALID
        msg = lib.hmm_last_error()
        assert b"extract_carry" in msg and say in msg, msg


def test_extractor_has_no_cpu_fallback(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from hippomm_amd import _lib, extract_frames, extraction_records
    frames = np.zeros((2, 48, 64, 3), np.uint8)
    with pytest.raises(_lib.HippoMMHipError, match="no CPU fallback"):
        extraction_records(frames, [0, 30], 30.0)
    with pytest.raises(_lib.HippoMMHipError, match="no CPU fallback"):
        extract_frames(list(frames), 30.0, tmp_path)
