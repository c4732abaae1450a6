"""CPU: the C ABI of the segmentation walk (hmm_segment_walk, hmm_segment_walk_workspace_bytes) -- declared, exported and bound with
matching signatures, the public struct layouts and status codes mirrored by the Python layer, the ABI version unchanged, and every
argument error reported as a status code with the function's name on a host without a GPU (nothing is dereferenced on the device
or launched before the checks)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = {"hmm_segment_walk_workspace_bytes": 2, "hmm_segment_walk": 22}
HMM_E_INVALID, HMM_E_WORKSPACE = -1, -2
FAR = 1 << 40                                                    # non-null, aligned device dummies far from each other
SCORES, FLAGS, TIMES, TRACK, REC, STATE, WS = (k * FAR for k in range(1, 8))
BIG = 1 << 62
C_TYPES = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64}


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def _header(comments: bool = False):
    text = (ROOT / "include" / "hippomm_hip.h").read_text()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


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
            want = ctypes.c_void_p if "*" in p or p.startswith("hmm_stream_t") else C_TYPES[p.split()[0]]
            assert a is want, (name, p, a)
        assert res is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
    assert _lib.load().hmm_abi_version() == 7


def test_struct_layouts_and_status_codes_are_the_python_layers():
    from hippomm_amd import segmentation as seg
    text = _header()
    for struct, dtype in (("hmm_segment_record", seg.SEGMENT_RECORD), ("hmm_segment_walk_state", seg.SEGMENT_STATE)):
        body = re.search(rf"typedef struct \{{([^}}]*)\}}\s*{struct};", text).group(1)
        fields = [(t, n) for t, n in re.findall(r"\b(int32_t|double)\s+(\w+);", body)]
        assert [n for _, n in fields] == list(dtype.names), struct
        assert [dtype[n] for _, n in fields] == [np.dtype("<i4") if t == "int32_t" else np.dtype("<f8") for t, _ in fields]
    assert seg.SEGMENT_RECORD.itemsize == 40 and seg.SEGMENT_STATE.itemsize == 24          # no padding: what a C compiler lays out
    codes = dict(re.findall(r"#define\s+HMM_SEGMENT_WALK_(\w+)\s+(\d+)", text))
    assert codes == {"RUNNING": "0", "DONE": str(seg.WALK_DONE), "FLAGGED": str(seg.WALK_FLAGGED), "BOUND": str(seg.WALK_BOUND)}


def test_walk_refuses_bad_arguments_without_a_gpu():
    lib = _lib()
    times = (ctypes.c_double * 4)(0.0, 1.0, 1.0, 3.0)
    T = ctypes.addressof(times)

    def refused(*args, say, code=HMM_E_INVALID):
        assert lib.hmm_segment_walk(*args) == code, args
        msg = lib.hmm_last_error()
        assert b"segment_walk" in msg and say in msg, msg

    need = lib.hmm_segment_walk_workspace_bytes(20, 8)
    assert need >= 20 * 16 + 20 * 8 and need % 256 == 0
    assert lib.hmm_segment_walk_workspace_bytes(0, 8) == 0 and lib.hmm_segment_walk_workspace_bytes(20, 0) == 0
    #       0 scores, 1 flags, 2 times_dev, 3 times_host, 4 n_frames, 5 track, 6 dtype, 7 track_len, 8 rate, 9 total, 10 max, 11 min,
    #       12 similarity threshold, 13 rms_cut, 14 silent_without_rms, 15 max_windows, 16 max_steps, 17 records, 18 state,
    #       19 workspace, 20 workspace_bytes, 21 stream
    good = [SCORES, FLAGS, TIMES, T, 4, TRACK, 1, 3000, 1000, 3.0, 10.0, 5.0, 0.95, 0.01, 1, 20, 8, REC, STATE, WS, BIG, None]

    def but(**changes):
        return [changes.get(f"a{i}", v) for i, v in enumerate(good)]

    for at in (0, 1, 2, 3, 17, 18, 19):                           # (a null track is no error: it means no audio)
        refused(*but(**{f"a{at}": None}), say=b"null pointer")
    refused(*but(a4=-1), say=b"negative")
    refused(*but(a11=0.0), say=b"must be positive")
    refused(*but(a11=-5.0), say=b"must be positive")
    for at in (9, 10, 11):
        for bad in (float("nan"), float("inf"), float("-inf")):
            refused(*but(**{f"a{at}": bad}), say=b"not finite")
    for at in (12, 13):
        refused(*but(**{f"a{at}": float("nan")}), say=b"NaN")
    for bad_times, say in (((0.0, 2.0, 1.0, 3.0), b"unsorted"), ((0.0, 1.0, float("nan"), 3.0), b"not finite"),
                           ((0.0, 1.0, 2.0, float("inf")), b"not finite"), ((1.0, 0.0, 0.0, 0.0), b"unsorted")):
        worse = (ctypes.c_double * 4)(*bad_times)
        refused(*but(a3=ctypes.addressof(worse)), say=say)
    for at, step in ((0, 4), (2, 4), (17, 4), (18, 4), (19, 4), (1, 2), (5, 8)):
        refused(*but(**{f"a{at}": good[at] + step}), say=b"misaligned")
    refused(*but(a16=0), say=b"max_steps")
    refused(*but(a15=-1), say=b"max_windows")
    refused(*but(a15=0), say=b"max_windows")                      # with audio at least one window row
    refused(*but(a6=2), say=b"track_dtype")
    refused(*but(a7=-1), say=b"track_len")
    refused(*but(a8=1), say=b"sample_rate")
    refused(*but(a9=1e13, a8=1000), say=b"2^52")
    refused(*but(a20=need - 1), say=b"workspace", code=HMM_E_WORKSPACE)
    refused(*but(a20=0), say=b"workspace", code=HMM_E_WORKSPACE)


def test_device_walk_has_no_cpu_fallback(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from hippomm_amd import _lib, segmentation as seg
    with pytest.raises(_lib.HippoMMHipError, match="no CPU fallback"):
        seg.segment_sequence([str(tmp_path / "a.png"), str(tmp_path / "b.png")], [0.0, 1.0], walk="device")
    with pytest.raises(ValueError, match="walk must be"):
        seg.segment_sequence(None, None, np.zeros(100), 10, walk="gpu")
    with pytest.raises(ValueError, match="AudioTrack"):
        seg.segment_sequence(None, None, np.zeros(100), 10, walk="device")
