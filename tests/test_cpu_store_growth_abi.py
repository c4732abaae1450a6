"""CPU: the C ABI of the growing store (hmm_store_ingest_rows, hmm_store_gather_segments) -- declared, exported and bound, the ABI
version unchanged, every argument error reported as a status code with the function's name on a host without a GPU (nothing is
dereferenced or launched before the checks), and zero counts answered with HMM_OK."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NEW = ["hmm_store_ingest_rows", "hmm_store_gather_segments"]
HMM_OK, HMM_E_INVALID = 0, -1
ONE = 1 << 20                                                    # a 16-byte aligned non-null dummy
FAR = 1 << 40                                                    # another one, far from the first


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


def test_ingest_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call, name = lib.hmm_store_ingest_rows, b"store_ingest_rows"

    def refused(*args, say):
        assert call(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg

    #      src, dtype, n_new, dim, store, shadow, capacity, row_offset, stream
    refused(ONE, 0, 5, 512, FAR, None, 100, 0, None, say=b"dim must be 1024")
    refused(ONE, 2, 5, 1024, FAR, None, 100, 0, None, say=b"src_dtype")
    refused(ONE, -1, 5, 1024, FAR, None, 100, 0, None, say=b"src_dtype")
    refused(ONE, 0, -1, 1024, FAR, None, 100, 0, None, say=b"negative")
    refused(ONE, 0, 5, 1024, FAR, None, -100, 0, None, say=b"negative")
    refused(ONE, 0, 5, 1024, FAR, None, 100, -1, None, say=b"negative")
    refused(ONE, 0, 5, 1024, FAR, None, 100, 96, None, say=b"exceed the capacity")
    refused(ONE, 0, 101, 1024, FAR, None, 100, 0, None, say=b"exceed the capacity")
    refused(ONE, 0, 1, 1024, FAR, None, 100, 2 ** 63 - 1, None, say=b"exceed the capacity")      # no overflow in the sum
    refused(None, 0, 5, 1024, FAR, None, 100, 0, None, say=b"null pointer")
    refused(ONE, 0, 5, 1024, None, None, 100, 0, None, say=b"null pointer")
    refused(ONE + 4, 0, 5, 1024, FAR, None, 100, 0, None, say=b"16-byte aligned")
    refused(ONE, 0, 5, 1024, FAR + 8, None, 100, 0, None, say=b"16-byte aligned")
    refused(ONE, 0, 5, 1024, FAR, 2 * FAR + 2, 100, 0, None, say=b"16-byte aligned")
    # overlap, by plain pointer arithmetic on the bytes read and the bytes written (rows 10 .. 15 of the store here)
    store = FAR
    for dtype, row_bytes in ((0, 4096), (1, 8192)):
        refused(store + 10 * 4096, dtype, 5, 1024, store, None, 100, 10, None, say=b"overlaps")
        refused(store + 15 * 4096 - 16, dtype, 5, 1024, store, None, 100, 10, None, say=b"overlaps")            # its first 16 bytes
        refused(store + 10 * 4096 - 5 * row_bytes + 16, dtype, 5, 1024, store, None, 100, 10, None, say=b"overlaps")   # its last 16
    shadow = 2 * FAR
    refused(shadow + 10 * 2048, 0, 5, 1024, store, shadow, 100, 10, None, say=b"overlaps")
    refused(shadow + 15 * 2048 - 16, 0, 5, 1024, store, shadow, 100, 10, None, say=b"overlaps")


def test_gather_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call, name = lib.hmm_store_gather_segments, b"store_gather_segments"
    src, src_sh, dst, dst_sh, tab = FAR, 2 * FAR, 3 * FAR, 4 * FAR, ONE

    def refused(*args, say):
        assert call(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg

    #      src_store, src_shadow, src_rows, src_offsets, n_src, src_segment, dst_offsets, n_dst, dim, dst_store, dst_shadow, dst_rows, dst_cap
    refused(src, src_sh, 50, tab, 4, tab, tab, 3, 512, dst, dst_sh, 40, 64, None, say=b"dim must be 1024")
    refused(src, src_sh, -1, tab, 4, tab, tab, 3, 1024, dst, dst_sh, 40, 64, None, say=b"negative")
    refused(src, src_sh, 50, tab, -4, tab, tab, 3, 1024, dst, dst_sh, 40, 64, None, say=b"negative")
    refused(src, src_sh, 50, tab, 4, tab, tab, -3, 1024, dst, dst_sh, 40, 64, None, say=b"negative")
    refused(src, src_sh, 50, tab, 4, tab, tab, 3, 1024, dst, dst_sh, -40, 64, None, say=b"negative")
    refused(src, src_sh, 50, tab, 4, tab, tab, 3, 1024, dst, dst_sh, 40, -64, None, say=b"negative")
    refused(src, src_sh, 50, tab, 4, tab, tab, 3, 1024, dst, dst_sh, 65, 64, None, say=b"exceeds the capacity")
    refused(src, None, 50, tab, 4, tab, tab, 3, 1024, dst, dst_sh, 40, 64, None, say=b"both")
    refused(src, src_sh, 50, tab, 4, tab, tab, 3, 1024, dst, None, 40, 64, None, say=b"both")
    for missing in range(5):                                     # source store, source offsets, segment table, destination offsets, destination
        p = [None if i == missing else v for i, v in enumerate((src, tab, tab, tab, dst))]
        refused(p[0], src_sh, 50, p[1], 4, p[2], p[3], 3, 1024, p[4], dst_sh, 40, 64, None, say=b"null pointer")
    for bad in range(4):                                         # the four row pointers
        p = [v + 8 if i == bad else v for i, v in enumerate((src, src_sh, dst, dst_sh))]
        refused(p[0], p[1], 50, tab, 4, tab, tab, 3, 1024, p[2], p[3], 40, 64, None, say=b"16-byte aligned")
    # overlap: the gather is out of place
    refused(src, None, 50, tab, 4, tab, tab, 3, 1024, src, None, 40, 64, None, say=b"overlaps")
    refused(src, None, 50, tab, 4, tab, tab, 3, 1024, src + 50 * 4096 - 16, None, 40, 64, None, say=b"overlaps")
    refused(src, None, 50, tab, 4, tab, tab, 3, 1024, src - 40 * 4096 + 16, None, 40, 64, None, say=b"overlaps")
    refused(src, src_sh, 50, tab, 4, tab, tab, 3, 1024, dst, src_sh + 50 * 2048 - 16, 40, 64, None, say=b"overlaps")
    refused(src, src_sh, 50, tab, 4, tab, tab, 3, 1024, src_sh, dst_sh, 40, 64, None, say=b"overlaps")


def test_zero_counts_return_ok_without_a_launch():
    """No GPU on this host: a launch would fail, HMM_OK means none was tried."""
    lib = _lib()
    assert lib.hmm_store_ingest_rows(ONE, 0, 0, 1024, FAR, None, 100, 0, None) == HMM_OK
    assert lib.hmm_store_ingest_rows(ONE, 1, 0, 1024, FAR, 2 * FAR, 100, 100, None) == HMM_OK
    assert lib.hmm_store_ingest_rows(ONE, 0, 0, 1024, FAR, None, 0, 0, None) == HMM_OK
    assert lib.hmm_store_gather_segments(FAR, None, 50, ONE, 4, ONE, ONE, 0, 1024, 3 * FAR, None, 0, 64, None) == HMM_OK
    assert lib.hmm_store_gather_segments(FAR, 2 * FAR, 50, ONE, 4, ONE, ONE, 0, 1024, 3 * FAR, 4 * FAR, 0, 0, None) == HMM_OK
    assert lib.hmm_store_gather_segments(FAR, None, 50, ONE, 4, ONE, ONE, 3, 1024, 3 * FAR, None, 0, 64, None) == HMM_OK
