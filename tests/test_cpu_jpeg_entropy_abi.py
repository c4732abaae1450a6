"""CPU: the C ABI of the device entropy route (hmm_jpeg_entropy_slot_bytes, hmm_jpeg_prepare_entropy,
hmm_jpeg_entropy_workspace_bytes, hmm_jpeg_decode_coefs_device) -- declared, exported and bound, the ABI version unchanged, every
argument error reported as a status code with the function's name on a host without a GPU (nothing is dereferenced or launched
before the checks), n = 0 answered with HMM_OK; and the prepare pass itself, which needs no GPU, on the corpus."""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np
import pytest

import jpeg_entropy_corpus as jc
from hippomm_amd import jpeg
from test_cpu_jpeg import encode, frame, unsupported_files

ROOT = Path(__file__).resolve().parent.parent
NEW = ["hmm_jpeg_entropy_slot_bytes", "hmm_jpeg_prepare_entropy", "hmm_jpeg_entropy_workspace_bytes", "hmm_jpeg_decode_coefs_device"]
HMM_OK, HMM_E_INVALID, HMM_E_WORKSPACE = 0, -1, -2
ONE = 1 << 20                                                    # a 16-byte aligned non-null dummy
FAR = 1 << 40
HEADER_INTS, QT_OFF, HUFF_OFF, DATA_OFF, PAD = 16, 64, 576, 6272, 16   # jpeg_entropy_core.h


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def _geom(*g):
    a = np.zeros(jpeg.GEOMETRY_INTS, dtype=np.int32)
    a[:len(g)] = g
    return a


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


def test_device_pass_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call, name = lib.hmm_jpeg_decode_coefs_device, b"jpeg_decode_coefs_device"
    g = _geom(64, 48, 3, 2, 2)
    gp = g.ctypes.data
    win = (0, 0, 64, 48)
    slot = jpeg.slot_bytes(tuple(g), win)
    bstride = 16384
    ws = lib.hmm_jpeg_entropy_workspace_bytes(gp, 3, bstride)
    assert ws > 0 and ws % 256 == 0

    def refused(*args, say, code=HMM_E_INVALID):
        assert call(*args) == code, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg

    #      bitslots, n, bitslot_stride, geometry, x0, y0, w, h, coef_slots, coef_slot_stride, status, workspace, workspace_bytes, stream
    for missing in range(4):
        p = [None if i == missing else v for i, v in enumerate((ONE, FAR, 2 * FAR, 3 * FAR))]
        refused(p[0], 3, bstride, gp, *win, p[1], slot, p[2], p[3], ws, None, say=b"null pointer")
    refused(ONE, 3, bstride, None, *win, FAR, slot, 2 * FAR, 3 * FAR, ws, None, say=b"null pointer")
    refused(ONE + 8, 3, bstride, gp, *win, FAR, slot, 2 * FAR, 3 * FAR, ws, None, say=b"16-byte aligned")
    refused(ONE, 3, bstride, gp, *win, FAR + 4, slot, 2 * FAR, 3 * FAR, ws, None, say=b"16-byte aligned")
    refused(ONE, 3, bstride, gp, *win, FAR, slot, 2 * FAR, 3 * FAR + 8, ws, None, say=b"16-byte aligned")
    refused(ONE, 3, bstride, gp, *win, FAR, slot, 2 * FAR + 2, 3 * FAR, ws, None, say=b"4-byte aligned")
    refused(ONE, -1, bstride, gp, *win, FAR, slot, 2 * FAR, 3 * FAR, ws, None, say=b"negative")
    refused(ONE, 3, bstride, gp, *win, FAR, slot - 16, 2 * FAR, 3 * FAR, ws, None, say=b"coefficient slot stride")
    refused(ONE, 3, bstride, gp, *win, FAR, slot + 8, 2 * FAR, 3 * FAR, ws, None, say=b"coefficient slot stride")
    refused(ONE, 3, DATA_OFF, gp, *win, FAR, slot, 2 * FAR, 3 * FAR, ws, None, say=b"bitstream slot stride")
    refused(ONE, 3, bstride + 4, gp, *win, FAR, slot, 2 * FAR, 3 * FAR, ws, None, say=b"bitstream slot stride")
    for bad in ((0, 0, 65, 48), (0, 0, 64, 49), (-1, 0, 8, 8), (60, 40, 8, 8), (0, 0, 0, 8)):
        refused(ONE, 3, bstride, gp, *bad, FAR, slot, 2 * FAR, 3 * FAR, ws, None, say=b"window")
    refused(ONE, 3, bstride, _geom(64, 48, 2, 1, 1).ctypes.data, *win, FAR, slot, 2 * FAR, 3 * FAR, ws, None, say=b"geometry")
    refused(ONE, 3, bstride, _geom(64, 48, 3, 1, 2).ctypes.data, *win, FAR, slot, 2 * FAR, 3 * FAR, ws, None, say=b"geometry")
    refused(ONE, 3, bstride, gp, *win, FAR, slot, 2 * FAR, 3 * FAR, ws - 1, None, say=b"workspace", code=HMM_E_WORKSPACE)
    refused(ONE, 1, bstride, gp, *win, FAR, slot, 2 * FAR, 3 * FAR, lib.hmm_jpeg_entropy_workspace_bytes(gp, 1, bstride) - 1, None,
            say=b"workspace", code=HMM_E_WORKSPACE)


def test_workspace_query():
    lib = _lib()
    gp = _geom(64, 48, 3, 2, 2).ctypes.data
    one = lib.hmm_jpeg_entropy_workspace_bytes(gp, 1, 16384)
    assert one > 0 and lib.hmm_jpeg_entropy_workspace_bytes(gp, 5, 16384) == 5 * one
    assert lib.hmm_jpeg_entropy_workspace_bytes(gp, 32, 16384) == lib.hmm_jpeg_entropy_workspace_bytes(gp, 256, 16384) == 32 * one
    assert lib.hmm_jpeg_entropy_workspace_bytes(gp, 1, 1 << 20) > one                    # more subsequences to keep states for
    assert lib.hmm_jpeg_entropy_workspace_bytes(gp, 0, 16384) == 0
    assert lib.hmm_jpeg_entropy_workspace_bytes(None, 1, 16384) == 0
    assert lib.hmm_jpeg_entropy_workspace_bytes(_geom(64, 48, 2, 1, 1).ctypes.data, 1, 16384) == 0


def test_zero_frames_return_ok_without_a_launch():
    """No GPU on this host: a launch would fail, HMM_OK means none was tried."""
    lib = _lib()
    g = _geom(64, 48, 3, 2, 2)
    slot = jpeg.slot_bytes(tuple(g), (0, 0, 64, 48))
    assert lib.hmm_jpeg_decode_coefs_device(ONE, 0, 16384, g.ctypes.data, 0, 0, 64, 48, FAR, slot, 2 * FAR, 3 * FAR, 0, None) == HMM_OK


def test_prepare_argument_errors():
    lib = _lib()
    data = jc.corpus()[1][1]
    g = _geom(*jpeg.parse(data))
    n = jc.entropy_slot_bytes(len(data))
    assert n % 256 == 0 and n >= len(data) + DATA_OFF
    raw = np.zeros(n + 32, dtype=np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 16
    for args in ((None, len(data), g.ctypes.data, base, n), (data, len(data), None, base, n), (data, len(data), g.ctypes.data, None, n)):
        assert lib.hmm_jpeg_prepare_entropy(*args) == HMM_E_INVALID
        assert b"jpeg_prepare_entropy" in lib.hmm_last_error() and b"null pointer" in lib.hmm_last_error()
    assert lib.hmm_jpeg_prepare_entropy(data, len(data), g.ctypes.data, base + 4, n) == HMM_E_INVALID
    assert b"16-byte aligned" in lib.hmm_last_error()
    st, slot = jc.prepare(data, tuple(g))
    need = DATA_OFF + int(slot[:64].view(np.int32)[6])
    assert lib.hmm_jpeg_prepare_entropy(data, len(data), g.ctypes.data, base, need) == jpeg.DECODED
    assert lib.hmm_jpeg_prepare_entropy(data, len(data), g.ctypes.data, base, need - 1) == HMM_E_WORKSPACE
    assert b"jpeg_prepare_entropy" in lib.hmm_last_error()


def _scan(data):
    """-> (first byte of the entropy data, index of the EOI marker that ends it) by a plain walk over the markers."""
    pos = 2
    while True:
        assert data[pos] == 0xFF
        marker, length = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])[0]
        pos += 2 + length
        if marker == 0xDA:
            break
    end = pos
    while not (data[end] == 0xFF and data[end + 1] != 0):
        end += 1
    assert data[end + 1] == 0xD9
    return pos, end


@pytest.mark.parametrize("name", [name for name, _ in jc.corpus()])
def test_prepare_pass_on_the_corpus(name):
    data = dict(jc.corpus())[name]
    g = jpeg.parse(data)
    assert g is not None and g[5] == 0
    st, slot = jc.prepare(data, g)
    assert st == jpeg.DECODED
    head = slot[:4 * HEADER_INTS].view(np.int32)
    start, end = _scan(data)
    stuffed = data[start:end].count(b"\xff\x00")
    assert int(head[0]) == 0x544E454A                                                   # "JENT"
    assert int(head[1]) == end - start - stuffed                                        # the scan without its FF 00 stuffing
    assert tuple(head[2:5]) == (g[2], g[3], g[4])
    assert int(head[6]) % PAD == 0 and 0 <= int(head[6]) - int(head[1]) < PAD
    assert not head[7:].any()
    assert DATA_OFF + int(head[6]) <= slot.nbytes
    body = slot[DATA_OFF:DATA_OFF + int(head[1])].tobytes()
    assert body == data[start:end].replace(b"\xff\x00", b"\xff")
    assert not slot[DATA_OFF + int(head[1]):DATA_OFF + int(head[6])].any()              # zero padding
    # the quantisation tables are the ones the host pass puts at the head of a coefficient slot
    st, host = jc.host_slot(data, g, (0, 0, g[0], g[1]))
    assert st == jpeg.DECODED
    np.testing.assert_array_equal(slot[QT_OFF:QT_OFF + 512], host[:512])
    sel = int(head[5])
    assert all(((sel >> (2 * k)) & 3) < 4 for k in range(6)) and sel >> (4 * g[2]) == 0
    if name in ("noise_q100_64x64",):
        assert stuffed > 0


def test_prepare_refuses_what_the_route_does_not_take():
    im = frame(64, 48, seed=2)
    g = (64, 48, 3, 1, 1, 0)
    for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=5), dict(restart_marker_rows=1)):
        data = encode(im, quality=90, subsampling=0, **kw)
        assert jpeg.parse(data)[5] > 0
        assert jc.prepare(data, g)[0] == jpeg.UNSUPPORTED
        assert jc.host_slot(data, g, (0, 0, 64, 48))[0] == jpeg.DECODED                  # such a file keeps the host entropy pass
    other = encode(frame(130, 90), quality=90, subsampling=2)
    assert jc.prepare(other, (130, 90, 3, 1, 1, 0))[0] == jpeg.OTHER_GEOMETRY
    assert jc.prepare(other, (64, 48, 3, 2, 2, 0))[0] == jpeg.OTHER_GEOMETRY
    for name, data in sorted(unsupported_files().items()):
        assert jc.prepare(data, g)[0] == jpeg.UNSUPPORTED, name
    base = encode(im, quality=90, subsampling=0)
    start, end = _scan(base)
    assert jc.prepare(base, g)[0] == jpeg.DECODED
    assert jc.prepare(base[:end], g)[0] == jpeg.UNSUPPORTED                              # no EOI
    assert jc.prepare(base[:end + 1], g)[0] == jpeg.UNSUPPORTED
    assert jc.prepare(base[:end] + b"\xff\xd0" + base[end:], g)[0] == jpeg.UNSUPPORTED   # another marker before the EOI
    assert jc.prepare(base + b"trailing bytes", g)[0] == jpeg.DECODED                    # what follows the EOI is not looked at
