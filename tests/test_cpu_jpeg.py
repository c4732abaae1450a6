"""CPU: the host entropy pass (hippomm_amd/csrc/jpeg_host.cpp through ctypes) plus the numpy restatement of the device
reconstruction (tests/jpeg_oracle.py) give Pillow's pixels bit for bit; files outside the supported class are classified as
such; damaged files always get a status and never crash the decoder.  Test files are written here with Pillow's encoder."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import jpeg_oracle as oracle
from hippomm_amd import jpeg

SIZES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (130, 90), (3, 5), (4, 4), (5, 3)]
LARGE = [(1279, 719), (1280, 720), (1920, 1080)]
QUALITIES = [5, 30, 75, 90, 95, 100]


def frame(w, h, seed=0, mode="RGB"):
    """Smooth gradients, noise and saturated colour patches (they push the colour conversion into its clamps)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 3) % 256], axis=-1).astype(np.int32)
    img = np.clip(img + rng.integers(-40, 41, img.shape), 0, 255)
    for k, colour in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]):
        x0, y0 = (k * w) // 6, (k * h) // 7
        img[y0:y0 + max(h // 5, 1), x0:x0 + max(w // 6, 1)] = colour
    im = Image.fromarray(img.astype(np.uint8))
    return im.convert("L") if mode == "L" else im


def encode(im, **kw):
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def device_route(data, window=None):
    """Entropy pass + numpy reconstruction -> (h, w, 3) u8, or None when the decoder does not take the file."""
    g = jpeg.parse(data)
    if g is None:
        return None
    window = window or (0, 0, g[0], g[1])
    slot = np.zeros(jpeg.slot_bytes(g, window), dtype=np.uint8)
    assert oracle.layout(g, window)["slot_bytes"] == slot.nbytes
    st = jpeg.decode_coefs(data, g, window, slot)
    return oracle.reconstruct(slot, g, window) if st == jpeg.DECODED else None


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_matrix_equals_pillow(size, subsampling):
    im = frame(*size, seed=size[0] * 31 + size[1])
    for q in QUALITIES:
        for optimize in (False, True):
            data = encode(im, quality=q, subsampling=subsampling, optimize=optimize)
            got = device_route(data)
            assert got is not None, (q, optimize)
            np.testing.assert_array_equal(got, pillow(data), err_msg=f"q={q} optimize={optimize}")


@pytest.mark.parametrize("size", LARGE, ids=[f"{w}x{h}" for w, h in LARGE])
@pytest.mark.parametrize("subsampling", [0, 1, 2])
def test_large_frames_equal_pillow(size, subsampling):
    im = frame(*size, seed=7)
    for q, optimize in ((90, False), (100, True) if subsampling == 2 else (30, False)):
        data = encode(im, quality=q, subsampling=subsampling, optimize=optimize)
        np.testing.assert_array_equal(device_route(data), pillow(data), err_msg=f"q={q}")


@pytest.mark.parametrize("kw", [dict(restart_marker_blocks=1), dict(restart_marker_blocks=5), dict(restart_marker_rows=1),
                                dict(restart_marker_rows=2)], ids=["blocks1", "blocks5", "rows1", "rows2"])
@pytest.mark.parametrize("subsampling", [0, 2])
def test_restart_markers(kw, subsampling):
    for size in ((130, 90), (15, 17), (1280, 720)):
        data = encode(frame(*size, seed=3), quality=85, subsampling=subsampling, **kw)
        assert b"\xff\xdd" in data
        assert jpeg.parse(data)[5] > 0
        np.testing.assert_array_equal(device_route(data), pillow(data))


@pytest.mark.parametrize("size", [(1, 1), (7, 9), (130, 90), (1280, 720)])
def test_grey(size):
    for q in (5, 75, 100):
        data = encode(frame(*size, seed=5, mode="L"), quality=q)
        assert jpeg.parse(data)[2] == 1
        np.testing.assert_array_equal(device_route(data), pillow(data))


def test_metadata_segments_are_skipped():
    im = frame(130, 90, seed=9)
    exif = Image.Exif()
    exif[0x010F] = "maker"
    exif[0x0110] = "model"
    icc = b"\0" * 128 + b"acsp" + bytes(range(256)) * 4                  # APP2 ICC_PROFILE bytes; only skipped here
    data = encode(im, quality=90, exif=exif.tobytes(), icc_profile=icc, comment=b"a comment")
    for tag in (b"Exif", b"ICC_PROFILE", b"\xff\xfe"):
        assert tag in data
    np.testing.assert_array_equal(device_route(data), pillow(data))


def test_window_equals_crop_of_full_decode():
    rng = np.random.default_rng(1)
    for size, sub in (((1280, 720), 2), ((130, 90), 1), ((130, 90), 0), ((15, 17), 2), ((5, 3), 2)):
        data = encode(frame(*size, seed=11), quality=90, subsampling=sub)
        full = pillow(data)
        for _ in range(6):
            x0, y0 = int(rng.integers(0, size[0])), int(rng.integers(0, size[1]))
            w, h = int(rng.integers(1, size[0] - x0 + 1)), int(rng.integers(1, size[1] - y0 + 1))
            got = device_route(data, (x0, y0, w, h))
            np.testing.assert_array_equal(got, full[y0:y0 + h, x0:x0 + w], err_msg=str((size, sub, x0, y0, w, h)))


def _segment(marker, body):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(body) + 2) + body


def _patch_sof(data, fn):
    i = data.index(b"\xff\xc0")
    out = bytearray(data)
    fn(out, i)
    return bytes(out)


def unsupported_files():
    im = frame(64, 48, seed=2)
    base = encode(im, quality=90, subsampling=0)
    files = {
        "progressive": encode(im, quality=90, progressive=True),
        "arithmetic": _patch_sof(base, lambda b, i: b.__setitem__(i + 1, 0xC9)),        # SOF9: arithmetic sequential
        "lossless": _patch_sof(base, lambda b, i: b.__setitem__(i + 1, 0xC3)),
        "12bit": _patch_sof(base, lambda b, i: b.__setitem__(i + 4, 12)),
        "cmyk": encode(im.convert("CMYK"), quality=90),
        "adobe": base[:2] + _segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01") + base[2:],
        "rgb_ids": _patch_sof(base, lambda b, i: [b.__setitem__(i + 10 + 3 * c, v) for c, v in enumerate(b"RGB")]),
        "440": _patch_sof(base, lambda b, i: b.__setitem__(i + 11, 0x12)),             # luma 1x2
        "411": _patch_sof(base, lambda b, i: b.__setitem__(i + 11, 0x41)),             # luma 4x1
        "dnl_height0": _patch_sof(base, lambda b, i: b.__setitem__(slice(i + 5, i + 7), b"\0\0")),
        "png": (lambda buf: (im.save(buf, "PNG"), buf.getvalue())[1])(io.BytesIO()),
        "empty": b"",
        "soi_only": b"\xff\xd8",
    }
    g = jpeg.parse(base)
    assert g is not None and g[3:5] == (1, 1)
    return files


@pytest.mark.parametrize("name", sorted(unsupported_files()))
def test_unsupported_files_are_classified(name):
    data = unsupported_files()[name]
    assert jpeg.parse(data) is None
    g = (64, 48, 3, 1, 1, 0)
    slot = np.zeros(jpeg.slot_bytes(g, (0, 0, 64, 48)), dtype=np.uint8)
    assert jpeg.decode_coefs(data, g, (0, 0, 64, 48), slot) == jpeg.UNSUPPORTED


def test_other_geometry_is_reported():
    data = encode(frame(130, 90), quality=90, subsampling=2)
    g = (130, 90, 3, 1, 1, 0)                                            # the file is 4:2:0
    slot = np.zeros(jpeg.slot_bytes(g, (0, 0, 130, 90)), dtype=np.uint8)
    assert jpeg.decode_coefs(data, g, (0, 0, 130, 90), slot) == jpeg.OTHER_GEOMETRY


def test_damaged_files_get_a_status_and_never_crash():
    """Seeded truncations and byte flips.  Whatever the decoder still takes must be what Pillow decodes, without error."""
    rng = np.random.default_rng(1234)
    sources = [encode(frame(130, 90, seed=s), quality=q, subsampling=sub, **kw)
               for s, q, sub, kw in ((1, 90, 2, {}), (2, 30, 0, {}), (3, 75, 1, dict(restart_marker_blocks=3)),
                                     (4, 95, 2, dict(optimize=True)))]
    taken = 0
    for data in sources:
        g = jpeg.parse(data)
        window = (0, 0, g[0], g[1])
        slot = np.zeros(jpeg.slot_bytes(g, window), dtype=np.uint8)
        cases = [data[:int(k)] for k in rng.integers(0, len(data), 40)]
        for _ in range(160):
            b = bytearray(data)
            for pos in rng.integers(0, len(b), int(rng.integers(1, 4))):
                b[pos] = int(rng.integers(0, 256))
            cases.append(bytes(b))
        for case in cases:
            st = jpeg.decode_coefs(case, g, window, slot)
            assert st in (jpeg.DECODED, jpeg.UNSUPPORTED, jpeg.OTHER_GEOMETRY)
            if st == jpeg.DECODED:
                taken += 1
                np.testing.assert_array_equal(oracle.reconstruct(slot, g, window), pillow(case))
    assert taken > 0                                                     # flips in skipped segments and in the data survive
