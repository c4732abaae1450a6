"""Files for the device entropy pass's tests (plain helper module): the corpus the route must decode itself, and the seeded damage
sweep of test_cpu_jpeg.test_damaged_files_get_a_status_and_never_crash (same seeds, same order of draws)."""
import functools

import numpy as np
from PIL import Image

from hippomm_amd import _lib, jpeg
from test_cpu_jpeg import encode, frame


def noise(w, h, seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def corpus():
    """-> ((name, bytes), ...)"""
    return (
        ("grey_8x8", encode(frame(8, 8, seed=1, mode="L"), quality=90)),                                # one block
        ("420_16x16", encode(frame(16, 16, seed=2), quality=90, subsampling=2)),                        # one MCU
        ("422_17x9", encode(frame(17, 9, seed=3), quality=90, subsampling=1)),                          # partial MCUs
        ("444_40x24", encode(frame(40, 24, seed=4), quality=90, subsampling=0)),
        ("noise_q100_64x64", encode(noise(64, 64, 5), quality=100, subsampling=0)),                     # 16-bit codes, dense FF 00
        ("flat_320x200", encode(Image.new("RGB", (320, 200), (200, 30, 90)), quality=90, subsampling=2)),   # EOB-only blocks
        ("noise_q95_256x144", encode(noise(256, 144, 6), quality=95, subsampling=2)),                   # dozens of subsequences
        ("noise_q95_256x144_opt", encode(noise(256, 144, 6), quality=95, subsampling=2, optimize=True)),   # per-file tables
        ("noise_q95_640x360", encode(noise(640, 360, 7), quality=95, subsampling=2)),                   # several subsequences per thread
    )


def windows(geometry):
    """The whole frame, an interior window, and one that touches the right and bottom edges."""
    w, h = geometry[0], geometry[1]
    return ((0, 0, w, h), (w // 4, h // 4, max(w // 2, 1), max(h // 2, 1)), (w // 2, h // 2, w - w // 2, h - h // 2))


@functools.lru_cache(maxsize=None)
def damage_sweep():
    """-> ((geometry, bytes), ...): 4 sources x (40 truncations + 160 byte flips), geometry the undamaged source's."""
    rng = np.random.default_rng(1234)
    sources = [encode(frame(130, 90, seed=s), quality=q, subsampling=sub, **kw)
               for s, q, sub, kw in ((1, 90, 2, {}), (2, 30, 0, {}), (3, 75, 1, dict(restart_marker_blocks=3)),
                                     (4, 95, 2, dict(optimize=True)))]
    out = []
    for data in sources:
        g = jpeg.parse(data)
        cases = [data[:int(k)] for k in rng.integers(0, len(data), 40)]
        for _ in range(160):
            b = bytearray(data)
            for pos in rng.integers(0, len(b), int(rng.integers(1, 4))):
                b[pos] = int(rng.integers(0, 256))
            cases.append(bytes(b))
        out.extend((g, case) for case in cases)
    return tuple(out)


def entropy_slot_bytes(file_bytes):
    return int(_lib.load().hmm_jpeg_entropy_slot_bytes(file_bytes))


def prepare(data, geometry, extra=0):
    """The prepare pass -> (status, the bitstream slot as a u8 array of hmm_jpeg_entropy_slot_bytes(len(data)) + extra bytes)."""
    n = entropy_slot_bytes(len(data)) + extra
    raw = np.zeros(n + 16, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 16
    slot = raw[skew:skew + n]
    g = np.zeros(jpeg.GEOMETRY_INTS, dtype=np.int32)
    g[:len(geometry)] = geometry
    st = _lib.load().hmm_jpeg_prepare_entropy(data, len(data), g.ctypes.data, slot.ctypes.data, n)
    return int(st), slot


def host_slot(data, geometry, window):
    slot = np.zeros(jpeg.slot_bytes(geometry, window), dtype=np.uint8)
    return jpeg.decode_coefs(data, geometry, window, slot), slot
