"""The case table of the JPEG encoder's tests and a short numpy model of its stages: header, colour transform, edge replication,
chroma downsampling, forward DCT, quantisation, scan order with libjpeg's dummy blocks, symbol stream, bit packing with padding
and byte stuffing.  The model restates libjpeg (jcparam.c, jcmarker.c, jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c, jccoefct.c,
jchuff.c) stage by stage, so a mismatch with Pillow's bytes can be located by stage; ``mutant=`` switches one rule off at a time
for tests/test_cpu_jpeg_encode.py.  Plain helper module: numpy and Pillow only, no GPU, nothing of the package.

The oracle everywhere is ``Image.fromarray(x).save(buf, "JPEG", quality=q, subsampling=s)`` and the comparison is byte equality.
"""
from __future__ import annotations

import io
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
SCAN_TILE = 1024                                   # blocks per step of the device prefix sum (jpeg_encode_core.h, kEncScanTile)
MUTANTS = ("no_bias", "no_edge", "half_up", "dc_shared", "zrl_before_eob", "pad_zero", "last_unstuffed", "bgr_unswapped")

STD_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])            # natural index of zigzag position k


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def pillow_bytes(frame: np.ndarray, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "RGB") -> bytes:
    """Pillow's file for `frame` ((h, w, 3) in `channel_order`, or (h, w) grey)."""
    from PIL import Image
    buf = io.BytesIO()
    if frame.ndim == 2:
        Image.fromarray(frame, "L").save(buf, "JPEG", quality=quality)
    else:
        rgb = frame[..., ::-1] if channel_order == "BGR" else frame
        Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def header_bytes_of(data: bytes) -> int:
    """Length of FF D8 ... SOS inclusive in a file."""
    i = 2
    while True:
        marker, length = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        i += 2 + length
        if marker == 0xDA:
            return i


# ---- header -------------------------------------------------------------------------------------------------------------------
def quant_tables(quality: int) -> np.ndarray:
    """jpeg_set_quality(q, force_baseline) -> (2, 64) in natural order."""
    q = max(1, min(100, int(quality)))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((t * scale + 50) // 100, 1, 255) for t in (STD_LUMA_Q, STD_CHROMA_Q)])


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(w: int, h: int, ncomp: int, hs: int, vs: int, quality: int) -> bytes:
    qt = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if ncomp == 3 else 1):
        out += _segment(0xDB, bytes([t]) + bytes(qt[t][ZIGZAG].tolist()))
    comps = [(1, hs << 4 | vs, 0), (2, 0x11, 1), (3, 0x11, 1)] if ncomp == 3 else [(1, 0x11, 0)]
    out += _segment(0xC0, b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([ncomp]) + b"".join(bytes(c) for c in comps))
    tables = [(0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS)]
    if ncomp == 3:
        tables += [(0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)]
    for ident, bits, vals in tables:
        out += _segment(0xC4, bytes([ident]) + bytes(bits) + bytes(vals))
    sel = [(1, 0x00), (2, 0x11), (3, 0x11)][:ncomp]
    return out + _segment(0xDA, bytes([ncomp]) + b"".join(bytes(s) for s in sel) + b"\x00\x3f\x00")


def huffman_codes(bits, vals) -> Dict[int, Tuple[int, int]]:
    """symbol -> (code, length), Annex C."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


# ---- pixel stages -------------------------------------------------------------------------------------------------------------
def color(frame: np.ndarray, channel_order: str = "RGB", mutant: Optional[str] = None) -> List[np.ndarray]:
    """jccolor.c: (h, w, 3) -> [Y, Cb, Cr] as int64 planes; (h, w) -> [Y]."""
    if frame.ndim == 2:
        return [frame.astype(np.int64)]
    px = frame.astype(np.int64)
    if channel_order == "BGR" and mutant != "bgr_unswapped":
        px = px[..., ::-1]
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    return [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]


def expand(plane: np.ndarray, width: int, height: int, mutant: Optional[str] = None) -> np.ndarray:
    """The right edge and the last row replicated up to width x height."""
    h, w = plane.shape
    mode = "constant" if mutant == "no_edge" else "edge"
    return np.pad(plane, ((0, height - h), (0, width - w)), mode=mode)


def downsample(plane: np.ndarray, hs: int, vs: int, mutant: Optional[str] = None) -> np.ndarray:
    """jcsample.c's box filter on a plane whose sides are multiples of (vs, hs): bias 0,1,0,1.. (h2v1) and 1,2,1,2.. (h2v2)."""
    if hs == 1 and vs == 1:
        return plane
    h, w = plane.shape
    cols = np.arange(w // hs)
    if vs == 1:
        bias = np.zeros_like(cols) if mutant == "no_bias" else cols & 1
        return (plane[:, 0::2] + plane[:, 1::2] + bias) >> 1
    bias = np.full_like(cols, 2) if mutant == "no_bias" else 1 + (cols & 1)
    return (plane[0::2, 0::2] + plane[0::2, 1::2] + plane[1::2, 0::2] + plane[1::2, 1::2] + bias) >> 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first: bool):
    """jfdctint.c along the last axis (CONST_BITS 13, PASS1_BITS 2)."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 + t12 * -15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(plane: np.ndarray, q: np.ndarray, mutant: Optional[str] = None) -> np.ndarray:
    """A sample plane whose sides are multiples of 8 -> (block rows, block columns, 64) quantised coefficients, natural order."""
    h, w = plane.shape
    blocks = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    rows = _fdct_1d(blocks, True)
    out = _fdct_1d(rows.swapaxes(-1, -2), False).swapaxes(-1, -2).reshape(h // 8, w // 8, 64)
    div = q.astype(np.int64) * 8                                      # the DCT's output carries a factor of 8
    if mutant == "half_up":
        return (out + div // 2) // div                                # floor: rounds halves up, also for negative values
    return np.sign(out) * ((np.abs(out) + div // 2) // div)


class Block(NamedTuple):
    comp: int
    coefs: np.ndarray                               # 64, zigzag order


def scan_blocks(frame: np.ndarray, quality: int, subsampling: str = "4:2:0", channel_order: str = "RGB",
                mutant: Optional[str] = None) -> List[Block]:
    """The frame's blocks in scan order.  A colour frame is one interleaved scan of MCUs of hs x vs luma blocks, Cb, Cr; where the
    luma block grid (ceil(w / 8) x ceil(h / 8)) ends inside the last MCU column or row, jccoefct.c fills the MCU with dummy blocks:
    no AC, the DC of the block before it in the MCU.  Grey is one block per MCU and has none."""
    qt = quant_tables(quality)
    planes = color(frame, channel_order, mutant)
    h, w = planes[0].shape
    if len(planes) == 1:
        c = fdct_quant(expand(planes[0], -(-w // 8) * 8, -(-h // 8) * 8, mutant), qt[0], mutant)
        return [Block(0, c[by, bx][ZIGZAG]) for by in range(c.shape[0]) for bx in range(c.shape[1])]
    hs, vs = SAMPLING[subsampling]
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    # jcprepct.c: the last row is replicated at full resolution only up to a whole row group (vs rows); below that, each
    # component's last DOWNSAMPLED row is replicated.  The right edge is replicated at full resolution (jcsample.c).
    groups = -(-h // vs)
    full = [expand(p, mcux * 8 * hs, groups * vs, mutant) for p in planes]
    small = [full[0]] + [downsample(p, hs, vs, mutant) for p in full[1:]]
    small = [expand(p, p.shape[1], mcuy * 8 * (vs if c == 0 else 1), mutant) for c, p in enumerate(small)]
    coefs = [fdct_quant(p, qt[min(c, 1)], mutant) for c, p in enumerate(small)]
    wib, hib = -(-w // 8), -(-h // 8)                                  # the luma blocks that exist
    out = []
    for my in range(mcuy):
        for mx in range(mcux):
            last = None
            for yi in range(vs):
                for xi in range(hs):
                    bx, by = mx * hs + xi, my * vs + yi
                    if bx < wib and by < hib:
                        last = coefs[0][by, bx]
                    else:
                        last = np.concatenate([last[:1], np.zeros(63, dtype=last.dtype)])
                    out.append(Block(0, last[ZIGZAG]))
            out += [Block(1, coefs[1][my, mx][ZIGZAG]), Block(2, coefs[2][my, mx][ZIGZAG])]
    return out


# ---- entropy stages -----------------------------------------------------------------------------------------------------------
def _category(v: int) -> int:
    return int(abs(int(v))).bit_length()


def _amplitude(v: int, nbits: int) -> Tuple[int, int]:
    v = int(v)
    return ((v - 1) if v < 0 else v) & ((1 << nbits) - 1), nbits


class Symbol(NamedTuple):
    kind: str                                       # "dc", "ac", "zrl", "eob" or "bits"
    code: int
    length: int
    value: int = 0                                  # dc: the difference; ac: the coefficient
    block: int = 0


def symbols(blocks: List[Block], mutant: Optional[str] = None) -> List[Symbol]:
    """jchuff.c's encode_one_block over the scan: the (code, length) stream, in order."""
    dc_tables = [huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(DC_CHROMA_BITS, DC_VALS)]
    ac_tables = [huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS)]
    pred = {}
    out = []
    for n, (comp, c) in enumerate(blocks):
        t = 0 if comp == 0 else 1
        key = 0 if mutant == "dc_shared" else comp
        diff = int(c[0]) - pred.get(key, 0)
        pred[key] = int(c[0])
        nbits = _category(diff)
        out.append(Symbol("dc", *dc_tables[t][nbits], diff, n))
        if nbits:
            out.append(Symbol("bits", *_amplitude(diff, nbits), diff, n))
        run = 0
        for k in range(1, 64):
            v = int(c[k])
            if v == 0:
                run += 1
                continue
            while run > 15:
                out.append(Symbol("zrl", *ac_tables[t][0xF0], 0, n))
                run -= 16
            nbits = _category(v)
            out.append(Symbol("ac", *ac_tables[t][run << 4 | nbits], v, n))
            out.append(Symbol("bits", *_amplitude(v, nbits), v, n))
            run = 0
        if run:
            if mutant == "zrl_before_eob":
                out += [Symbol("zrl", *ac_tables[t][0xF0], 0, n)] * (run // 16)
            out.append(Symbol("eob", *ac_tables[t][0x00], 0, n))
    return out


def pack(stream: List[Symbol], mutant: Optional[str] = None) -> bytes:
    """The bits, the last byte padded with ones, every FF followed by 00."""
    acc = nbits = 0
    for s in stream:
        acc = acc << s.length | s.code
        nbits += s.length
    pad = -nbits % 8
    acc = acc << pad | (0 if mutant == "pad_zero" else (1 << pad) - 1)
    raw = acc.to_bytes((nbits + pad) // 8, "big")
    out = raw.replace(b"\xff", b"\xff\x00")
    if mutant == "last_unstuffed" and raw.endswith(b"\xff"):
        out = out[:-1]
    return out


def encode(frame: np.ndarray, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "RGB",
           mutant: Optional[str] = None) -> bytes:
    """The whole file by the stage model."""
    h, w = frame.shape[:2]
    hs, vs = SAMPLING[subsampling] if frame.ndim == 3 else (1, 1)
    head = header(w, h, 3 if frame.ndim == 3 else 1, hs, vs, quality)
    return head + pack(symbols(scan_blocks(frame, quality, subsampling, channel_order, mutant), mutant), mutant) + b"\xff\xd9"


# ---- the case table -------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (7, 5), (8, 8), (9, 7), (16, 16), (17, 15), (24, 8), (31, 33), (40, 24)]        # (width, height)
SCAN_TILE_SIZE = (216, 200)                        # 14 x 13 MCUs of 6 blocks = 1092 blocks at 4:2:0: crosses the 1024-block scan tile
CONTENTS = ("zero", "mid", "full", "ramp", "checker", "blocks", "noise", "impulse")
QUALITIES = (1, 50, 75, 95, 100)


def content(kind: str, w: int, h: int, channels: int, seed: int = 0) -> np.ndarray:
    """(h, w, 3) or (h, w) uint8."""
    rng = np.random.default_rng([seed, w, h, channels, CONTENTS.index(kind) if kind in CONTENTS else 99])
    shape = (h, w, channels)
    y, x = np.mgrid[0:h, 0:w]
    if kind in ("zero", "mid", "full"):
        a = np.full(shape, {"zero": 0, "mid": 128, "full": 255}[kind])
    elif kind == "ramp":
        a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 255 // max(w + h - 2, 1))][:channels], -1)
    elif kind == "checker":
        a = np.repeat((((x + y) & 1) * 255)[..., None], channels, -1)
    elif kind == "blocks":
        a = np.repeat(((((x >> 3) + (y >> 3)) & 1) * 255)[..., None], channels, -1)
    elif kind == "noise":
        a = rng.integers(0, 256, shape)
    elif kind == "impulse":
        a = np.full(shape, 100)
        for _ in range(3):
            a[rng.integers(0, h), rng.integers(0, w), rng.integers(0, channels)] = rng.choice([0, 255])
    elif kind == "extreme":                        # +-1 per sample along the sign of one DCT basis function: the largest AC
        u, v = 4, 4
        basis = np.cos((2 * (x % 8) + 1) * u * np.pi / 16) * np.cos((2 * (y % 8) + 1) * v * np.pi / 16)
        a = np.repeat(((basis > 0) * 255)[..., None], channels, -1)
    elif kind == "sparse":                         # one high-frequency term on a flat field: long zero runs, then a last coefficient
        basis = np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
        a = np.repeat((128 + np.round(100 * basis))[..., None], channels, -1)
    else:
        raise ValueError(kind)
    a = a.astype(np.uint8)
    return a[..., 0] if channels == 1 else a


class Case(NamedTuple):
    name: str
    frame: np.ndarray
    quality: int
    subsampling: str
    channel_order: str

    @property
    def grey(self) -> bool:
        return self.frame.ndim == 2


def _case(kind, w, h, quality=75, subsampling="4:2:0", order="RGB", grey=False, seed=0) -> Case:
    tag = "grey" if grey else subsampling.replace(":", "") + ("_bgr" if order == "BGR" else "")
    return Case(f"{kind}_{w}x{h}_q{quality}_{tag}" + (f"_s{seed}" if seed else ""), content(kind, w, h, 1 if grey else 3, seed), quality, subsampling, order)


def cases() -> List[Case]:
    """Every size under every option with noise; every content and every quality on sizes that end inside a block, an MCU and on
    both; the frames the census needs; the scan-tile crosser; the 128 x 96 noise frame at quality 100."""
    out = []
    for w, h in SIZES:
        for sub in SAMPLING:
            out.append(_case("noise", w, h, 75, sub))
        out.append(_case("noise", w, h, 75, grey=True))
        out.append(_case("noise", w, h, 75, order="BGR"))
        out.append(_case("ramp", w, h, 95))
    for kind in CONTENTS:
        out.append(_case(kind, 17, 15, 95, "4:2:0"))
        out.append(_case(kind, 24, 8, 50, "4:2:2"))
        out.append(_case(kind, 16, 16, 100, "4:4:4"))
        out.append(_case(kind, 9, 7, 75, grey=True))
    for q in QUALITIES:
        out.append(_case("noise", 31, 33, q, "4:2:0", seed=1))
        out.append(_case("ramp", 40, 24, q, "4:2:2"))
        out.append(_case("noise", 17, 15, q, grey=True, seed=1))
    out.append(_case("blocks", 40, 24, 100, "4:4:4"))              # DC differences of category 11
    out.append(_case("extreme", 16, 16, 100, "4:4:4"))             # the largest AC coefficients 8-bit input can give
    out.append(_case("sparse", 24, 8, 95, "4:4:4"))                # runs of zeros: ZRLs
    out.append(_case("sparse", 17, 15, 50, grey=True))
    out.append(_case("noise", 8, 8, 75, "4:4:4", seed=11))         # the padded last byte is FF (found by a seed search)
    out.append(_case("noise", *SCAN_TILE_SIZE, 75, "4:2:0"))
    out.append(_case("noise", 128, 96, 100, "4:4:4"))
    return list({c.name: c for c in out}.values())                 # a frame two of the rules above ask for is listed once


def batches() -> List[List[Case]]:
    """Frames of one geometry and different contents, hence different lengths: n = 1 and n = 3."""
    three = [_case(k, 31, 33, 95, "4:2:0") for k in ("noise", "mid", "ramp")]
    return [three[:1], three]


_ORACLE = {}


def expected(case: Case) -> bytes:
    """Pillow's bytes for the case, computed once per process."""
    if case.name not in _ORACLE:
        _ORACLE[case.name] = pillow_bytes(case.frame, case.quality, case.subsampling, case.channel_order)
    return _ORACLE[case.name]
