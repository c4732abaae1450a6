"""Test-side model of hmm_jpeg_encoded_pixels' block lookup: the encoder's scan-order zigzag blocks (jpeg_encode_cases.scan_blocks,
what hmm_jpeg_encode leaves in its workspace) re-indexed into a coefficient slot of tests/jpeg_oracle.layout, which
jpeg_oracle.reconstruct turns into pixels.  ``mutant=`` breaks one index rule at a time.  Plain helper: numpy and Pillow only.

The oracle everywhere is Pillow's decode of Pillow's file, ``Image.open(BytesIO(pillow_bytes)).convert("RGB")``, and equality
is exact."""
import io

import numpy as np

import jpeg_encode_cases as ec
import jpeg_oracle

MUTANTS = ("luma_transposed", "chroma_offset_dropped", "zigzag_kept", "chroma_table0")


def geometry_of(case):
    h, w = case.frame.shape[:2]
    hs, vs = (1, 1) if case.grey else ec.SAMPLING[case.subsampling]
    return (w, h, 1 if case.grey else 3, hs, vs, 0)


def source_block(geometry, c, gx, gy, mutant=None):
    """Index in scan order of block (gx, gy) of component c's block grid."""
    w, h, ncomp, hs, vs = geometry[:5]
    mcux = -(-w // (8 * hs))
    if ncomp == 1:
        return gy * mcux + gx
    bpm = hs * vs + 2
    if c == 0:
        inside = (gx % hs) * vs + gy % vs if mutant == "luma_transposed" else (gy % vs) * hs + gx % hs
        return ((gy // vs) * mcux + gx // hs) * bpm + inside
    return (gy * mcux + gx) * bpm + (0 if mutant == "chroma_offset_dropped" else hs * vs) + (c - 1)


def slot_from_scan(blocks, geometry, quality, window, mutant=None):
    """The coefficient slot (u8 array) a decoder's entropy pass would have filled for `window`, from the scan-order blocks."""
    L = jpeg_oracle.layout(geometry, window)
    qt = ec.quant_tables(quality)
    slot = np.zeros(L["slot_bytes"], dtype=np.uint8)
    tables = slot[:384].view(np.uint16).reshape(3, 64)
    for c in range(L["ncomp"]):
        tables[c] = qt[0 if mutant == "chroma_table0" else min(c, 1)]
    coefs = slot[jpeg_oracle.QT_BYTES:jpeg_oracle.QT_BYTES + L["blocks"] * 128].view(np.int16).reshape(-1, 64)
    for c, comp in enumerate(L["comps"]):
        for by in range(comp["nby"]):
            for bx in range(comp["nbx"]):
                zz = blocks[source_block(geometry, c, comp["bx0"] + bx, comp["by0"] + by, mutant)].coefs
                dst = coefs[comp["first"] + by * comp["nbx"] + bx]
                if mutant == "zigzag_kept":
                    dst[:] = zz
                else:
                    dst[ec.ZIGZAG] = zz
    return slot


def pixels_from_scan(case, window, mutant=None):
    blocks = ec.scan_blocks(case.frame, case.quality, case.subsampling, case.channel_order)
    g = geometry_of(case)
    return jpeg_oracle.reconstruct(slot_from_scan(blocks, g, case.quality, window, mutant), g, window)


_DECODED = {}


def pillow_decoded(case) -> np.ndarray:
    """Pillow's decode of Pillow's file for the case, (h, w, 3) u8, computed once per process."""
    if case.name not in _DECODED:
        from PIL import Image
        with Image.open(io.BytesIO(ec.expected(case))) as im:
            _DECODED[case.name] = np.array(im.convert("RGB"))
    return _DECODED[case.name]


def cut(pixels: np.ndarray, window) -> np.ndarray:
    x0, y0, w, h = window
    return pixels[y0:y0 + h, x0:x0 + w]


def interior_window(w: int, h: int):
    """A window that starts on odd x and y and ends inside the frame where the frame has room for that; None for a 1-pixel side."""
    if w < 2 or h < 2:
        return None
    return (1, 1, max(w - 2, 1), max(h - 2, 1))


def max_column_sum(case) -> int:
    """The largest sum over a block column of |coefficient * quantiser| in the case's scan: what the decoder bounds by 5800."""
    blocks = ec.scan_blocks(case.frame, case.quality, case.subsampling, case.channel_order)
    qt = ec.quant_tables(case.quality)
    best = 0
    for comp, zz in blocks:
        nat = np.zeros(64, dtype=np.int64)
        nat[ec.ZIGZAG] = zz
        best = max(best, int(np.abs(nat * qt[min(comp, 1)]).reshape(8, 8).sum(axis=0).max()))
    return best
