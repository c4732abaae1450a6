"""numpy restatement of cv2.resize(frame, (w, h)) for 8-bit frames and targets no larger than the source, the contract of
hmm_resize_linear_u8 (include/hippomm_hip.h): OpenCV's INTER_LINEAR fixed-point path (resize.cpp: INTER_RESIZE_COEF_BITS = 11,
HResizeLinear, VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>>) and the 2 x 2 area mean OpenCV takes instead when both
scales are exactly 2.  Written from the published source, index by index and independently of the package's table code; OpenCV
itself is not a dependency of this repository."""
from __future__ import annotations

import math

import numpy as np

ONE = 2048                                             # INTER_RESIZE_COEF_SCALE


def tables(src: int, dst: int):
    """-> (ofs int64 [dst], coef int64 [dst][2]) of one axis, one output index at a time with scalar float32 arithmetic."""
    assert 1 <= dst <= src
    inv = dst / src
    scale = 1.0 / inv
    ofs, coef = np.zeros(dst, np.int64), np.zeros((dst, 2), np.int64)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = math.floor(float(f))
        f = np.float32(f - np.float32(s))
        ofs[d] = s
        coef[d, 0] = int(np.rint(np.float32(np.float32(1.0) - f) * np.float32(ONE)))      # rint: half to even
        coef[d, 1] = int(np.rint(np.float32(f * np.float32(ONE))))
    return ofs, coef


def is_area(src_hw, dst_hw) -> bool:
    eps = np.finfo(np.float64).eps
    return all(abs(1.0 / (d / s) - 2) < eps for s, d in zip(src_hw, dst_hw))


def resize(frames: np.ndarray, size) -> np.ndarray:
    """frames (n, H, W, C) uint8, size (width, height) -> (n, height, width, C) uint8."""
    n, sh, sw, c = frames.shape
    dw, dh = size
    assert dh <= sh and dw <= sw, "enlargements are not restated"
    if is_area((sh, sw), (dh, dw)):
        src = frames.astype(np.int64)
        return ((src[:, 0::2, 0::2] + src[:, 0::2, 1::2] + src[:, 1::2, 0::2] + src[:, 1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xofs, xcoef = tables(sw, dw)
    yofs, ycoef = tables(sh, dh)
    inside = xofs + 1 < sw                                                # s + 1 would leave the row: S[s] * ONE
    right = np.where(inside, xofs + 1, xofs)
    a0 = np.where(inside, xcoef[:, 0], ONE)[None, None, :, None]
    a1 = np.where(inside, xcoef[:, 1], 0)[None, None, :, None]

    def horizontal(rows):                                                 # (n, dh, W, C) source rows -> (n, dh, dw, C)
        rows = rows.astype(np.int64)
        h = rows[:, :, xofs] * a0 + rows[:, :, right] * a1
        assert h.max(initial=0) < 2 ** 31 and h.min(initial=0) >= -2 ** 31, "the int32 of the horizontal pass would overflow"
        return h

    top, bottom = horizontal(frames[:, yofs]), horizontal(frames[:, np.minimum(yofs + 1, sh - 1)])
    b0, b1 = ycoef[:, 0][None, :, None, None], ycoef[:, 1][None, :, None, None]
    out = (((b0 * (top >> 4)) >> 16) + ((b1 * (bottom >> 4)) >> 16) + 2) >> 2
    return (out & 0xFF).astype(np.uint8)                                  # the cast to uchar
