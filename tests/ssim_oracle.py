"""numpy restatement of the SSIM contract of hmm_ssim_pairs (include/hippomm_hip.h): skimage 0.18.3 structural_similarity with
its defaults on uint8 gray frames -- exact integer 7x7 box sums over the (H-6) x (W-6) window positions inside the image, then
fp64 in numpy's operation order -- and OpenCV's 8-bit BGR2GRAY rule."""
from __future__ import annotations

import numpy as np


def gray_from_bgr(frame: np.ndarray) -> np.ndarray:
    """(..., 3) uint8 B,G,R -> uint8 gray: (1868 B + 9617 G + 4899 R + 8192) >> 14."""
    b, g, r = (frame[..., c].astype(np.int64) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def box7(x: np.ndarray) -> np.ndarray:
    """Exact 7x7 sums of an integer image at the window positions inside it: (H-6, W-6) int64."""
    c = np.zeros((x.shape[0] + 1, x.shape[1] + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(x.astype(np.int64), 0), 1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim_map(a: np.ndarray, b: np.ndarray, data_range: float) -> np.ndarray:
    x, y = a.astype(np.int64), b.astype(np.int64)
    ux, uy = box7(x) / 49.0, box7(y) / 49.0
    uxx, uyy, uxy = box7(x * x) / 49.0, box7(y * y) / 49.0, box7(x * y) / 49.0
    cov_norm = 49.0 / 48.0
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = float(data_range)
    C1, C2 = (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim(a: np.ndarray, b: np.ndarray, data_range=None) -> float:
    """data_range None: max(a) - min(a), as _compute_frame_similarity passes it."""
    if data_range is None:
        data_range = int(a.max()) - int(a.min())
    return float(ssim_map(a, b, data_range).mean())
