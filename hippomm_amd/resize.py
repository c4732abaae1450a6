"""The shrink of the frames read back after retrieval (``retrieval.recall_window_frames``): OpenCV's 8-bit INTER_LINEAR for targets
no larger than the source (``hmm_resize_linear_u8``, hippomm_amd/csrc/resize.hip):

    resize_frames, resize_linear_tables   <- cv2.resize(frame, (320, 180)), hippomm/core/hippocampal_memory.py:2232, :2795
"""
from __future__ import annotations

from functools import lru_cache
from typing import Tuple

import numpy as np
import torch

from . import _lib
from .ssim import check_u8_cuda

RESIZE_COEF_SCALE = 2048                   # OpenCV's INTER_RESIZE_COEF_SCALE (11 bits)
RESIZE_LINEAR, RESIZE_AREA2X = 0, 1        # HMM_RESIZE_* of include/hippomm_hip.h


@lru_cache(maxsize=64)
def resize_linear_tables(src: int, dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """OpenCV's 8-bit INTER_LINEAR tables of one axis (resize.cpp, restated from the published source), for dst <= src:
    -> (ofs int32 [dst], coef int16 [dst][2]).  With scale = 1.0 / ((double)dst / src), output index d reads source indices s and
    s + 1, where f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s in float, with the weights (short)rint((1.f - f) * 2048)
    and (short)rint(f * 2048), rounded half to even -- a pair need not sum to 2048.  The arrays are cached per geometry and
    read-only.  An enlargement raises ``ValueError``: OpenCV's border handling decides bits there, and it is not built."""
    src, dst = int(src), int(dst)
    if not 1 <= dst <= src:
        raise ValueError(f"resize_linear_tables: {src} -> {dst}: only targets of 1..source are built (no enlargement)")
    scale = 1.0 / (dst / src)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = f - s                                                              # float32 - float32
    coef = np.stack([np.rint((np.float32(1.0) - f) * np.float32(RESIZE_COEF_SCALE)),
                     np.rint(f * np.float32(RESIZE_COEF_SCALE))], axis=1).astype(np.int16)
    ofs = s.astype(np.int32)
    ofs.setflags(write=False)
    coef.setflags(write=False)
    return ofs, coef


def resize_mode(src_hw: Tuple[int, int], dst_hw: Tuple[int, int]) -> int:
    """Which arithmetic cv2.resize(..., interpolation=INTER_LINEAR) runs for (h, w) -> (h, w): RESIZE_AREA2X when both scales are
    exactly 2 (|scale - 2| < DBL_EPSILON on both axes: OpenCV then takes its fast area path), else RESIZE_LINEAR.  An enlargement
    on either axis raises ``ValueError``."""
    (sh, sw), (dh, dw) = (tuple(int(v) for v in hw) for hw in (src_hw, dst_hw))
    if not (1 <= dh <= sh and 1 <= dw <= sw):
        raise ValueError(f"resize: {sw} x {sh} -> {dw} x {dh}: only targets no larger than the source on both axes are built "
                         "(OpenCV's border handling decides the bits of an enlargement)")
    eps = float(np.finfo(np.float64).eps)
    scale_x, scale_y = 1.0 / (dw / sw), 1.0 / (dh / sh)
    return RESIZE_AREA2X if abs(scale_x - 2) < eps and abs(scale_y - 2) < eps else RESIZE_LINEAR


@lru_cache(maxsize=32)
def _resize_tables_on(dev: torch.device, sh: int, sw: int, dh: int, dw: int):
    """The tables of a geometry in device memory, uploaded once: (xofs, xcoef, yofs, ycoef) as views of one buffer."""
    (xofs, xcoef), (yofs, ycoef) = resize_linear_tables(sw, dw), resize_linear_tables(sh, dh)
    packed = np.concatenate([a.reshape(-1).view(np.uint8) for a in (xofs, yofs, xcoef, ycoef)])
    buf = torch.from_numpy(packed).to(dev)
    x4, y4 = 4 * dw, 4 * dh
    return buf[:x4], buf[x4 + y4:x4 + y4 + x4], buf[x4:x4 + y4], buf[x4 + y4 + x4:]


def resize_frames(frames_u8: torch.Tensor, size: Tuple[int, int] = (320, 180)) -> torch.Tensor:
    """``cv2.resize(frame, size)`` (INTER_LINEAR, the default) for every frame of (n, H, W, C) uint8, C = 1 or 3, on the GPU in one
    launch -> (n, h, w, C) uint8 on the device.  ``size`` is (width, height), cv2's order (default: ``retrieval.RECALL_SIZE``).
    OpenCV's 8-bit arithmetic, restated from its published source (``resize_linear_tables``; the 2 x 2 area mean where both scales
    are exactly 2, ``resize_mode``); a build of OpenCV that routes 8-bit resize through IPP or another HAL may differ.  The target
    may not exceed the source on either axis: ``ValueError`` (enlargements are not built)."""
    f = check_u8_cuda(frames_u8, 4, "frames_u8")
    n, sh, sw, c = f.shape
    if c not in (1, 3):
        raise ValueError(f"frames_u8 must be (n, H, W, 1) or (n, H, W, 3), got {tuple(f.shape)}")
    dw, dh = (int(v) for v in size)
    mode = resize_mode((sh, sw), (dh, dw))
    out = torch.empty((n, dh, dw, c), dtype=torch.uint8, device=f.device)
    if n:
        tables = _resize_tables_on(f.device, sh, sw, dh, dw) if mode == RESIZE_LINEAR else (None,) * 4
        xofs, xcoef, yofs, ycoef = (0 if t is None else t.data_ptr() for t in tables)
        _lib.check(_lib.load().hmm_resize_linear_u8(f.data_ptr(), n, sh, sw, c, out.data_ptr(), dh, dw, xofs, xcoef, yofs, ycoef,
                                                    mode, _lib.stream_ptr()), "hmm_resize_linear_u8")
    return out
