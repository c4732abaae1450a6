"""Frame SSIM on MI355X: the gray and SSIM kernels as tensor calls, the upload of host frames, and the drop-in for the
reference's frame-difference call:

    compute_frame_difference      <- hippomm/core/batch_process.py:32-69

The SSIM is skimage 0.18.3 ``structural_similarity`` with its defaults, computed by ``hmm_ssim_pairs`` (exact integer 7x7 box sums,
fp64 formula, fixed-order mean; include/hippomm_hip.h), on gray frames made by ``hmm_gray_u8`` with OpenCV's 8-bit BGR2GRAY rule.

Host frames reach the device through one pinned staging buffer per device (``upload``, the discipline of ``_pinned``); what
follows a copy is ordered by the stream.  Deliberate deviation from the reference: ``compute_frame_difference`` takes uint8 frames
only (``TypeError`` otherwise).  There is no CPU fallback for the SSIM: without a GPU these calls raise ``HippoMMHipError``.
"""
from __future__ import annotations

import threading
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, _pinned

WIN = 7                                   # skimage's default win_size
ORDER = {"RGB": 0, "BGR": 1}              # hmm_gray_u8's channel orders (2: the frames are gray already, min / max only)


def gray_into(frames: torch.Tensor, order: int, gray: Optional[torch.Tensor], minmax: torch.Tensor) -> None:
    n, h, w = frames.shape[:3]
    _lib.check(_lib.load().hmm_gray_u8(frames.data_ptr(), n, h, w, order, 0 if gray is None else gray.data_ptr(),
                                       minmax.data_ptr(), _lib.stream_ptr()), "hmm_gray_u8")


def check_u8_cuda(t: torch.Tensor, ndim: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != ndim:
        raise TypeError(f"{what} must be a uint8 tensor with {ndim} dimensions")
    return t.to(_lib.require_gpu()).contiguous()


def gray_frames(frames_u8: torch.Tensor, channel_order: str = "RGB", return_minmax: bool = False):
    """(n, H, W, 3) uint8 frames -> (n, H, W) uint8 gray by OpenCV's 8-bit BGR2GRAY rule, g = (1868 B + 9617 G + 4899 R + 8192) >> 14,
    on the GPU.  ``channel_order`` "RGB" (Pillow) or "BGR" (OpenCV).  ``return_minmax``: also the (n, 2) int32 (min, max) per frame."""
    if channel_order not in ORDER:
        raise ValueError(f"channel_order must be 'RGB' or 'BGR', got {channel_order!r}")
    f = check_u8_cuda(frames_u8, 4, "frames_u8")
    if f.shape[3] != 3:
        raise ValueError(f"frames_u8 must be (n, H, W, 3), got {tuple(f.shape)}")
    n, h, w = f.shape[:3]
    gray = torch.empty((n, h, w), dtype=torch.uint8, device=f.device)
    minmax = torch.empty((max(n, 1), 2), dtype=torch.int32, device=f.device)
    if n:
        gray_into(f, ORDER[channel_order], gray, minmax)
    return (gray, minmax[:n]) if return_minmax else gray


def ssim_launch(gray: torch.Tensor, pairs: np.ndarray, data_range: float, minmax: Optional[torch.Tensor],
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gray (n, H, W) uint8 CUDA, pairs (m, 2) int32 host -> (m,) float64 CUDA.  data_range < 0: R of frame a from minmax.
    out: a contiguous (m,) float64 view on gray's device to write the scores into."""
    lib = _lib.load()
    (n, h, w), m = gray.shape, len(pairs)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    ws = torch.empty(max(lib.hmm_ssim_pairs_workspace_bytes(h, w, m), 256), dtype=torch.uint8, device=gray.device)
    if out is None:
        out = torch.empty(m, dtype=torch.float64, device=gray.device)
    _lib.check(lib.hmm_ssim_pairs(gray.data_ptr(), n, h, w, pairs.ctypes.data, m, float(data_range),
                                  0 if minmax is None else minmax.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _lib.stream_ptr()), "hmm_ssim_pairs")
    return out


def ssim_pairs(gray: torch.Tensor, pairs, data_range: Optional[float] = None) -> torch.Tensor:
    """SSIM of gray frames, one float64 score per pair.  gray: (n, H, W) uint8; pairs: (m, 2) integer indices (a, b), where a
    plays skimage's im1.  data_range None: R = max(a) - min(a) (what ``_compute_frame_similarity`` passes); a number: that R on the
    0..255 scale (``data_range=1.0`` on frames / 255 is 255 here).  Same scores as skimage 0.18.3 ``structural_similarity(a, b,
    data_range=R)`` to ~1e-15 relative; NaN where skimage gives NaN."""
    g = check_u8_cuda(gray, 3, "gray")
    p = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs).reshape(-1, 2)
    if len(p) == 0:
        return torch.empty(0, dtype=torch.float64, device=g.device)
    if g.shape[1] < WIN or g.shape[2] < WIN:
        raise ValueError("win_size exceeds image extent.  Either ensure that your images are at least 7x7; or pass win_size "
                         "explicitly in the function call, with an odd value less than or equal to the smaller side of your images.")
    if data_range is None:
        minmax = torch.empty((g.shape[0], 2), dtype=torch.int32, device=g.device)
        gray_into(g, 2, None, minmax)
        return ssim_launch(g, p, -1.0, minmax)
    if not data_range >= 0:
        raise ValueError(f"data_range must be >= 0, got {data_range}")
    return ssim_launch(g, p, float(data_range), None)


_stages: dict = {}                        # device -> PinnedStage of flat bytes; whoever holds _stage_lock owns the table
_stage_lock = threading.Lock()


def upload(dev, shape, fill) -> torch.Tensor:
    """``fill(host)`` writes a uint8 array of `shape`, a view of the pinned staging buffer of `dev` -> that array on the device: one
    copy on the current stream, not waited for.  Under the module's lock: wait() before ``fill``, mark() right after the copy."""
    nbytes = int(np.prod(shape))
    with _stage_lock:
        st = _pinned.stage(_stages, dev, (max(nbytes, 1 << 20),))
        st.wait()
        fill(st.host[:nbytes].reshape(shape))
        up = st.pinned[:nbytes].to(dev, non_blocking=True)
        st.mark()
    return up.view(*shape)


def upload_frames(frames: Sequence[np.ndarray], dev) -> torch.Tensor:
    """Host frames of one shape -> one (n, *shape) uint8 tensor on `dev`, through the pinned staging buffer."""
    return upload(dev, (len(frames), *frames[0].shape), lambda host: np.stack(frames, out=host))


def host_gray(frame: np.ndarray) -> np.ndarray:
    """OpenCV's 8-bit BGR2GRAY rule on the host (the reference's MSE fallback needs the gray frames there)."""
    if frame.ndim == 2:
        return frame
    b, g, r = (frame[..., c].astype(np.int32) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def check_frame(frame, name: str) -> np.ndarray:
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8:
        raise TypeError(f"{name} must be a uint8 numpy array (H, W, 3) BGR or (H, W) gray, got "
                        f"{type(frame).__name__} {getattr(frame, 'dtype', '')}")
    if not (frame.ndim == 2 or (frame.ndim == 3 and frame.shape[2] == 3)):
        raise ValueError(f"{name} must be (H, W, 3) BGR or (H, W) gray, got shape {frame.shape}")
    return frame


def _mse_fallback(frame1: np.ndarray, frame2: np.ndarray):
    """The reference's own fallback expression (batch_process.py:66-69), with whatever it returns or raises."""
    frame1_norm = host_gray(frame1).astype(float) / 255.0
    frame2_norm = host_gray(frame2).astype(float) / 255.0
    mse = np.mean((frame1_norm - frame2_norm) ** 2)
    return min(1.0, mse)


def compute_frame_difference(frame1: np.ndarray, frame2: np.ndarray) -> float:
    """Drop-in for ``batch_process.compute_frame_difference``: 1 - SSIM(gray1, gray2) with data_range 1.0 on frames / 255 (R = 255
    here), gray by OpenCV's BGR2GRAY rule.  Frames: uint8 (H, W, 3) BGR or (H, W) gray; any other dtype raises ``TypeError`` (the
    reference would hand it to cv2 / skimage), any other shape ``ValueError``.  Where the reference's SSIM raises (frames of
    different shapes, a side under 7) or is not finite, the reference's numpy MSE expression runs on the host instead, with
    whatever it then returns or raises."""
    frame1, frame2 = check_frame(frame1, "frame1"), check_frame(frame2, "frame2")
    dev = _lib.require_gpu()
    h, w = frame1.shape[:2]
    if frame2.shape[:2] != (h, w) or h < WIN or w < WIN:
        return _mse_fallback(frame1, frame2)
    n1 = frame1.size

    def both(host):                                    # two plain copies: np.concatenate(out=) measured 3-5 % slower here
        host[:n1].reshape(frame1.shape)[...] = frame1
        host[n1:].reshape(frame2.shape)[...] = frame2
    up = upload(dev, (n1 + frame2.size,), both)
    gray =torch.empty((2, h, w), dtype=torch.uint8, device=dev)
    minmax = torch.empty((1, 2), dtype=torch.int32, device=dev)
    for k, (frame, part) in enumerate(((frame1, up[:n1]), (frame2, up[n1:]))):
        if frame.ndim == 3:
            gray_into(part.view(1, h, w, 3), ORDER["BGR"], gray[k:k + 1], minmax)
        else:
            gray[k].view(-1).copy_(part)
    score = ssim_launch(gray, np.array([[0, 1]], np.int32), 255.0, None).cpu().numpy()[0]
    if np.isfinite(score):
        return 1.0 - score
    return _mse_fallback(frame1, frame2)
