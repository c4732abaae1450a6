"""Frame SSIM and sequence segmentation on MI355X -- drop-ins for the reference's two SSIM call sites:

    compute_frame_difference      <- hippomm/core/batch_process.py:32-69
    _compute_frame_similarity     <- hippomm/core/hippocampal_memory.py:980-991
    _segment_sequence             <- hippomm/core/hippocampal_memory.py:1002-1114 (segment_sequence: the same as a function)

and for the write of every frame the formation path keeps (the JPEG is encoded on the GPU, byte for byte Pillow's file):

    save_frame, save_frames       <- hippomm/core/batch_process.py:73-114 (cv2.imwrite)

and for the loop those two sit in, with the last saved frame, the cumulative difference and the time of the last save on the device
(``hmm_extract_walk``, hippomm_amd/csrc/extract_walk.hip: every candidate uploaded once, one read-back per batch):

    extract_frames, FrameExtractor, extraction_records   <- hippomm/core/batch_process.py:179-228

and for the shrink of the frames read back after retrieval (OpenCV's 8-bit INTER_LINEAR for targets no larger than the source,
``hmm_resize_linear_u8``, hippomm_amd/csrc/resize.hip) and the dedup walk over them (``retrieval.recall_window_frames`` strings
the steps together):

    resize_frames, resize_linear_tables   <- cv2.resize(frame, (320, 180)), hippomm/core/hippocampal_memory.py:2232, :2795
    walk_recall_window                    <- the keep / drop loop around it, :2223-2249, :2786-2812

The SSIM is skimage 0.18.3 ``structural_similarity`` with its defaults, computed by ``hmm_ssim_pairs`` (exact integer 7x7 box sums,
fp64 formula, fixed-order mean; include/hippomm_hip.h), on gray frames made by ``hmm_gray_u8`` with OpenCV's 8-bit BGR2GRAY rule.

The window walk of ``_segment_sequence`` is a pure host function of the scores (``walk_segments``).  The GPU scorer behind it
decodes a frame only when the walk first consults a pair that needs it, keeps decoded gray frames in a byte-bounded device cache
keyed by path (boundary frames are shared between windows), scores the last pair of a window on its own and, when that one does
not break, the rest of the window in one launch.  Errors -- an unreadable file, frames of different shapes, a side under 7 pixels
-- are raised only when the walk consults the pair they belong to, which is where the reference raises them.

The audio-level scan of the walk (500 ms windows from the end of a step backwards) has two routes, chosen by the caller.  Given
only the ndarray, it is the reference's numpy expression on the host, window by window (``audio_level``), and an audio-only call
needs no GPU.  Given ``audio_track=`` -- the video's ``AudioTrack``, the waveform the caller uploads once anyway to embed its
segments -- the levels of all windows of a step come from one ``AudioTrack.window_levels`` call (``hmm_audio_window_sums``: the
sum of squares per window in numpy's own summation order; mean, sqrt and log10 on the host in the track's dtype), bit for bit
the levels of the host route, so the segment list is the same.

``segment_sequence(..., walk="device")`` takes the walk itself to the device (``hmm_segment_walk``, hippomm_amd/csrc/segment_walk.hip):
every adjacent pair is scored into one device array (``PathScorer.score_adjacent``), the steps are taken there over the scores, the
frame times and the resident track, and the segment list is the one read-back.  Opt-in; ``walk="host"`` is the route above.

Deliberate deviations from the reference, all documented on the functions: ``compute_frame_difference`` takes uint8 frames only
(``TypeError`` otherwise); ``_segment_sequence`` raises ``ValueError`` where the reference would loop forever; an unreadable image
raises ``OSError`` naming the path where the reference raises ``cv2.error``.
There is no CPU fallback for the SSIM: without a GPU these calls raise ``HippoMMHipError``.
"""
from __future__ import annotations

import logging
import os
import threading
from collections import OrderedDict
from dataclasses import dataclass
from functools import lru_cache
from pathlib import Path
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, jpeg

WIN = 7                                   # skimage's default win_size
CACHE_BYTES = 512 << 20                   # device cache of gray frames (1080p: 2 MiB per frame)
UPLOAD_FRAMES = 32                        # frames per pinned staging round
ADJACENT_CHUNK = 64                       # frames per load-and-score round of PathScorer.score_adjacent

# the reference's __init__ defaults (hippocampal_memory.py:263-266)
MAX_SEGMENT_DURATION = 10.0
MIN_SEGMENT_DURATION = 5.0
FRAME_SIMILARITY_THRESHOLD = 0.95
AUDIO_SILENCE_THRESHOLD = -40


@dataclass
class SequenceSegment:
    """The fields of the reference's SequenceSegment (hippocampal_memory.py:36-42)."""
    start_time: float
    end_time: float
    frames: Optional[List[str]] = None
    audio_data: Optional[np.ndarray] = None
    frame_times: Optional[List[float]] = None


# ---------------------------------------------------------------------------------------------------------------------------------
# tensor-in kernels
# ---------------------------------------------------------------------------------------------------------------------------------
_ORDER = {"RGB": 0, "BGR": 1}


def _gray_into(frames: torch.Tensor, order: int, gray: Optional[torch.Tensor], minmax: torch.Tensor) -> None:
    n, h, w = frames.shape[:3]
    _lib.check(_lib.load().hmm_gray_u8(frames.data_ptr(), n, h, w, order, 0 if gray is None else gray.data_ptr(),
                                       minmax.data_ptr(), _lib.stream_ptr()), "hmm_gray_u8")


def _check_u8_cuda(t: torch.Tensor, ndim: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != ndim:
        raise TypeError(f"{what} must be a uint8 tensor with {ndim} dimensions")
    dev = _lib.require_gpu()
    return t.to(dev).contiguous()


def gray_frames(frames_u8: torch.Tensor, channel_order: str = "RGB", return_minmax: bool = False):
    """(n, H, W, 3) uint8 frames -> (n, H, W) uint8 gray by OpenCV's 8-bit BGR2GRAY rule,
    g = (1868 B + 9617 G + 4899 R + 8192) >> 14, on the GPU.  ``channel_order`` "RGB" (Pillow) or "BGR" (OpenCV).
    ``return_minmax``: also return the (n, 2) int32 (min, max) of each gray frame, computed in the same pass."""
    if channel_order not in _ORDER:
        raise ValueError(f"channel_order must be 'RGB' or 'BGR', got {channel_order!r}")
    f = _check_u8_cuda(frames_u8, 4, "frames_u8")
    if f.shape[3] != 3:
        raise ValueError(f"frames_u8 must be (n, H, W, 3), got {tuple(f.shape)}")
    n, h, w = f.shape[:3]
    gray = torch.empty((n, h, w), dtype=torch.uint8, device=f.device)
    minmax = torch.empty((max(n, 1), 2), dtype=torch.int32, device=f.device)
    if n:
        _gray_into(f, _ORDER[channel_order], gray, minmax)
    return (gray, minmax[:n]) if return_minmax else gray


def _ssim_launch(gray: torch.Tensor, pairs: np.ndarray, data_range: float, minmax: Optional[torch.Tensor],
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gray (n, H, W) uint8 CUDA, pairs (m, 2) int32 host -> (m,) float64 CUDA.  data_range < 0: R of frame a from minmax.
    out: a contiguous (m,) float64 view on gray's device to write the scores into."""
    lib = _lib.load()
    n, h, w = gray.shape
    m = len(pairs)
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
    g = _check_u8_cuda(gray, 3, "gray")
    p = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs).reshape(-1, 2)
    if len(p) == 0:
        return torch.empty(0, dtype=torch.float64, device=g.device)
    if g.shape[1] < WIN or g.shape[2] < WIN:
        raise ValueError("win_size exceeds image extent.  Either ensure that your images are at least 7x7; or pass win_size "
                         "explicitly in the function call, with an odd value less than or equal to the smaller side of your images.")
    if data_range is None:
        minmax = torch.empty((g.shape[0], 2), dtype=torch.int32, device=g.device)
        _gray_into(g, 2, None, minmax)
        return _ssim_launch(g, p, -1.0, minmax)
    if not data_range >= 0:
        raise ValueError(f"data_range must be >= 0, got {data_range}")
    return _ssim_launch(g, p, float(data_range), None)


# ---------------------------------------------------------------------------------------------------------------------------------
# cv2.resize(frame, (w, h)) for targets no larger than the source, and the dedup walk of a recall window
# ---------------------------------------------------------------------------------------------------------------------------------
RESIZE_COEF_SCALE = 2048                   # OpenCV's INTER_RESIZE_COEF_SCALE (11 bits)
RESIZE_LINEAR, RESIZE_AREA2X = 0, 1        # HMM_RESIZE_* of include/hippomm_hip.h
RECALL_SIZE = (320, 180)                   # (width, height) of cv2.resize at hippocampal_memory.py:2232, :2795
RECALL_SIMILARITY_CUT = 0.3                # :2238, :2801


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


def resize_frames(frames_u8: torch.Tensor, size: Tuple[int, int] = RECALL_SIZE) -> torch.Tensor:
    """``cv2.resize(frame, size)`` (INTER_LINEAR, the default) for every frame of (n, H, W, C) uint8, C = 1 or 3, on the GPU in one
    launch -> (n, h, w, C) uint8 on the device.  ``size`` is (width, height), cv2's order.  OpenCV's 8-bit arithmetic, restated
    from its published source (``resize_linear_tables``; the 2 x 2 area mean where both scales are exactly 2, ``resize_mode``); a
    build of OpenCV that routes 8-bit resize through IPP or another HAL may differ.  The target may not exceed the source on either axis:
    ``ValueError`` (enlargements are not built)."""
    f = _check_u8_cuda(frames_u8, 4, "frames_u8")
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


def walk_recall_window(scores, similarity_cut: float = RECALL_SIMILARITY_CUT) -> List[int]:
    """The dedup walk of one recall window (hippocampal_memory.py:2223-2249, :2786-2812) as a host function of the scores:
    ``scores[i][j]``, i < j, is the SSIM of frames i and j of the window with i in the im1 role; only those entries are read, and
    only the ones the walk consults.  -> the kept indices.  Frame 0 is kept; frame j is dropped iff
    ``scores[last kept][j] > similarity_cut`` -- a NaN score (a flat earlier frame) keeps the frame, as Python's comparison does
    -- and a dropped frame does not become the comparison base."""
    m = len(scores)
    kept = [0] if m else []
    for j in range(1, m):
        if not scores[kept[-1]][j] > similarity_cut:
            kept.append(j)
    return kept


# ---------------------------------------------------------------------------------------------------------------------------------
# batch_process.compute_frame_difference
# ---------------------------------------------------------------------------------------------------------------------------------
_pinned = {"buf": None}
_pinned_lock = threading.Lock()


def _pinned_bytes(nbytes: int) -> torch.Tensor:
    """A pinned host buffer of at least nbytes, reused across calls; every user synchronises before it returns."""
    buf = _pinned["buf"]
    if buf is None or buf.numel() < nbytes:
        buf = _pinned["buf"] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    return buf


def _upload_frames(frames: Sequence[np.ndarray], dev) -> torch.Tensor:
    """Host frames of one shape -> one (n, *shape) uint8 tensor on `dev`: one copy through the pinned staging buffer."""
    shape, each = frames[0].shape, frames[0].size
    with _pinned_lock:
        stage = _pinned_bytes(len(frames) * each)[:len(frames) * each]
        host = stage.numpy().reshape(len(frames), *shape)
        for k, frame in enumerate(frames):
            host[k] = frame
        up = stage.to(dev, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()                             # the staging buffer is free again
    return up.view(len(frames), *shape)


def _host_gray(frame: np.ndarray) -> np.ndarray:
    """OpenCV's 8-bit BGR2GRAY rule on the host (the reference's MSE fallback needs the gray frames there)."""
    if frame.ndim == 2:
        return frame
    b, g, r = (frame[..., c].astype(np.int32) for c in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def _check_frame(frame, name: str) -> np.ndarray:
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8:
        raise TypeError(f"{name} must be a uint8 numpy array (H, W, 3) BGR or (H, W) gray, got "
                        f"{type(frame).__name__} {getattr(frame, 'dtype', '')}")
    if not (frame.ndim == 2 or (frame.ndim == 3 and frame.shape[2] == 3)):
        raise ValueError(f"{name} must be (H, W, 3) BGR or (H, W) gray, got shape {frame.shape}")
    return frame


def _mse_fallback(frame1: np.ndarray, frame2: np.ndarray):
    """The reference's own fallback expression (batch_process.py:66-69), with whatever it returns or raises."""
    frame1_norm = _host_gray(frame1).astype(float) / 255.0
    frame2_norm = _host_gray(frame2).astype(float) / 255.0
    mse = np.mean((frame1_norm - frame2_norm) ** 2)
    return min(1.0, mse)


def compute_frame_difference(frame1: np.ndarray, frame2: np.ndarray) -> float:
    """Drop-in for ``batch_process.compute_frame_difference``: 1 - SSIM(gray1, gray2) with data_range 1.0 on frames / 255 (R = 255
    here), gray by OpenCV's BGR2GRAY rule.  Frames: uint8 (H, W, 3) BGR or (H, W) gray; any other dtype raises ``TypeError`` (the
    reference would hand it to cv2 / skimage), any other shape ``ValueError``.  Where the reference's SSIM raises (frames of
    different shapes, a side under 7) or is not finite, the reference's numpy MSE expression runs on the host instead, with
    whatever it then returns or raises."""
    frame1 = _check_frame(frame1, "frame1")
    frame2 = _check_frame(frame2, "frame2")
    dev = _lib.require_gpu()
    h, w = frame1.shape[:2]
    if frame2.shape[:2] != (h, w) or h < WIN or w < WIN:
        return _mse_fallback(frame1, frame2)
    with _pinned_lock:
        n1, n2 = frame1.size, frame2.size
        stage = _pinned_bytes(n1 + n2)
        stage[:n1].numpy().reshape(frame1.shape)[...] = frame1
        stage[n1:n1 + n2].numpy().reshape(frame2.shape)[...] = frame2
        up = stage[:n1 + n2].to(dev, non_blocking=True)
        gray = torch.empty((2, h, w), dtype=torch.uint8, device=dev)
        minmax = torch.empty((1, 2), dtype=torch.int32, device=dev)
        for k, (frame, off, nb) in enumerate(((frame1, 0, n1), (frame2, n1, n2))):
            if frame.ndim == 3:
                _lib.check(_lib.load().hmm_gray_u8(up.data_ptr() + off, 1, h, w, 1, gray[k].data_ptr(), minmax.data_ptr(),
                                                   _lib.stream_ptr()), "hmm_gray_u8")
            else:
                gray[k].view(-1).copy_(up[off:off + nb])
        score = _ssim_launch(gray, np.array([[0, 1]], np.int32), 255.0, None).cpu().numpy()[0]
    if np.isfinite(score):
        return 1.0 - score
    return _mse_fallback(frame1, frame2)


# ---------------------------------------------------------------------------------------------------------------------------------
# frames by path: decode, gray, device cache
# ---------------------------------------------------------------------------------------------------------------------------------
class _Slab:
    """Gray frames of one (H, W) in device memory, LRU over slots."""

    def __init__(self, h: int, w: int, capacity: int, dev):
        self.h, self.w, self.capacity = h, w, capacity
        self.gray = torch.empty((capacity, h, w), dtype=torch.uint8, device=dev)
        self.minmax = torch.empty((capacity, 2), dtype=torch.int32, device=dev)
        self.slots: "OrderedDict[tuple, int]" = OrderedDict()
        self.free = list(range(capacity - 1, -1, -1))

    def take(self, key) -> int:
        if not self.free:
            _, slot = self.slots.popitem(last=False)
            self.free.append(slot)
        slot = self.free.pop()
        self.slots[key] = slot
        return slot


class FrameCache:
    """Gray frames decoded from image files, on the device, keyed by (path, size, mtime); at most ``cache_bytes`` of frames per
    frame size (and always room for the frames of one launch).  Decoding runs on the package's decode thread pool and goes
    through pinned staging; the gray kernel writes the frame's min and max alongside (the data range of
    ``_compute_frame_similarity``)."""

    def __init__(self, cache_bytes: int = CACHE_BYTES):
        self.cache_bytes = cache_bytes
        self.slabs = {}
        self.decodes = 0
        self.device_decodes = 0                        # of them, frames the JPEG device route decoded
        self.lock = threading.Lock()

    @staticmethod
    def key(path):
        st = os.stat(path)
        return (str(path), st.st_size, st.st_mtime_ns)

    def _slab(self, h: int, w: int, need: int, dev) -> _Slab:
        slab = self.slabs.get((h, w))
        if slab is None or slab.capacity < need:
            grown = _Slab(h, w, max(need, self.cache_bytes // max(h * w, 1), 4), dev)
            if slab is not None:                       # more frames in one call than the budget holds: keep every slot
                grown.gray[:slab.capacity].copy_(slab.gray)
                grown.minmax[:slab.capacity].copy_(slab.minmax)
                grown.slots = slab.slots
                grown.free = list(range(grown.capacity - 1, slab.capacity - 1, -1)) + slab.free
            slab = self.slabs[(h, w)] = grown
        return slab

    def lookup(self, path):
        """-> (slab, slot) of a cached frame, or None."""
        try:
            k = self.key(path)
        except OSError:
            return None
        for slab in self.slabs.values():
            slot = slab.slots.get(k)
            if slot is not None:
                slab.slots.move_to_end(k)
                return slab, slot
        return None

    def _store(self, h: int, w: int, keys: Sequence[tuple], up: torch.Tensor, dev, protect: int = 0) -> Tuple[_Slab, List[int]]:
        """Frames (n, h, w, 3) u8 RGB `up` on `dev` -> gray + min / max into n slots of the slab of that size, under `keys`.
        protect: slots of that slab the caller still needs (they are the most recently used: the n new ones do not evict them)."""
        slab = self._slab(h, w, protect + len(keys), dev)
        gray = torch.empty((len(keys), h, w), dtype=torch.uint8, device=dev)
        minmax = torch.empty((len(keys), 2), dtype=torch.int32, device=dev)
        _gray_into(up, 0, gray, minmax)
        slots = [slab.take(k) for k in keys]
        idx = torch.tensor(slots, dtype=torch.int64).to(dev)
        slab.gray.index_copy_(0, idx, gray)
        slab.minmax.index_copy_(0, idx, minmax)
        return slab, slots

    def put(self, path, rgb: torch.Tensor) -> None:
        """Insert the decoded frame(s) of file(s) that exist: path and an (h, w, 3) uint8 RGB tensor on the device -- what
        ``load`` would decode from the file, e.g. ``encode_jpeg(..., return_decoded=True)``'s pixels of the file just written -- or
        a list of paths and an (n, h, w, 3) tensor.  Gray and min / max go under ``key(path)`` of the file as it is now, by the
        same kernel and into the same slabs as ``load``, with its eviction rules (least recently used first; the frames of one
        call never evict each other).  ``decodes`` does not move.  An entry of the same path under an older key (the file has
        been rewritten since) is simply never hit again."""
        paths = [path] if isinstance(path, (str, os.PathLike)) else list(path)
        frames = rgb[None] if rgb.dim() == 3 else rgb
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] != len(paths):
            raise ValueError(f"FrameCache.put takes (h, w, 3) uint8 RGB per path, got {tuple(rgb.shape)} {rgb.dtype} for {len(paths)} paths")
        keys = [self.key(p) for p in paths]
        n, h, w = frames.shape[:3]
        with self.lock:
            for slab in self.slabs.values():           # a path put twice keeps one slot
                for k in keys:
                    slot = slab.slots.pop(k, None)
                    if slot is not None:
                        slab.free.append(slot)
            self._store(h, w, keys, frames.contiguous(), frames.device)

    def load(self, paths: Sequence[str], dev) -> dict:
        """Decode the paths that are not cached; -> {path: (slab, slot) or the exception its decode raised}.  The frames of one
        call are never evicted by that call."""
        from . import preprocess as pp
        out, todo = {}, []
        for p in dict.fromkeys(paths):
            hit = self.lookup(p)
            if hit is None:
                todo.append(p)
            else:
                out[p] = hit
        lib = _lib.load()

        def read_one(path):
            try:
                k = self.key(path)
                with open(path, "rb") as fh:
                    return k, fh.read()
            except Exception as exc:                   # noqa: BLE001 - raised later, when the walk consults this frame
                return None, OSError(f"cannot read image file {path!r}: {exc}")

        def open_one(item):
            path, data = item
            try:
                return pp._open_rgb_bytes(data)
            except Exception as exc:                   # noqa: BLE001 - raised later, when the walk consults this frame
                return OSError(f"cannot read image file {path!r}: {exc}")

        def store(h, w, items, up):
            """items [(path, key)] of frames (n, h, w, 3) u8 `up` on the device -> gray + min / max into the slab."""
            protect = sum(1 for v in out.values() if isinstance(v, tuple) and v[0].h == h and v[0].w == w)
            slab, slots = self._store(h, w, [k for _, k in items], up, dev, protect)
            for (p, _), slot in zip(items, slots):
                out[p] = (slab, slot)

        workers = pp.decode_workers()
        for c0 in range(0, len(todo), UPLOAD_FRAMES):
            chunk = todo[c0:c0 + UPLOAD_FRAMES]
            read = list(pp._decode_pool(workers).map(read_one, chunk)) if len(chunk) > 1 else [read_one(chunk[0])]
            self.decodes += len(chunk)
            on_host = []
            # the JPEG device route (hippomm_amd/jpeg.py) for the files it takes; Pillow for the rest, as before
            jpegs = [(p, k, data) for p, (k, data) in zip(chunk, read) if k is not None and jpeg.takes(jpeg.parse(data))]
            if jpegs and jpeg.route_ok(jpegs[0][2], dev):
                frames, errors, n_dev = jpeg._decode_many([d for _, _, d in jpegs], dev)
                self.device_decodes += n_dev
                sizes = {}
                for (p, k, _), frame, exc in zip(jpegs, frames, errors):
                    if exc is not None:
                        out[p] = OSError(f"cannot read image file {p!r}: {exc}")
                    else:
                        sizes.setdefault((frame.shape[0], frame.shape[1]), []).append((p, k, frame))
                for (h, w), items in sizes.items():
                    store(h, w, [(p, k) for p, k, _ in items], torch.stack([f for _, _, f in items]))
                taken = {p for p, _, _ in jpegs}
            else:
                taken = set()
            for p, (k, data) in zip(chunk, read):
                if k is None:
                    out[p] = data
                elif p not in taken:
                    on_host.append((p, k, data))
            opened = list(pp._decode_pool(workers).map(open_one, [(p, d) for p, _, d in on_host])) if len(on_host) > 1 else \
                [open_one((p, d)) for p, _, d in on_host]
            groups = {}
            for (p, k, _), im in zip(on_host, opened):
                if isinstance(im, Exception):
                    out[p] = im
                else:
                    groups.setdefault((im.size[1], im.size[0]), []).append((p, k, im))
            for (h, w), items in groups.items():
                with _pinned_lock:
                    stage = _pinned_bytes(len(items) * h * w * 3)[:len(items) * h * w * 3].view(len(items), h, w, 3)
                    arrs = stage.numpy()
                    list(pp._decode_pool(workers).map(lambda it: pp._pack_into(it[1][2], arrs[it[0]], lib), enumerate(items)))
                    store(h, w, [(p, k) for p, k, _ in items], stage.to(dev, non_blocking=True))
                    torch.cuda.current_stream().synchronize()      # the staging buffer is free again
        return out


_default_cache = None


def default_cache() -> FrameCache:
    global _default_cache
    if _default_cache is None:
        _default_cache = FrameCache()
    return _default_cache


_SHAPE_MSG = "Input images must have the same dimensions."
_EXTENT_MSG = "win_size exceeds image extent."


class PathScorer:
    """SSIM of (later, earlier) image-file pairs as ``_compute_frame_similarity`` computes it (R from the first frame), with the
    errors of a pair raised only when its score is asked for.  ``pairs_scored`` counts the pairs sent to the GPU."""

    def __init__(self, cache: Optional[FrameCache] = None):
        self.cache = cache if cache is not None else default_cache()
        self.pairs_scored = 0
        self.dev = _lib.require_gpu()

    def _problem(self, loaded: dict, p1: str, p2: str) -> Optional[Exception]:
        for p in (p1, p2):
            if isinstance(loaded[p], Exception):
                return loaded[p]
        (s1, _), (s2, _) = loaded[p1], loaded[p2]
        if (s1.h, s1.w) != (s2.h, s2.w):
            return ValueError(f"{_SHAPE_MSG} {p1!r} is {s1.h}x{s1.w}, {p2!r} is {s2.h}x{s2.w}")
        if s1.h < WIN or s1.w < WIN:
            return ValueError(f"{_EXTENT_MSG} {p1!r} and {p2!r} are {s1.h}x{s1.w}; the window is {WIN}x{WIN}")
        return None

    def score(self, pairs: Sequence[Tuple[str, str]]) -> Iterable[float]:
        """Yield the scores of the pairs in order; raise a pair's error when its turn comes.  Every pair before the first
        problem is scored in one launch per frame size (one in practice)."""
        with self.cache.lock:
            loaded = self.cache.load([p for pair in pairs for p in pair], self.dev)
            good, err = [], None
            for p1, p2 in pairs:
                err = self._problem(loaded, p1, p2)
                if err is not None:
                    break
                good.append((p1, p2))
            scores = np.empty(0)
            if good:
                first = loaded[good[0][0]][0]
                slab = self.cache.slabs[(first.h, first.w)]    # the current slab of that size (it may have grown meanwhile)
                idx = np.array([[loaded[p1][1], loaded[p2][1]] for p1, p2 in good], dtype=np.int32)
                scores = _ssim_launch(slab.gray, idx, -1.0, slab.minmax).cpu().numpy()
                self.pairs_scored += len(good)
        yield from (np.float64(s) for s in scores)
        if err is not None:
            raise err

    def score_adjacent(self, video_frames: Sequence[str], chunk: int = ADJACENT_CHUNK) -> Tuple[torch.Tensor, List[Optional[Exception]]]:
        """Every pair the walk of ``_segment_sequence`` can consult, scored without a read-back: -> (scores_dev, problems).
        scores_dev: float64 [n - 1] on the device, scores_dev[i] the SSIM of (video_frames[i + 1], video_frames[i]) -- the later
        frame in the im1 role, as ``score`` has it.  problems[i]: the exception ``score`` would raise for pair i, or None; such a
        pair is not scored (its entry stays NaN) and it is the caller's to flag (``hmm_segment_walk`` takes the flags), so that
        the error is raised only if the walk consults the pair.  Frames go through the cache ``chunk`` at a time, the last frame
        of a chunk staying for the first pair of the next; one ``hmm_ssim_pairs`` launch per chunk and frame size.

        This decodes every frame, where the host walk decodes only the frames of pairs it consults (539 of 600 on the "cuts"
        video of DESIGN.md section 11): the price of taking the walk off the host when the frames are not cached already."""
        n = len(video_frames)
        scores = torch.full((max(n - 1, 0),), float("nan"), dtype=torch.float64, device=self.dev)
        problems: List[Optional[Exception]] = [None] * max(n - 1, 0)
        chunk = max(int(chunk), 1)
        with self.cache.lock:
            for c0 in range(1, n, chunk):                       # frames c0 - 1 .. c1 - 1: pairs c0 - 1 .. c1 - 2
                c1 = min(c0 + chunk, n)
                paths = list(video_frames[c0 - 1:c1])
                loaded = self.cache.load(paths, self.dev)
                sizes = {}
                for i in range(c0 - 1, c1 - 1):
                    later, earlier = paths[i + 1 - (c0 - 1)], paths[i - (c0 - 1)]
                    problems[i] = self._problem(loaded, later, earlier)
                    if problems[i] is None:
                        slab = loaded[later][0]
                        sizes.setdefault((slab.h, slab.w), []).append((i, loaded[later][1], loaded[earlier][1]))
                for size, items in sizes.items():
                    slab = self.cache.slabs[size]               # the current slab of that size (it may have grown meanwhile)
                    idx = np.array([[a, b] for _, a, b in items], dtype=np.int32)
                    first, m = items[0][0], len(items)
                    if items[-1][0] - first + 1 == m:           # one run of pairs: straight into the array
                        _ssim_launch(slab.gray, idx, -1.0, slab.minmax, out=scores[first:first + m])
                    else:
                        where = torch.tensor([i for i, _, _ in items], dtype=torch.int64).to(self.dev)
                        scores.index_copy_(0, where, _ssim_launch(slab.gray, idx, -1.0, slab.minmax))
                    self.pairs_scored += m
        return scores, problems


def _compute_frame_similarity(self, frame1_path: str, frame2_path: str) -> float:
    """Drop-in for ``HippocampalMemory._compute_frame_similarity`` (assign it on the class; ``self`` is unused): SSIM of the two
    files' gray frames with data_range = max - min of the first.  Pillow decodes (the reference uses cv2.imread); an unreadable
    file raises ``OSError`` naming its path, frames of different shapes or under 7x7 raise ``ValueError`` as skimage does."""
    return next(iter(PathScorer().score([(frame1_path, frame2_path)])))


# ---------------------------------------------------------------------------------------------------------------------------------
# HippocampalMemory._segment_sequence
# ---------------------------------------------------------------------------------------------------------------------------------
def audio_level(audio_data: np.ndarray, sample_rate: int):
    """RMS level in dB with the reference's numpy expression (hippocampal_memory.py:993-1000), so levels are bit-identical."""
    if len(audio_data.shape) > 1:
        audio_data = audio_data.mean(axis=1)
    rms = np.sqrt(np.mean(np.square(audio_data)))
    return 20 * np.log10(rms) if rms > 0 else -100


def walk_segments(video_frames, frame_times, audio_data, audio_sample_rate,
                  score_window: Callable[[List[Tuple[int, int]]], Iterable[float]],
                  max_segment_duration: float = MAX_SEGMENT_DURATION, min_segment_duration: float = MIN_SEGMENT_DURATION,
                  frame_similarity_threshold: float = FRAME_SIMILARITY_THRESHOLD,
                  audio_silence_threshold: float = AUDIO_SILENCE_THRESHOLD, *, audio_track=None) -> List[SequenceSegment]:
    """The window walk of ``_segment_sequence`` as a host function of the scores.  ``score_window(pairs)`` gets one window's pairs
    of frame indices (later, earlier) -- adjacent entries of the window's frame list, scanned from the end -- and yields their
    similarities in that order; the walk stops reading at the first score below the threshold (NaN never breaks).

    Behaviour of the reference kept: the walk starts at 0.0 whatever frame_times[0] is; a frame is in a window when
    start <= t <= end; the audio scan (500 ms windows, from the end backwards, excluding offset 0) runs after the video scan and
    overrides it; then the minimum-duration clamp; segment contents take inclusive time bounds and audio samples
    int(start * sr):int(end * sr).  One deviation: where the reference would loop forever (a start it has already been at, which
    only happens with min_segment_duration <= 0), this raises ValueError.

    ``audio_track`` (an ``audio_track.AudioTrack`` of the same waveform): the levels of a step's windows come from one
    ``window_level_values`` call over all of the step's window starts instead of one host expression per window -- the same
    objects, so the same segments; the level is a pure function of the window, and the first window from the end below the
    threshold still decides.  Its rate must be ``audio_sample_rate`` (ValueError).  ``audio_data`` may then be None: the track's
    length stands in for ``len(audio_data)`` and ``seg.audio_data`` is None (form spans with ``audio_track.spans_of``)."""
    segments: List[SequenceSegment] = []
    if audio_track is not None:
        if audio_track.sample_rate != audio_sample_rate:
            raise ValueError(f"audio_track is at {audio_track.sample_rate} Hz, audio_sample_rate is {audio_sample_rate}")
        if audio_data is not None and len(audio_data) != audio_track.n_samples:
            raise ValueError(f"audio_track holds {audio_track.n_samples} samples, audio_data {len(audio_data)}")
    if video_frames is None and audio_data is None and audio_track is None:
        return segments
    has_video = bool(video_frames and frame_times)
    has_audio = (audio_data is not None or audio_track is not None) and bool(audio_sample_rate)
    if has_video:
        total_duration = frame_times[-1] - frame_times[0]
    elif has_audio:
        total_duration = (len(audio_data) if audio_data is not None else audio_track.n_samples) / audio_sample_rate
    else:
        return segments

    current_start = 0.0
    seen = set()
    while current_start < total_duration:
        if current_start in seen:
            raise ValueError(f"segmentation makes no progress at t = {current_start} (min_segment_duration = "
                             f"{min_segment_duration}); the reference would loop forever here")
        seen.add(current_start)
        current_end = min(current_start + max_segment_duration, total_duration)
        optimal_end = current_end

        if has_video:
            inside = [i for i, t in enumerate(frame_times) if current_start <= t <= current_end]
            if len(inside) > 1:
                pairs = [(inside[k], inside[k - 1]) for k in range(len(inside) - 1, 0, -1)]
                for (later, _), similarity in zip(pairs, score_window(pairs)):
                    if similarity < frame_similarity_threshold:
                        optimal_end = frame_times[later]
                        break

        if has_audio:
            start_sample = int(current_start * audio_sample_rate)
            end_sample = int(current_end * audio_sample_rate)
            window = int(0.5 * audio_sample_rate)
            if audio_track is not None:                      # every window of this step in one launch
                starts = [start_sample + off for off in range(end_sample - start_sample - window, 0, -window)]
                resident = dict(zip(starts, audio_track.window_level_values(starts, window)))
            for off in range(end_sample - start_sample - window, 0, -window):
                lo = start_sample + off
                level = resident[lo] if audio_track is not None else audio_level(audio_data[lo:lo + window], audio_sample_rate)
                if level < audio_silence_threshold:
                    optimal_end = lo / audio_sample_rate
                    break

        if optimal_end - current_start < min_segment_duration:
            optimal_end = min(current_start + min_segment_duration, total_duration)

        seg = SequenceSegment(start_time=current_start, end_time=optimal_end)
        if has_video:
            seg.frames = [f for f, t in zip(video_frames, frame_times) if current_start <= t <= optimal_end]
            seg.frame_times = [t for t in frame_times if current_start <= t <= optimal_end]
        if has_audio and audio_data is not None:
            seg.audio_data = audio_data[int(current_start * audio_sample_rate):int(optimal_end * audio_sample_rate)]
        segments.append(seg)
        current_start = optimal_end
    return segments


def _window_scorer(video_frames, scorer: PathScorer):
    """score_window for walk_segments on the GPU: the window's last pair alone first (at threshold 0.95 it usually breaks), then,
    if it did not, the rest of the window in one launch."""
    def score_window(pairs):
        paths = [(video_frames[a], video_frames[b]) for a, b in pairs]
        yield from scorer.score(paths[:1])
        if len(paths) > 1:
            yield from scorer.score(paths[1:])
    return score_window


# hmm_segment_record and hmm_segment_walk_state of include/hippomm_hip.h
SEGMENT_RECORD = np.dtype([("start_time", "<f8"), ("end_time", "<f8"), ("first_frame", "<i4"), ("last_frame", "<i4"),
                           ("cut_pair", "<i4"), ("cut_window", "<i4"), ("pairs_consulted", "<i4"), ("windows_consulted", "<i4")])
SEGMENT_STATE = np.dtype([("n_segments", "<i4"), ("status", "<i4"), ("flagged_pair", "<i4"), ("steps", "<i4"),
                          ("current_start", "<f8")])
WALK_DONE, WALK_FLAGGED, WALK_BOUND = 1, 2, 3       # HMM_SEGMENT_WALK_*
MAX_DEVICE_STEPS = 4096                             # two launches per step with audio: beyond this the host walks
MAX_DEVICE_WINDOWS = 65535                          # windows of one step (one workgroup each)


def _silent_on_host(rms, threshold) -> bool:
    """The host route's decision for a window whose rms is the numpy scalar `rms`: ``audio_level``'s last line, then the walk's
    comparison, with the very objects the host route compares."""
    with np.errstate(all="ignore"):
        return bool((20 * np.log10(rms) if rms > 0 else -100) < threshold)


@lru_cache(maxsize=64)
def _silence_cut(dtype_name: str, threshold, _threshold_type) -> Tuple[float, bool]:
    T = np.dtype(dtype_name).type
    U = np.uint32 if T is np.float32 else np.uint64
    value = lambda bits: U(bits).view(T)                                      # noqa: E731
    lo, hi = 1, int(T(np.inf).view(U))                                        # positive floats in the order of their bit patterns
    if _silent_on_host(value(hi), threshold):
        raise AssertionError(f"silence_cut: an infinite rms is silent under threshold {threshold!r}")
    while lo < hi:                                                            # the least pattern that is not silent
        mid = (lo + hi) // 2
        if _silent_on_host(value(mid), threshold):
            lo = mid + 1
        else:
            hi = mid
    cut = value(lo)
    if _silent_on_host(cut, threshold) or (lo > 1 and not _silent_on_host(value(lo - 1), threshold)):
        raise AssertionError(f"silence_cut: the level is not monotonic around rms = {cut!r} for threshold {threshold!r}")
    return float(cut), bool(-100 < threshold)


def silence_cut(dtype, threshold) -> Tuple[float, bool]:
    """The silence rule of the walk without a logarithm: -> (rms_cut, silent_without_rms) such that, for an rms of `dtype`
    (float32 or float64), ``(20 * np.log10(rms) if rms > 0 else -100) < threshold`` is ``rms < rms_cut if rms > 0 else
    silent_without_rms``.  rms_cut is found by bisection over the bit patterns of the positive floats with this host's own scalar
    expression, and checked: the float below it is silent, it is not (``AssertionError`` otherwise -- a log10 that is not
    monotonic there).  Cached per (dtype, threshold)."""
    return _silence_cut(np.dtype(dtype).name, threshold, type(threshold))


def _device_walk(video_frames, frame_times, audio_data, audio_sample_rate, max_segment_duration, min_segment_duration,
                 frame_similarity_threshold, audio_silence_threshold, scorer, audio_track, stats: dict):
    """The walk by ``hmm_segment_walk`` -> the segments, or a str: why this call stays on the host route."""
    has_video = bool(video_frames and frame_times)
    has_audio = (audio_data is not None or audio_track is not None) and bool(audio_sample_rate)
    if not has_video and not has_audio:
        return "nothing to segment"
    if has_audio and audio_track is None:
        raise ValueError("walk='device' needs the video's AudioTrack (audio_track=) when there is audio")
    params = (max_segment_duration, min_segment_duration, frame_similarity_threshold, audio_silence_threshold)
    if any(p != p for p in params) or not all(np.isfinite(p) for p in params[:2]):
        return "NaN parameters"
    if not min_segment_duration > 0:
        return "min_segment_duration <= 0"
    times = np.empty(0)
    if has_video:
        if len(video_frames) != len(frame_times) or not all(isinstance(t, float) for t in frame_times):
            return "frame_times are not one float per frame"
        times = np.asarray(frame_times, dtype=np.float64)
        if not np.all(np.isfinite(times)) or np.any(times[1:] < times[:-1]):
            return "unsorted frame_times"
        total = frame_times[-1] - frame_times[0]
    rate = 0
    if has_audio:
        if audio_track.sample_rate != audio_sample_rate or (audio_data is not None and len(audio_data) != audio_track.n_samples):
            return "audio_track does not match the call"                       # the host route raises the ValueError
        if audio_track.source_dtype not in (np.float32, np.float64):
            return "track not float32 / float64 at its source"
        rate = int(audio_sample_rate)
        if rate != audio_sample_rate or rate < 2:
            return "sample rate not an integer >= 2"
        if not has_video:
            total = audio_track.n_samples / audio_sample_rate
    if not np.isfinite(total) or (has_audio and not total * rate < 2.0 ** 52):
        return "duration out of range"
    span = min(max_segment_duration, max(total, 0.0))                          # no step is longer, up to rounding
    window = int(0.5 * rate)
    if has_audio and getattr(audio_track, "pcm", False) and window > (1 << 22):
        return "a window above 2^22 samples on a 16-bit track"
    if not total / min_segment_duration < MAX_DEVICE_STEPS or (has_audio and not span * rate / window < MAX_DEVICE_WINDOWS):
        return "more steps or windows than the device route launches"
    max_steps = max(int(np.ceil(total / min_segment_duration)), 0) + 2         # a clamped step advances by min, or reaches the end
    max_windows = int((span * rate + 2) // window) + 1 if has_audio else 0

    lib = _lib.load()
    dev = audio_track.device if has_audio else scorer.dev
    rms_cut, silent_without_rms = silence_cut(np.float64 if audio_track.dtype_code else np.float32,
                                              audio_silence_threshold) if has_audio else (0.0, False)
    problems: List[Optional[Exception]] = []
    scores = flags = times_dev = None
    with torch.cuda.device(dev):
        if has_video:
            scores, problems = scorer.score_adjacent(video_frames)
            scores = scores.to(dev)
            flags = torch.tensor([p is not None for p in problems], dtype=torch.int32).to(dev)
            times_dev = torch.from_numpy(times).to(dev)
        ws = torch.empty(max(lib.hmm_segment_walk_workspace_bytes(max_windows, max_steps), 256), dtype=torch.uint8, device=dev)
        out = torch.empty(max_steps * SEGMENT_RECORD.itemsize + SEGMENT_STATE.itemsize, dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None   # noqa: E731
        head = (ptr(scores), ptr(flags), ptr(times_dev), times.ctypes.data if has_video else None, len(times),
                audio_track.samples.data_ptr() if has_audio else None)
        rest = (audio_track.n_samples if has_audio else 0, rate, float(total), float(max_segment_duration), float(min_segment_duration),
                float(frame_similarity_threshold), rms_cut, int(silent_without_rms), max_windows, max_steps, out.data_ptr(),
                out.data_ptr() + max_steps * SEGMENT_RECORD.itemsize, ws.data_ptr(), ws.numel(), _lib.stream_ptr())
        if has_audio and getattr(audio_track, "pcm", False):                   # int16 samples: the entry point without a track_dtype
            _lib.check(lib.hmm_segment_walk_pcm16(*head, *rest), "hmm_segment_walk_pcm16")
        else:
            _lib.check(lib.hmm_segment_walk(*head, audio_track.dtype_code if has_audio else 0, *rest), "hmm_segment_walk")
        host = out.cpu().numpy()                                               # the one read-back
    state = host[max_steps * SEGMENT_RECORD.itemsize:].view(SEGMENT_STATE)[0]
    records = host[:int(state["n_segments"]) * SEGMENT_RECORD.itemsize].view(SEGMENT_RECORD)
    stats.update(steps=int(state["steps"]), launches=2 * max_steps + 1 if has_audio else 1, read_backs=1,
                 pairs_scored=len(problems) - sum(p is not None for p in problems),
                 pairs_consulted=int(records["pairs_consulted"].sum()), windows_consulted=int(records["windows_consulted"].sum()))
    if state["status"] == WALK_FLAGGED:
        raise problems[int(state["flagged_pair"])]
    if state["status"] != WALK_DONE:
        return "step bound exhausted"
    segments = []
    for rec in records:
        start, end = float(rec["start_time"]), float(rec["end_time"])
        seg = SequenceSegment(start_time=start, end_time=end)
        if has_video:                                                          # the frames with start <= t <= end: one index range
            inside = slice(int(rec["first_frame"]), int(rec["last_frame"]) + 1)
            seg.frames = list(video_frames[inside])
            seg.frame_times = list(frame_times[inside])
        if has_audio and audio_data is not None:
            seg.audio_data = audio_data[int(start * audio_sample_rate):int(end * audio_sample_rate)]
        segments.append(seg)
    return segments


def segment_sequence(video_frames: Optional[List[str]] = None, frame_times: Optional[List[float]] = None,
                     audio_data: Optional[np.ndarray] = None, audio_sample_rate: Optional[int] = None, *,
                     max_segment_duration: float = MAX_SEGMENT_DURATION, min_segment_duration: float = MIN_SEGMENT_DURATION,
                     frame_similarity_threshold: float = FRAME_SIMILARITY_THRESHOLD,
                     audio_silence_threshold: float = AUDIO_SILENCE_THRESHOLD,
                     scorer: Optional[PathScorer] = None, audio_track=None, walk: str = "host",
                     stats: Optional[dict] = None) -> List[SequenceSegment]:
    """``_segment_sequence`` as a function; the four parameters default to the reference's __init__ defaults.  Frame similarities
    come from the GPU (``PathScorer``).  Without ``audio_track`` an audio-only call needs no GPU (the audio scan is host numpy,
    as in the reference); with the video's ``AudioTrack`` the scan reads the resident track (see ``walk_segments``).

    ``walk="device"`` (opt-in; "host" is the default and is the route above, untouched) takes the control loop to the device as
    well: every adjacent pair is scored into one device array (``PathScorer.score_adjacent``), ``hmm_segment_walk`` walks it and
    the resident track, and the segment list is the one read-back -- the same segments: times equal as floats, the same frame
    lists, the same audio slices (times come back as Python floats; the frames of a segment are taken as one index range, which
    is what the reference's comprehension selects when the times are sorted).  It needs the video's ``audio_track`` when there
    is audio (``ValueError``).  It scores every pair, the host route only the consulted ones: with frames that are not in the
    cache yet it decodes them all.  A pair that cannot be scored raises its error only if the walk consults it, as on the host
    route.  Calls it does not take go the host route and say why in ``stats["reason"]``: unsorted or non-float frame_times, NaN
    parameters, min_segment_duration <= 0, a track that was not float32 / float64 at its source (a 16-bit track of
    ``AudioTrack.from_wav`` / ``from_pcm16`` stands for a float64 array and is walked by ``hmm_segment_walk_pcm16``), more steps than
    MAX_DEVICE_STEPS, a walk that did not finish within its step bound.  Measured on one MI355X with every input resident (600
    cached 1080p frames, a 600 s float64 track at 16 kHz, 80 segments; profiles/segment_walk.json): 9.4 ms
    against 31.3 ms for the host walk, 1 read-back against 226; uncached frames and other inputs were not measured.

    ``stats``: a dict that receives ``route`` ("host" / "device") and, from the device walk, ``steps``, ``launches``,
    ``read_backs``, ``pairs_scored``, ``pairs_consulted``, ``windows_consulted``; ``reason`` when a device call went to the host."""
    if walk not in ("host", "device"):
        raise ValueError(f"walk must be 'host' or 'device', got {walk!r}")
    stats = {} if stats is None else stats
    if video_frames and frame_times and scorer is None:
        scorer = PathScorer()
    if walk == "device":
        done = _device_walk(video_frames, frame_times, audio_data, audio_sample_rate, max_segment_duration, min_segment_duration,
                            frame_similarity_threshold, audio_silence_threshold, scorer, audio_track, stats)
        if not isinstance(done, str):
            stats["route"] = "device"
            return done
        stats["reason"] = done
    stats["route"] = "host"
    score_window = _window_scorer(video_frames, scorer) if scorer is not None else None
    return walk_segments(video_frames, frame_times, audio_data, audio_sample_rate, score_window,
                         max_segment_duration, min_segment_duration, frame_similarity_threshold, audio_silence_threshold,
                         audio_track=audio_track)


def _segment_sequence(self, video_frames: Optional[List[str]] = None, frame_times: Optional[List[float]] = None,
                      audio_data: Optional[np.ndarray] = None, audio_sample_rate: Optional[int] = None,
                      audio_track=None) -> List[SequenceSegment]:
    """Drop-in for ``HippocampalMemory._segment_sequence`` (assign it on the class): reads self.max_segment_duration,
    self.min_segment_duration, self.frame_similarity_threshold and self.audio_silence_threshold.  The video's ``AudioTrack``,
    given as the ``audio_track`` argument or set as ``self.audio_track``, moves the audio-level scan to the device;
    ``self.segment_walk = "device"`` moves the walk itself there (``segment_sequence``'s ``walk``; "host" when not set)."""
    if audio_track is None:
        audio_track = getattr(self, "audio_track", None)
    return segment_sequence(video_frames, frame_times, audio_data, audio_sample_rate,
                            max_segment_duration=self.max_segment_duration, min_segment_duration=self.min_segment_duration,
                            frame_similarity_threshold=self.frame_similarity_threshold,
                            audio_silence_threshold=self.audio_silence_threshold, audio_track=audio_track,
                            walk=getattr(self, "segment_walk", "host"))


# ---------------------------------------------------------------------------------------------------------------------------------
# frames to disk: the write of extract_frames_from_video
# ---------------------------------------------------------------------------------------------------------------------------------
SAVE_QUALITY, SAVE_SUBSAMPLING = 95, "4:2:0"       # libjpeg's defaults under cv2.imwrite (recalled, not checkable here)
_save_log = logging.getLogger(__name__)


def _encode_bgr(frames, **decoded):
    """-> the files; with return_decoded=True (and window=), (files, their decoded RGB pixels on the device)."""
    return jpeg.encode_jpeg(frames, quality=SAVE_QUALITY, subsampling=SAVE_SUBSAMPLING, channel_order="BGR", **decoded)


def _fill_caches(written, cache, tower_inputs) -> None:
    """written: (path, the decoded RGB of the file just written -- the whole frame, or its needed_window when only the tower
    asks --, the frame's (h, w)).  One gray launch and one preprocess launch per frame size."""
    from . import preprocess as pp
    groups = {}
    for path, rgb, hw in written:
        groups.setdefault((tuple(rgb.shape), hw), []).append((path, rgb))
    for (shape, hw), items in groups.items():
        paths = [str(p) for p, _ in items]
        frames = torch.stack([f for _, f in items])
        if cache is not None:
            cache.put(paths, frames)
        if tower_inputs is not None:
            if shape[:2] == hw:                          # whole frames: the tower's taps touch this window of them
                x0, y0, ww, wh = pp.needed_window(*hw)
                frames = frames[:, y0:y0 + wh, x0:x0 + ww]
            tower_inputs.put_frames(paths, frames, hw)


def save_frame(frame, frame_path, cache: Optional[FrameCache] = None, tower_inputs=None) -> bool:
    """Drop-in for ``batch_process.save_frame`` (batch_process.py:73-114) with the JPEG encoded on the GPU instead of by
    ``cv2.imwrite``: a BGR (or grey) uint8 frame, a numpy array or a CUDA tensor, at quality 95 and 4:2:0.  The same return rules:
    an existing file returns True untouched; ``None`` or an empty frame returns False; the parent directory is created; every
    error is logged and returns False.  The bytes are Pillow's for the channel-swapped array (``jpeg.encode_jpeg``); they are not
    claimed to equal OpenCV's file.

    Measured on one MI355X (profiles/jpeg_encode.json; the encode alone, without the file write): one
    1280 x 720 host frame 0.41 ms against 2.14 ms for Pillow on one thread, one 1920 x 1080 host frame 0.68 against 4.69 ms,
    upload and read-back included; a resident frame 0.29 and 0.44 ms.  ``save_frames`` on 32 host frames: 5.9 ms (720p) and
    12.6 ms (1080p) against 68 and 152 ms, bound by the upload.  No point measured was slower than Pillow on one thread; several
    Pillow threads, and a GPU busy with the tower at the same time, were not measured.

    ``cache`` / ``tower_inputs``: see ``save_frames``; the same return rules."""
    if cache is not None or tower_inputs is not None:
        try:
            return save_frames([frame], [frame_path], cache=cache, tower_inputs=tower_inputs)[0]
        except Exception as e:                       # noqa: BLE001 - the reference's rule: log and return False
            _save_log.error(f"Error saving frame to {frame_path}: {e}")
            return False
    try:
        frame_path = Path(frame_path)
        if frame_path.exists():
            return True
        if frame is None or (frame.numel() if isinstance(frame, torch.Tensor) else frame.size) == 0:
            _save_log.error(f"Invalid frame data for {frame_path}")
            return False
        frame_path.parent.mkdir(parents=True, exist_ok=True)
        frame_path.write_bytes(_encode_bgr(frame)[0])
        if not frame_path.exists():
            _save_log.error(f"Frame file not found after save: {frame_path}")
            return False
        _save_log.debug(f"Successfully saved frame to {frame_path}")
        return True
    except Exception as e:                           # noqa: BLE001 - the reference's rule: log and return False
        _save_log.error(f"Error saving frame to {frame_path}: {e}")
        return False


def save_frames(frames, paths, cache: Optional[FrameCache] = None, tower_inputs=None) -> List[bool]:
    """``save_frame`` for a batch: the frames that still need a file are encoded in one ``encode_jpeg`` call (one upload, one launch
    sequence per geometry, one read-back).  frames: a list of frames or an (n, h, w, 3) array or tensor; paths: one per frame.
    -> save_frame's answer for each.

    Opt-in, for the two reads of these files that follow in the formation path.  While a frame is encoded the GPU holds all a
    decoder would recover from its file, so the decoded pixels -- Pillow's decode of the file, to the bit -- are made there
    (``encode_jpeg(return_decoded=True)``) and handed to
      cache: a ``FrameCache`` -- gray frame and min / max of every file this call wrote, under the key of the file as written, so
        that ``segment_sequence`` / ``_compute_frame_similarity`` over these paths (``PathScorer(cache)``, or ``default_cache()``)
        decode nothing: ``cache.decodes`` does not move, scores and segments are the same bits;
      tower_inputs: a ``preprocess.TowerInputCache`` -- the (3, 224, 224) tower input of every file this call wrote, for
        ``ImageBind(..., tower_inputs=)``.extract_features over these paths.
    A frame whose file already existed is not put (the file may not be this frame's), nor one whose write failed.  Rewriting a
    file later changes its key: the path is then a miss and is decoded from the file as before.  Return values and logging are
    those without the caches; a failure while filling a cache is logged and leaves the answer True (the file is there)."""
    paths = [Path(p) for p in paths]
    frames = list(frames) if frames is not None else []
    if len(frames) != len(paths):
        raise ValueError(f"save_frames: {len(frames)} frames for {len(paths)} paths")
    results = [False] * len(paths)
    todo = []
    for i, (frame, path) in enumerate(zip(frames, paths)):
        try:
            if path.exists():
                results[i] = True
            elif frame is None or (frame.numel() if isinstance(frame, torch.Tensor) else frame.size) == 0:
                _save_log.error(f"Invalid frame data for {path}")
            else:
                todo.append(i)
        except Exception as e:                       # noqa: BLE001
            _save_log.error(f"Error saving frame to {path}: {e}")
    if not todo:
        return results
    resident = cache is not None or tower_inputs is not None
    decoded = None
    try:
        if resident:
            # only the tower asks and every frame has one size: the pixels under the resampling taps are all it needs
            sizes = {tuple(frames[i].shape[:2]) for i in todo}
            window = None
            if cache is None and len(sizes) == 1:
                from . import preprocess as pp
                window = pp.needed_window(*next(iter(sizes)))
            files, decoded = _encode_bgr([frames[i] for i in todo], return_decoded=True, window=window)
        else:
            files = _encode_bgr([frames[i] for i in todo])
    except Exception as e:                           # noqa: BLE001
        _save_log.error(f"Error encoding {len(todo)} frames: {e}")
        return results
    written = []
    for k, (i, data) in enumerate(zip(todo, files)):
        try:
            paths[i].parent.mkdir(parents=True, exist_ok=True)
            paths[i].write_bytes(data)
            results[i] = paths[i].exists()
            if results[i] and resident:
                written.append((paths[i], decoded[k], tuple(int(v) for v in frames[i].shape[:2])))
        except Exception as e:                       # noqa: BLE001
            _save_log.error(f"Error saving frame to {paths[i]}: {e}")
    if written:
        try:
            _fill_caches(written, cache, tower_inputs)
        except Exception as e:                       # noqa: BLE001
            _save_log.error(f"Error keeping {len(written)} decoded frames on the device: {e}")
    return results


# ---------------------------------------------------------------------------------------------------------------------------------
# the decision loop of extract_frames_from_video (batch_process.py:179-228), its state on the device
# ---------------------------------------------------------------------------------------------------------------------------------
CHECK_INTERVAL = 30                       # extract_frames_from_video's defaults (batch_process.py:121-123)
MAX_DIFF_THRESHOLD = 0.3
MIN_SAVE_GAP = 1.0                        # "ensure at least 1 second between saves" (:191)
EXTRACT_BATCH = 16                        # candidates per flush: the best of 1, 4, 16 measured (profiles/frame_extraction.json)

# hmm_extract_state and hmm_extract_record of include/hippomm_hip.h
EXTRACT_STATE = np.dtype([("has_anchor", "<i4"), ("anchor_slot", "<i4"), ("cumulative_diff", "<f8"), ("last_save_time", "<f8")])
EXTRACT_RECORD = np.dtype([("compared", "<i4"), ("saved", "<i4"), ("anchor_slot_after", "<i4"), ("has_anchor_after", "<i4"),
                           ("diff", "<f8"), ("cumulative_after", "<f8"), ("last_save_time_after", "<f8")])


@dataclass
class ExtractionState:
    """The walk's state between calls: ``record`` is one EXTRACT_STATE element (its ``anchor_slot`` is 0 whenever there is an
    anchor), ``anchor`` the (H, W) uint8 gray of the last saved frame on the device, or None."""
    record: np.ndarray
    anchor: Optional[torch.Tensor] = None


def _state_record(has_anchor=0, anchor_slot=0, cumulative_diff=0.0, last_save_time=0.0) -> np.ndarray:
    rec = np.zeros(1, EXTRACT_STATE)
    rec[0] = (has_anchor, anchor_slot, cumulative_diff, last_save_time)
    return rec


def _state_after(record) -> np.ndarray:
    """The state a record leaves behind."""
    return _state_record(record["has_anchor_after"], record["anchor_slot_after"], record["cumulative_after"],
                         record["last_save_time_after"])


class _Walker:
    """The device buffers of the walk for one frame size: gray slots (slot 0: the anchor), records and state in one buffer (one
    read-back), workspace."""

    def __init__(self, h: int, w: int, capacity: int, dev):
        lib = _lib.load()
        self.h, self.w, self.capacity, self.dev = h, w, capacity, dev
        self.slots = torch.empty((capacity + 1, h, w), dtype=torch.uint8, device=dev)
        self.minmax = torch.empty((capacity + 1, 2), dtype=torch.int32, device=dev)
        self.out = torch.zeros(capacity * EXTRACT_RECORD.itemsize + EXTRACT_STATE.itemsize, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(max(lib.hmm_extract_walk_workspace_bytes(h, w), 256), dtype=torch.uint8, device=dev)

    @property
    def _state_at(self) -> int:
        return self.capacity * EXTRACT_RECORD.itemsize

    def set_state(self, record: np.ndarray) -> None:
        self.out[self._state_at:].copy_(torch.from_numpy(record.view(np.uint8).copy()))

    def fill(self, frames: torch.Tensor) -> None:
        """(n, H, W, 3) BGR or (n, H, W) gray on the device -> slots 1 .. n."""
        n = frames.shape[0]
        if frames.dim() == 4:
            _gray_into(frames, _ORDER["BGR"], self.slots[1:n + 1], self.minmax[1:n + 1])
        else:
            self.slots[1:n + 1].copy_(frames)

    def walk(self, first: int, times, check, deny, threshold: float, min_gap: float) -> None:
        """Candidates first .. first + len(times) - 1 (0-based in the batch; slot = index + 1); record i lands at index i."""
        times = np.ascontiguousarray(times, dtype=np.float64)
        check = np.ascontiguousarray(check, dtype=np.int32)
        deny = np.ascontiguousarray(deny, dtype=np.int32)
        base = self.out.data_ptr()
        _lib.check(_lib.load().hmm_extract_walk(self.slots.data_ptr(), self.capacity + 1, self.h, self.w, first + 1, len(times),
                                                times.ctypes.data, check.ctypes.data, deny.ctypes.data, float(threshold),
                                                float(min_gap), base + self._state_at, base + first * EXTRACT_RECORD.itemsize,
                                                self.ws.data_ptr(), self.ws.numel(), _lib.stream_ptr()), "hmm_extract_walk")

    def carry(self) -> None:
        _lib.check(_lib.load().hmm_extract_carry(self.slots.data_ptr(), self.capacity + 1, self.h, self.w,
                                                 self.out.data_ptr() + self._state_at, _lib.stream_ptr()), "hmm_extract_carry")

    def read(self, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """One read-back -> (records[:n], the state)."""
        host = self.out.cpu().numpy()
        return host[:n * EXTRACT_RECORD.itemsize].view(EXTRACT_RECORD).copy(), host[self._state_at:].view(EXTRACT_STATE).copy()


def extraction_records(frames, frame_counts, video_fps, *, check_interval: int = CHECK_INTERVAL,
                       max_diff_threshold: float = MAX_DIFF_THRESHOLD, min_gap: float = MIN_SAVE_GAP,
                       state: Optional[ExtractionState] = None, deny=()):
    """The decisions of ``extract_frames_from_video``'s loop (batch_process.py:184-218) for a batch of candidate frames, on the GPU:
    one gray launch, one walk (``hmm_extract_walk``), one read-back.  frames: (n, H, W, 3) BGR or (n, H, W) gray uint8, a numpy
    array or a tensor on the host or the device; frame_counts: the frames' positions in the video.  ``current_time`` is
    ``frame_count / video_fps`` in Python floats (:184) and a frame is checked when ``frame_count % check_interval == 0``; while
    there is no anchor every frame is saved without a comparison.  ``deny``: positions in this batch whose save failed
    (``save_frame`` returned False): they leave the state as it is.  ``state``: what an earlier call returned, None to start.
    -> (records, state): an EXTRACT_RECORD array, one element per frame -- ``diff`` is ``1.0 - ssim_pairs(gray, [(frame, anchor)],
    255)`` bit for bit where ``compared`` -- and the ``ExtractionState`` to hand to the next call.  Slot numbers in the records
    count from 1 within this batch; 0 is the anchor carried in.  Sides under 7 raise ``ValueError`` (the reference's MSE fallback
    for them is ``compute_frame_difference``'s, on the host)."""
    f = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
    if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or not (f.dim() == 3 or (f.dim() == 4 and f.shape[3] == 3)):
        raise TypeError("frames must be uint8 (n, H, W, 3) BGR or (n, H, W) gray")
    dev = _lib.require_gpu()
    counts = [int(c) for c in frame_counts]
    n, h, w = f.shape[:3]
    if len(counts) != n:
        raise ValueError(f"extraction_records: {n} frames for {len(counts)} frame counts")
    if h < WIN or w < WIN:
        raise ValueError(f"win_size exceeds image extent: {h}x{w} frames, the window is {WIN}x{WIN}")
    if state is not None and state.anchor is not None and tuple(state.anchor.shape) != (h, w):
        raise ValueError(f"Input images must have the same dimensions: the anchor is {tuple(state.anchor.shape)}, frames are {(h, w)}")
    if n == 0:
        return np.zeros(0, EXTRACT_RECORD), state if state is not None else ExtractionState(_state_record())
    walker = _Walker(h, w, n, dev)
    if state is not None:
        rec = state.record.copy()
        if state.anchor is not None:
            walker.slots[0].copy_(state.anchor)
            rec["anchor_slot"] = 0
        else:
            rec["has_anchor"] = 0
        walker.set_state(rec)
    walker.fill(f.to(dev).contiguous())
    denied = np.zeros(n, np.int32)
    denied[list(deny)] = 1
    walker.walk(0, [c / video_fps for c in counts], [c % check_interval == 0 for c in counts], denied, max_diff_threshold, min_gap)
    walker.carry()
    records, final = walker.read(n)
    return records, ExtractionState(final, walker.slots[0].clone() if final["has_anchor"][0] else None)


class FrameExtractor:
    """The loop body of ``extract_frames_from_video`` (batch_process.py:179-228) with the last saved frame, ``cumulative_diff`` and
    ``last_save_time`` on the device: ``push(frame_count, frame)`` for every frame ``cap.read()`` yields, ``flush()`` at the end;
    ``frame_paths``, ``frame_times`` and ``failed_saves`` then hold what the reference's variables of those names hold, and
    ``records`` one entry per frame that was looked at.  Opening the video, the ``metadata.yaml`` resume logic around the loop and
    the progress bar stay with the caller.

    A frame that is not due for a check returns at once.  A candidate is copied into pinned staging (the caller may reuse its
    buffer); every ``batch`` candidates are uploaded in one copy, made gray, walked (``hmm_extract_walk``: two launches per
    candidate, no synchronisation between them) and the records read back once; the kept frames are written from the resident BGR
    by ``save_frames`` (``cache=`` / ``tower_inputs=`` as there), to ``frames_dir / f"t_{int(t):04d}" / f"frame_{n:06d}.jpg"``.  So
    files appear at each flush, not frame by frame.  While no frame has been saved yet every frame is a candidate and is flushed
    alone, as the reference tries frame 1, 2, ... when frame 0 cannot be saved.

    A save that fails (``save_frames`` answers False; a file that already exists counts as saved, as in the reference) is counted in
    ``failed_saves``; the state is put back to what it was before that candidate and the rest of the batch is walked again with
    the candidate denied.  Files this flush had already written for later candidates of the batch are removed again: the second
    walk decides about them anew.

    A candidate whose shape differs from the anchor's, or with a side under 7, is decided on the host with
    ``compute_frame_difference`` (the reference's MSE fallback) against the anchor's gray read back from the device.

    Measured on one MI355X (profiles/frame_extraction.json; 64 checked host frames of which 32 are kept,
    files on tmpfs): 0.26 ms per checked 720p frame and 0.58 ms per 1080p frame at ``batch`` 16, against 0.60 and 1.26 ms for
    ``compute_frame_difference`` + ``save_frame`` per frame; ``batch`` 4: 0.34 and 0.69 ms, ``batch`` 1: 0.47 and 0.82 ms.  No
    batch measured was slower than the two single-shot calls; batches above 16 and a caller's own ``cap.read()`` beside it were
    not measured."""

    def __init__(self, video_fps: float, frames_dir, *, check_interval: int = CHECK_INTERVAL,
                 max_diff_threshold: float = MAX_DIFF_THRESHOLD, batch: int = EXTRACT_BATCH,
                 cache: Optional[FrameCache] = None, tower_inputs=None):
        if batch < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        self.video_fps, self.frames_dir = video_fps, Path(frames_dir)
        self.check_interval, self.max_diff_threshold, self.batch = check_interval, max_diff_threshold, int(batch)
        self.cache, self.tower_inputs = cache, tower_inputs
        self.frame_paths: List[str] = []
        self.frame_times: List[float] = []
        self.failed_saves = 0
        self._dev = _lib.require_gpu()
        self._state = _state_record()                  # host mirror of the device state, exact after every flush
        self._walker: Optional[_Walker] = None         # its slot 0 holds the anchor's gray
        self._stage = None                             # PinnedStage of (batch, *frame shape)
        self._counts: List[int] = []
        self._log: List[Tuple[int, np.ndarray]] = []

    @property
    def records(self) -> np.ndarray:
        """One element per frame looked at, in order: ``frame_count`` and the EXTRACT_RECORD fields (slots count from 1 within the
        frame's flush)."""
        out = np.zeros(len(self._log), np.dtype([("frame_count", "<i8")] + EXTRACT_RECORD.descr))
        for k, (count, rec) in enumerate(self._log):
            out[k] = (count, *rec.tolist())
        return out

    def _path(self, frame_count: int) -> Path:
        return self.frames_dir / f"t_{int(frame_count / self.video_fps):04d}" / f"frame_{frame_count:06d}.jpg"

    def push(self, frame_count: int, frame: np.ndarray) -> None:
        has_anchor = bool(self._state["has_anchor"][0])
        if has_anchor and frame_count % self.check_interval != 0:
            return
        frame = _check_frame(frame, "frame")
        h, w = frame.shape[:2]
        if self._counts and self._stage.host.shape[1:] != frame.shape:
            self.flush()
            has_anchor = bool(self._state["has_anchor"][0])
        if h < WIN or w < WIN or (has_anchor and (self._walker.h, self._walker.w) != (h, w)):
            self.flush()
            self._decide_on_host(frame_count, frame)
            return
        if self._stage is None or self._stage.host.shape[1:] != frame.shape:
            from ._pinned import PinnedStage
            if self._stage is not None:
                self._stage.wait()
            self._stage = PinnedStage((self.batch, *frame.shape))
        if not self._counts:
            self._stage.wait()
        self._stage.host[len(self._counts)] = frame
        self._counts.append(int(frame_count))
        if len(self._counts) >= self.batch or not has_anchor:
            self.flush()

    def _walker_for(self, h: int, w: int) -> _Walker:
        wk = self._walker
        if wk is None or (wk.h, wk.w) != (h, w):
            wk = self._walker = _Walker(h, w, self.batch, self._dev)       # a new size starts without an anchor on the device
            wk.set_state(self._state)
        return wk

    def _commit(self, frame_count: int, path: Path) -> None:
        self.frame_paths.append(str(path))
        self.frame_times.append(frame_count / self.video_fps)

    def flush(self) -> None:
        n = len(self._counts)
        if not n:
            return
        counts, self._counts = self._counts, []
        up = self._stage.pinned[:n].to(self._dev, non_blocking=True)
        self._stage.mark()
        wk = self._walker_for(*up.shape[1:3])
        wk.fill(up)
        times = [c / self.video_fps for c in counts]
        check = [c % self.check_interval == 0 for c in counts]
        deny = np.zeros(n, np.int32)
        snapshot, first = self._state.copy(), 0
        while True:
            wk.walk(first, times[first:], check[first:], deny[first:], self.max_diff_threshold, MIN_SAVE_GAP)
            records, _ = wk.read(n)
            kept = [i for i in range(first, n) if records["saved"][i]]
            paths = [self._path(counts[i]) for i in kept]
            existed = [p.exists() for p in paths]
            done = save_frames([up[i] for i in kept], paths, cache=self.cache, tower_inputs=self.tower_inputs) if kept else []
            bad = next((k for k, ok in enumerate(done) if not ok), None)
            for i, path in list(zip(kept, paths))[:bad]:
                self._commit(counts[i], path)
            if bad is None:
                break
            for k in range(bad + 1, len(kept)):                            # the second walk decides about these anew
                if done[k] and not existed[k]:
                    try:
                        paths[k].unlink()
                    except OSError as e:
                        _save_log.error(f"Error removing {paths[k]}: {e}")
            self.failed_saves += 1
            first = kept[bad]
            deny[first] = 1
            wk.set_state(snapshot if first == 0 else _state_after(records[first - 1]))
        self._log.extend((c, records[i]) for i, c in enumerate(counts))
        wk.carry()
        self._state = _state_after(records[n - 1])
        if self._state["has_anchor"][0]:
            self._state["anchor_slot"] = 0

    def _decide_on_host(self, frame_count: int, frame: np.ndarray) -> None:
        """Lines :184-223 for one frame on the host: a frame of another shape than the anchor's, or with a side under 7."""
        st = self._state
        t = frame_count / self.video_fps
        rec = np.zeros(1, EXTRACT_RECORD)
        save = not st["has_anchor"][0]
        if not save and t - st["last_save_time"][0] >= MIN_SAVE_GAP and frame_count % self.check_interval == 0:
            diff = compute_frame_difference(frame, self._walker.slots[0].cpu().numpy())
            st["cumulative_diff"] += diff
            rec["compared"], rec["diff"] = 1, diff
            save = diff > self.max_diff_threshold or st["cumulative_diff"][0] > self.max_diff_threshold
        if save:
            path = self._path(frame_count)
            if save_frames([frame], [path], cache=self.cache, tower_inputs=self.tower_inputs)[0]:
                self._commit(frame_count, path)
                h, w = frame.shape[:2]
                wk = self._walker_for(h, w)
                wk.slots[0].copy_(torch.from_numpy(np.ascontiguousarray(_host_gray(frame))))
                st[0] = (1, 0, 0.0, t)
                rec["saved"] = 1
            else:
                self.failed_saves += 1
        if self._walker is not None:
            self._walker.set_state(st)
        rec["has_anchor_after"], rec["cumulative_after"], rec["last_save_time_after"] = \
            st["has_anchor"], st["cumulative_diff"], st["last_save_time"]
        self._log.append((int(frame_count), rec[0]))


def extract_frames(frames, video_fps: float, frames_dir, **kw) -> Tuple[List[str], List[float], int]:
    """The loop of ``extract_frames_from_video`` over ``frames``, any iterable of BGR uint8 arrays in video order (what
    ``cap.read()`` yields): every frame is pushed into a ``FrameExtractor(video_fps, frames_dir, **kw)`` with its running count,
    then the extractor is flushed.  -> (frame_paths, frame_times, failed_saves) as the reference's variables of those names.
    Left with the caller: opening the video (``cv2.VideoCapture``, fps and frame count), the ``metadata.yaml`` resume logic around
    the loop and the progress bar."""
    ex = FrameExtractor(video_fps, frames_dir, **kw)
    for frame_count, frame in enumerate(frames):
        ex.push(frame_count, frame)
    ex.flush()
    return ex.frame_paths, ex.frame_times, ex.failed_saves
