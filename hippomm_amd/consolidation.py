"""Consolidation similarity on MI355X -- host-side mirror of
``HippocampalMemory._select_key_frames`` (hippomm/core/hippocampal_memory.py:944-967),
bound to ``hmm_gram_select`` (fp32 normalise, fp64-accumulated gram via f64 MFMA, greedy scan).  ``KeyFrameSelector`` is the
same selection grown batch by batch (``hmm_keyframe_extend``): each frame is decided when its embedding arrives.
"""
from __future__ import annotations

import threading
from typing import Optional, Union

import numpy as np
import torch

from . import _lib

FEATURE_DIM = 1024


# (device, stream, host thread, n) -> (kept int64[n], n_kept int32[1], workspace): select_key_frames_async allocates nothing
# after its first call.  The stream and the thread are part of the key: two selections of the same n on different streams or
# threads never share a workspace.  Only the async entry point uses the cache; the synchronous wrappers own their buffers.
_BUFFERS = {}
_BUFFERS_LOCK = threading.Lock()     # lookup / evict / insert as one step; an evicted entry stays alive with whoever holds it


def _new_buffers(lib, n, dev):
    need = lib.hmm_gram_select_workspace_bytes(n)
    return (torch.empty(max(n, 1), dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
            torch.empty(max(need, 256), dtype=torch.uint8, device=dev))


def _prepare(features: torch.Tensor) -> torch.Tensor:
    if features.dim() != 2 or features.shape[1] != FEATURE_DIM:
        raise ValueError(f"features must be (n,{FEATURE_DIM}), got {tuple(features.shape)}")
    return features if features.dtype == torch.float32 and features.is_contiguous() else features.to(dtype=torch.float32).contiguous()


def _launch(lib, f, similarity_threshold, buf):
    kept, n_kept, ws = buf
    thr = float(np.float32(similarity_threshold))     # the reference compares in float32 (:960)
    _lib.check(lib.hmm_gram_select(f.data_ptr(), f.shape[0], FEATURE_DIM, thr, kept.data_ptr(), n_kept.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "hmm_gram_select")
    return kept, n_kept


def select_key_frames_async(features: torch.Tensor, similarity_threshold: float = 0.9):
    """features: (n,1024) fp32 CUDA tensor -> (kept int64[n], n_kept int32[1]) CUDA tensors, WITHOUT synchronising: the
    kept indices are ``kept[:n_kept]`` once the stream has run.  Launch-only (no allocation after the first call for a
    given n on this stream and thread, no read-back); the two tensors are reused by the next such call, so consume or copy
    them before that."""
    lib = _lib.load()
    f = _prepare(features)
    n, dev = f.shape[0], f.device
    key = (dev.index, int(_lib.stream_ptr().value or 0), threading.get_ident(), n)
    with _BUFFERS_LOCK:
        buf = _BUFFERS.get(key)
        if buf is None:
            if len(_BUFFERS) >= 16:                         # a handful of sizes recur (frame buffer, per-video totals)
                _BUFFERS.pop(next(iter(_BUFFERS)), None)    # the evicted tuple lives on in the caller that still uses it
            buf = _BUFFERS[key] = _new_buffers(lib, n, dev)
    return _launch(lib, f, similarity_threshold, buf)


def select_key_frames_device(features: torch.Tensor, similarity_threshold: float = 0.9) -> torch.Tensor:
    """features: (n,1024) fp32 CUDA tensor -> kept indices int64 CUDA tensor (synchronises once to read the count; buffers
    and result are this call's own)."""
    lib = _lib.load()
    f = _prepare(features)
    kept, n_kept = _launch(lib, f, similarity_threshold, _new_buffers(lib, f.shape[0], f.device))
    return kept[: int(n_kept.item())]


def select_key_frames(features: Union[np.ndarray, torch.Tensor], times: Optional[np.ndarray] = None,
                      similarity_threshold: float = 0.9) -> np.ndarray:
    """Same contract as the reference method: int64 indices, increasing, first is 0; ``times`` is
    accepted and unused, as in the reference.  Features are taken as float32, which is what the encoder hands over
    (hippocampal_memory.py:1186, :842).  A float64 matrix (what ``load_theta_event`` yields) holds exactly-float32 values
     and is converted without loss; the reference would then run its gram in float64, which can differ from the
    float32 comparison only for pairs within ~1e-7 of the threshold -- the same band in which its float32 answer already
    depends on the host's BLAS (tests/test_gpu_select.py pins that band to the fp64-accumulated definition)."""
    if len(features) <= 2:                              # :947-948
        return np.arange(len(features))
    dev = _lib.require_gpu()
    if isinstance(features, np.ndarray):
        f = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(dev)
    else:
        f = features.to(dev)
    return select_key_frames_device(f, similarity_threshold).cpu().numpy()


def _select_key_frames(self, features: np.ndarray, times: np.ndarray,
                       similarity_threshold: float = 0.9) -> np.ndarray:
    """Drop-in for ``HippocampalMemory._select_key_frames`` (assign it on the class; ``self`` is
    unused there as well)."""
    return select_key_frames(features, times, similarity_threshold)


class KeyFrameSelector:
    """The key-frame selection of one video, grown batch by batch: ``extend`` takes the embeddings of the next frames and decides
    each of them at once, so that the kept frames can be used (captioned, stored) while later frames are still being encoded.

    After any number of ``extend`` calls ``kept()`` is what ``select_key_frames`` answers for all rows given so far, bit for bit,
    pairs within 1e-7 of the threshold included: new rows are compared with the kept rows and with each other by the kernels'
    one gram mainloop (``hmm_keyframe_extend``).  The state on the device is the normalised kept rows alone, 4 KB each.

    Rows must arrive in time order: the reference sorts by time before it selects, and its live path delivers frames in order.
    A frame's decision is final on arrival, with one exception: the reference keeps both rows of a two-row video without
    comparing them (hippocampal_memory.py:947-948), so ``kept()`` is ``arange(n_seen)`` while ``n_seen <= 2`` and the greedy
    state from the third row on -- row 1's status is provisional until a third row has arrived.

    The threshold is fixed for the selector's life (compared in float32, as ``select_key_frames`` does).  One selector's calls
    belong on one stream.  There is no CPU fallback."""

    def __init__(self, similarity_threshold: float = 0.9, device=None, capacity: int = 1024):
        self.similarity_threshold = float(np.float32(similarity_threshold))     # the reference compares in float32 (:960)
        self._device = None if device is None else torch.device(device)
        self._initial_capacity = max(int(capacity), 1)
        self._rows = None            # (capacity,1024) fp32: the normalised kept rows, in kept order
        self._meta = None            # int64[1 + capacity]: the kept count, then the kept global indices (one read-back gets both)
        self._ws = None
        self._n_seen = 0
        self._bound = 0              # min(n_seen, last count read + rows given since) >= the count on the device

    @property
    def n_seen(self) -> int:
        return self._n_seen

    @property
    def capacity(self) -> int:
        return 0 if self._rows is None else self._rows.shape[0]

    def reset(self):
        """Start over (the next ``extend`` begins a selection); the buffers stay."""
        self._n_seen = self._bound = 0
        return self

    def _read_count(self) -> int:
        count = min(max(int(self._meta[0].item()), 0), self._bound) if self._n_seen else 0
        self._bound = count
        return count

    def _reserve(self, m: int, dev):
        if self._rows is not None and self._bound + m <= self.capacity:
            return
        count = self._read_count() if self._rows is not None else 0      # the exact count: grow only when needed
        if self._rows is not None and count + m <= self.capacity:
            return
        capacity = max(count + m, 2 * self.capacity, self._initial_capacity)
        rows = torch.empty(capacity, FEATURE_DIM, dtype=torch.float32, device=dev)
        meta = torch.empty(1 + capacity, dtype=torch.int64, device=dev)
        if count:
            rows[:count].copy_(self._rows[:count])
            meta[: 1 + count].copy_(self._meta[: 1 + count])
        self._rows, self._meta = rows, meta

    def extend(self, features: Union[np.ndarray, torch.Tensor]) -> "KeyFrameSelector":
        """Append the next rows, in time order: (m,1024) or one (1024,) row, numpy or torch.  Features are taken as float32; a
        float64 numpy array is converted as ``select_key_frames`` converts it.  With a device tensor the call is launch-only on
        the current stream (it reads the count back only when the kept rows may outgrow their buffer)."""
        dev = _lib.require_gpu() if self._device is None else self._device
        if self._device is not None:
            _lib.require_gpu()
        if isinstance(features, np.ndarray):
            features = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32))
        if features.dim() == 1:
            features = features.unsqueeze(0)
        f = _prepare(features.to(dev))
        m = f.shape[0]
        if m == 0:
            return self
        self._device = dev
        lib = _lib.load()
        with torch.cuda.device(dev):
            self._reserve(m, dev)
            need = lib.hmm_keyframe_extend_workspace_bytes(m)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            _lib.check(lib.hmm_keyframe_extend(f.data_ptr(), m, FEATURE_DIM, self.similarity_threshold, self._rows.data_ptr(),
                                               self._meta.data_ptr() + 8, self.capacity, self._meta.data_ptr(), self._n_seen,
                                               self._bound, self._ws.data_ptr(), self._ws.numel(), _lib.stream_ptr()),
                       "hmm_keyframe_extend")
        self._n_seen += m
        self._bound = min(self._n_seen, self._bound + m)
        return self

    def kept_device(self) -> torch.Tensor:
        """The kept indices as an int64 tensor of its own on the device (synchronises once to read the count)."""
        if self._n_seen <= 2:                                # hippocampal_memory.py:947-948
            dev = self._device if self._device is not None else _lib.require_gpu()
            return torch.arange(self._n_seen, dtype=torch.int64, device=dev)
        count = self._read_count()
        return self._meta[1: 1 + count].clone()

    def kept(self) -> np.ndarray:
        """The kept indices so far, int64, increasing, first is 0.  One read-back of the count and the indices (one
        synchronisation); it also tightens the host's bound on the count."""
        if self._n_seen <= 2:                                # hippocampal_memory.py:947-948
            return np.arange(self._n_seen, dtype=np.int64)
        host = self._meta[: 1 + self._bound].cpu().numpy()
        count = min(max(int(host[0]), 0), self._bound)
        self._bound = count
        return host[1: 1 + count].copy()
