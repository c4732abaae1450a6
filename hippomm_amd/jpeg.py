"""Baseline JPEG decoding with the pixel work on the GPU, bit-exact with Pillow (``Image.open(p).convert("RGB")``).

The host runs the marker parser and the Huffman (entropy) pass into dense int16 coefficient blocks (hippomm_amd/csrc/
jpeg_host.cpp, through ctypes: no interpreter lock held); the GPU dequantises, runs libjpeg-turbo's islow IDCT, its fancy chroma
upsampling and its fixed-point YCbCr -> RGB (hippomm_amd/csrc/jpeg.hip).  Only 8-bit Huffman sequential files with one
interleaved scan of grey or YCbCr at 4:4:4, 4:2:2 or 4:2:0 take this route; every other file, and every file with an anomaly
in its data, is decoded by Pillow as before.  The route is chosen by the input alone; there is no user option.

The first frame a process decodes on the device is compared with Pillow's decode of the same bytes; on a mismatch (another
Pillow or libjpeg-turbo build) the route is turned off for the process and a warning is logged.
"""
from __future__ import annotations

import io
import logging
import threading
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

GEOMETRY_INTS = 6
DECODED, UNSUPPORTED, OTHER_GEOMETRY = 0, 1, 2

_log = logging.getLogger(__name__)
_route = {"on": True}                  # private A/B switch for measurements (False: every frame takes Pillow's route); no user option
_check = {"ok": None}                  # None: not verified in this process yet; False: this Pillow disagrees, route off
_check_lock = threading.Lock()
_counts = {"device": 0, "host": 0}     # frames per route since the process started (decode_stats)
_pinned = {}                           # device -> [pinned u8 buffer, event behind its last upload]


def _geom_array(geometry) -> np.ndarray:
    g = np.zeros(GEOMETRY_INTS, dtype=np.int32)
    g[:len(geometry)] = geometry
    return g


def parse(data: bytes) -> Optional[Tuple[int, ...]]:
    """-> (width, height, components, luma h sampling, luma v sampling, restart interval) of a file this decoder takes, else None."""
    g = np.zeros(GEOMETRY_INTS, dtype=np.int32)
    st = _lib.load().hmm_jpeg_parse(data, len(data), g.ctypes.data)
    return tuple(int(v) for v in g) if st == DECODED else None


def slot_bytes(geometry, window) -> int:
    """Bytes of one coefficient slot for frames of `geometry` cut to `window` (x0, y0, w, h)."""
    n = _lib.load().hmm_jpeg_slot_bytes(_geom_array(geometry).ctypes.data, *map(int, window))
    if n <= 0:
        raise ValueError(f"window {tuple(window)} does not fit a {geometry[0]} x {geometry[1]} frame")
    return int(n)


def decode_coefs(data: bytes, geometry, window, slot: np.ndarray) -> int:
    """Entropy pass of one file into `slot` (a u8 array of at least slot_bytes) -> DECODED, UNSUPPORTED or OTHER_GEOMETRY."""
    st = _lib.load().hmm_jpeg_decode_coefs(data, len(data), _geom_array(geometry).ctypes.data, *map(int, window),
                                           slot.ctypes.data, slot.nbytes)
    if st < 0:
        _lib.check(st, "hmm_jpeg_decode_coefs")
    return int(st)


def reconstruct(slots: torch.Tensor, geometry, window, out: torch.Tensor) -> torch.Tensor:
    """slots (n, stride) u8 on the GPU -> out (n, h, w, 3) u8 (the window of every frame), on the current stream."""
    lib = _lib.load()
    g = _geom_array(geometry)
    n = slots.shape[0]
    x0, y0, w, h = map(int, window)
    ws = torch.empty(lib.hmm_jpeg_workspace_bytes(g.ctypes.data, n, x0, y0, w, h), dtype=torch.uint8, device=slots.device)
    _lib.check(lib.hmm_jpeg_reconstruct(slots.data_ptr(), n, slots.stride(0), g.ctypes.data, x0, y0, w, h, out.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "hmm_jpeg_reconstruct")
    return out


def _pillow_rgb(source) -> np.ndarray:
    from PIL import Image
    with Image.open(io.BytesIO(source) if isinstance(source, (bytes, bytearray, memoryview)) else source) as im:
        return np.asarray(im.convert("RGB"))


def route_ok(data: bytes, dev) -> bool:
    """May frames take the device route in this process?  The first time, `data` (a supported JPEG) is decoded on the device and
    compared with Pillow's decode of the same bytes; the answer is kept for the process."""
    if not _route["on"] or _check["ok"] is False:
        return False
    if _check["ok"]:
        return True
    with _check_lock:
        if _check["ok"] is None:
            geometry = parse(data)
            if geometry is None:
                return False
            window = (0, 0, geometry[0], geometry[1])
            slot = np.zeros(slot_bytes(geometry, window), dtype=np.uint8)
            if decode_coefs(data, geometry, window, slot) != DECODED:
                return False
            with torch.cuda.device(dev):
                out = torch.empty(1, geometry[1], geometry[0], 3, dtype=torch.uint8, device=dev)
                reconstruct(torch.from_numpy(slot).to(dev)[None], geometry, window, out)
                got = out[0].cpu().numpy()
            ok = bool(np.array_equal(got, _pillow_rgb(data)))
            if not ok:
                _log.warning("hippomm_amd.jpeg: the device JPEG route disagrees with this Pillow's decoder; "
                             "every JPEG is decoded by Pillow in this process")
            _check["ok"] = ok
    return bool(_check["ok"])


def decode_stats() -> dict:
    """Frames decoded per route ("device", "host") by decode_jpeg since the process started."""
    return dict(_counts)


def takes(geometry) -> bool:
    """May a file of `geometry` (parse's answer, or None) take the device route?  Not beyond Pillow's decompression-bomb limit
    (Image.MAX_IMAGE_PIXELS): Pillow warns or raises there, so such a file goes through Pillow."""
    if geometry is None:
        return False
    from PIL import Image
    limit = Image.MAX_IMAGE_PIXELS
    return limit is None or geometry[0] * geometry[1] <= limit


def _pinned_slots(dev, nbytes: int) -> list:
    """The pinned staging buffer of `dev` (at least nbytes), once its previous upload has left it.  Caller holds _stage_lock."""
    key = str(dev)
    ent = _pinned.get(key)
    if ent is None or ent[0].numel() < nbytes:
        if ent is not None and ent[1] is not None:
            ent[1].synchronize()
        ent = _pinned[key] = [torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True), None]
    elif ent[1] is not None:
        ent[1].synchronize()                         # the previous call's upload has left the buffer
    return ent


_stage_lock = threading.Lock()                     # one call at a time fills and uploads the pinned staging buffer


def _read(source):
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    try:
        with open(source, "rb") as fh:
            return fh.read()
    except OSError:
        return None                                  # Pillow's route raises its own error for it


def _decode_many(srcs: Sequence, dev, window=None) -> Tuple[list, list, int]:
    """-> (per source: an (h, w, 3) uint8 tensor on `dev` or None, per source: the exception Pillow raised or None, frames
    decoded on the device).  The work of decode_jpeg, without raising; the current stream is used."""
    from . import preprocess as pp
    n = len(srcs)
    workers = min(pp.decode_workers(), n)
    pool = pp._decode_pool(workers) if workers > 1 else None
    datas = list(pool.map(_read, srcs)) if pool and n > 1 else [_read(x) for x in srcs]
    geoms = [parse(d) if d is not None else None for d in datas]

    def crop_of(geometry):
        if window is None:
            return (0, 0, geometry[0], geometry[1])
        x0, y0, w, h = map(int, window)
        return (x0, y0, w, h) if x0 >= 0 and y0 >= 0 and w > 0 and h > 0 and x0 + w <= geometry[0] and y0 + h <= geometry[1] else None

    cand = [i for i in range(n) if takes(geoms[i]) and crop_of(geoms[i]) is not None]
    groups = {}                                      # (geometry[:5], window) -> frame indices on the device route
    if cand and route_ok(datas[cand[0]], dev):
        for i in cand:
            groups.setdefault((geoms[i][:5], crop_of(geoms[i])), []).append(i)
    plan, total = [], 0
    for (g5, crop), idx in groups.items():
        sb = slot_bytes(g5, crop)
        plan.append((g5, crop, idx, total, sb))
        total += sb * len(idx)
    results, errors = [None] * n, [None] * n
    on_dev = {}
    with torch.cuda.device(dev), _stage_lock:
        ent = _pinned_slots(dev, total) if total else None
        host_all = ent[0].numpy() if ent else None

        def entropy(job):
            g5, crop, i, off, sb = job
            return decode_coefs(datas[i], g5, crop, host_all[off:off + sb])

        jobs = [(g5, crop, i, off + k * sb, sb) for g5, crop, idx, off, sb in plan for k, i in enumerate(idx)]
        status = list(pool.map(entropy, jobs)) if pool and len(jobs) > 1 else [entropy(j) for j in jobs]
        on_dev = {j[2]: st == DECODED for j, st in zip(jobs, status)}
        if total:
            up = torch.empty(total, dtype=torch.uint8, device=dev)
            up.copy_(ent[0][:total], non_blocking=True)
            ent[1] = torch.cuda.Event()
            ent[1].record()
            for g5, crop, idx, off, sb in plan:
                keep = [k for k, i in enumerate(idx) if on_dev[i]]
                if not keep:
                    continue
                slots = up[off:off + sb * len(idx)].view(len(idx), sb)
                if len(keep) != len(idx):
                    slots = slots[torch.tensor(keep, device=dev)]
                out = torch.empty(len(keep), crop[3], crop[2], 3, dtype=torch.uint8, device=dev)
                reconstruct(slots, g5, crop, out)
                for k, o in zip(keep, out):
                    results[idx[k]] = o

    def host(i):
        try:
            arr = _pillow_rgb(srcs[i])                   # a path is opened by Pillow itself: its errors name the path
            if window is not None:
                x0, y0, w, h = map(int, window)
                if x0 < 0 or y0 < 0 or x0 + w > arr.shape[1] or y0 + h > arr.shape[0]:
                    raise ValueError(f"window {tuple(window)} does not fit a {arr.shape[1]} x {arr.shape[0]} frame")
                arr = arr[y0:y0 + h, x0:x0 + w]
            return np.array(arr, order="C"), None       # a writable copy: np.asarray(image) is read-only
        except Exception as exc:                     # noqa: BLE001 - the caller decides
            return None, exc

    rest = [i for i in range(n) if not on_dev.get(i, False)]
    done = list(pool.map(host, rest)) if pool and len(rest) > 1 else [host(i) for i in rest]
    with torch.cuda.device(dev):
        for i, (arr, exc) in zip(rest, done):
            if exc is not None:
                errors[i] = exc
            else:
                results[i] = torch.from_numpy(arr).to(dev)
    n_dev = sum(1 for v in on_dev.values() if v)
    _counts["device"] += n_dev
    _counts["host"] += n - n_dev
    return results, errors, n_dev


def decode_jpeg(sources: Sequence[Union[str, bytes]], device=None, window=None,
                stats: dict = None) -> Union[torch.Tensor, List[torch.Tensor]]:
    """Image files (paths or bytes) -> uint8 RGB on the device, each equal to ``np.asarray(Image.open(p).convert("RGB"))``
    (cut to ``window`` = (x0, y0, w, h) when given).  Returns an (n, h, w, 3) tensor when every frame has one size, else a list
    of (h, w, 3) tensors, in the order of `sources`.  Files this decoder does not take are decoded by Pillow on the host and
    uploaded; a file Pillow cannot open raises Pillow's error (the first in order).  `stats`, when given, receives the number
    of frames per route ("device", "host").  Safe to call from several threads."""
    dev = torch.device(device) if device is not None else _lib.require_gpu()
    srcs = list(sources)
    if not srcs:
        return torch.empty(0, 0, 0, 3, dtype=torch.uint8, device=dev)
    results, errors, n_dev = _decode_many(srcs, dev, window)
    for exc in errors:
        if exc is not None:
            raise exc
    if stats is not None:
        stats.update(device=n_dev, host=len(srcs) - n_dev)
    if len({tuple(r.shape) for r in results}) == 1:
        return torch.stack(results)
    return results
