"""Baseline JPEG decoding with the pixel work on the GPU, bit-exact with Pillow (``Image.open(p).convert("RGB")``).

The host runs the marker parser and the Huffman (entropy) pass into dense int16 coefficient blocks (hippomm_amd/csrc/
jpeg_host.cpp, through ctypes: no interpreter lock held); the GPU dequantises, runs libjpeg-turbo's islow IDCT, its fancy chroma
upsampling and its fixed-point YCbCr -> RGB (hippomm_amd/csrc/jpeg.hip).  Only 8-bit Huffman sequential files with one
interleaved scan of grey or YCbCr at 4:4:4, 4:2:2 or 4:2:0 take this route; every other file, and every file with an anomaly
in its data, is decoded by Pillow as before.  The route is chosen by the input alone; there is no user option.

The entropy pass itself can run on the GPU too (hippomm_amd/csrc/jpeg_entropy.hip): opt-in, ``entropy="device"`` or
``HMM_JPEG_ENTROPY=device``.  The host then only strips the scan of its byte stuffing (hmm_jpeg_prepare_entropy); the kernel
leaves the coefficient slots the host pass would have written, byte for byte.  A frame the kernel does not report as decoded
(and every file with a restart interval) is decoded by the host entropy pass, and by Pillow if that refuses too: the outcome
for every file is the host route's.

The first frame a process decodes on the device is compared with Pillow's decode of the same bytes; on a mismatch (another
Pillow or libjpeg-turbo build) the route is turned off for the process and a warning is logged.
"""
from __future__ import annotations

import io
import logging
import os
import threading
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._pinned import stage

GEOMETRY_INTS = 6
DECODED, UNSUPPORTED, OTHER_GEOMETRY = 0, 1, 2

_log = logging.getLogger(__name__)
_route = {"on": True}                  # private A/B switch for measurements (False: every frame takes Pillow's route); no user option
_check = {"ok": None}                  # None: not verified in this process yet; False: this Pillow disagrees, route off
_check_lock = threading.Lock()
_counts = {"device": 0, "host": 0}     # frames per route since the process started (decode_stats)
_staging = {}                          # device (+ kind) -> PinnedStage of flat u8; _stage_lock held
_entropy_check = {"ok": None}          # the device entropy pass: None: not verified in this process yet; False: off


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
    g = _geom_array(geometry)                        # kept alive across the call: .ctypes.data of a temporary dangles
    n = _lib.load().hmm_jpeg_slot_bytes(g.ctypes.data, *map(int, window))
    if n <= 0:
        raise ValueError(f"window {tuple(window)} does not fit a {geometry[0]} x {geometry[1]} frame")
    return int(n)


def decode_coefs(data: bytes, geometry, window, slot: np.ndarray) -> int:
    """Entropy pass of one file into `slot` (a u8 array of at least slot_bytes) -> DECODED, UNSUPPORTED or OTHER_GEOMETRY."""
    g = _geom_array(geometry)                        # kept alive across the call (it runs without the interpreter lock, and
    st = _lib.load().hmm_jpeg_decode_coefs(data, len(data), g.ctypes.data, *map(int, window),   # another pool thread may allocate)
                                           slot.ctypes.data, slot.nbytes)
    if st < 0:
        _lib.check(st, "hmm_jpeg_decode_coefs")
    return int(st)


def entropy_mode(entropy: Optional[str] = None) -> str:
    """Where the Huffman pass runs: `entropy` when given, else HMM_JPEG_ENTROPY (read at call time), else "host"."""
    mode = entropy if entropy is not None else (os.environ.get("HMM_JPEG_ENTROPY") or "host")
    if mode not in ("host", "device"):
        raise ValueError(f"entropy / HMM_JPEG_ENTROPY must be 'host' or 'device', not {mode!r}")
    return mode


def entropy_slot_bytes(file_bytes: int) -> int:
    """Bytes of a bitstream slot for a file of `file_bytes` bytes."""
    return int(_lib.load().hmm_jpeg_entropy_slot_bytes(int(file_bytes)))


def prepare_entropy(data: bytes, geometry, slot: np.ndarray) -> int:
    """The host's share of the device entropy route: one file into the bitstream slot `slot` (a 16-byte aligned u8 array of at
    least entropy_slot_bytes(len(data))) -> DECODED, UNSUPPORTED ("not by this route") or OTHER_GEOMETRY."""
    g = _geom_array(geometry)
    st = _lib.load().hmm_jpeg_prepare_entropy(data, len(data), g.ctypes.data, slot.ctypes.data, slot.nbytes)
    if st < 0:
        _lib.check(st, "hmm_jpeg_prepare_entropy")
    return int(st)


def entropy_workspace_bytes(geometry, n: int, bitslot_stride: int) -> int:
    """Workspace bytes of decode_coefs_device for n frames of `geometry` whose bitstream slots are bitslot_stride apart."""
    g = _geom_array(geometry)
    return max(int(_lib.load().hmm_jpeg_entropy_workspace_bytes(g.ctypes.data, int(n), int(bitslot_stride))), 16)


def decode_coefs_device(bitslots: torch.Tensor, geometry, window, coef_slots: torch.Tensor, status: torch.Tensor,
                        workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bitslots (n, stride) u8 on the GPU -> coef_slots (n, >= slot_bytes) u8 and status (n, 2) int32 (status, rounds), on the
    current stream.  Slots whose status is not DECODED hold nothing usable.  workspace: a u8 tensor of at least
    entropy_workspace_bytes(geometry, n, stride) that calls on one stream may share; allocated here when not given."""
    lib = _lib.load()
    g = _geom_array(geometry)
    n = bitslots.shape[0]
    ws = workspace if workspace is not None else torch.empty(entropy_workspace_bytes(geometry, n, bitslots.stride(0)),
                                                             dtype=torch.uint8, device=bitslots.device)
    _lib.check(lib.hmm_jpeg_decode_coefs_device(bitslots.data_ptr(), n, bitslots.stride(0), g.ctypes.data, *map(int, window),
                                                coef_slots.data_ptr(), coef_slots.stride(0), status.data_ptr(), ws.data_ptr(),
                                                ws.numel(), _lib.stream_ptr()), "hmm_jpeg_decode_coefs_device")
    return status


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


def _slots_equal(device_slot: np.ndarray, host_slot: np.ndarray) -> bool:
    return bool(np.array_equal(device_slot, host_slot))


def entropy_route_ok(data: bytes, dev) -> bool:
    """May frames take the device entropy pass in this process?  The first time, `data` (a supported JPEG without restart
    interval) goes through it and its coefficient slot is compared with the host pass's; the answer is kept for the process."""
    if _entropy_check["ok"] is not None:
        return bool(_entropy_check["ok"])
    with _check_lock:
        if _entropy_check["ok"] is None:
            geometry = parse(data)
            if geometry is None:
                return False
            window = (0, 0, geometry[0], geometry[1])
            slot = np.zeros(slot_bytes(geometry, window), dtype=np.uint8)
            bits = torch.zeros(entropy_slot_bytes(len(data)), dtype=torch.uint8)
            if prepare_entropy(data, geometry, bits.numpy()) != DECODED or decode_coefs(data, geometry, window, slot) != DECODED:
                return False                             # nothing to compare: the next call decides
            with torch.cuda.device(dev):
                got = torch.empty(1, slot.nbytes, dtype=torch.uint8, device=dev)
                status = decode_coefs_device(bits.to(dev)[None], geometry, window, got,
                                             torch.empty(1, 2, dtype=torch.int32, device=dev)).cpu()
                ok = int(status[0, 0]) == DECODED and _slots_equal(got[0].cpu().numpy(), slot)
            if not ok:
                _log.warning("hippomm_amd.jpeg: the device entropy pass disagrees with the host entropy pass; "
                             "the Huffman pass stays on the host in this process")
            _entropy_check["ok"] = ok
    return bool(_entropy_check["ok"])


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


def _pinned_slots(dev, nbytes: int, kind: str = ""):
    """The pinned staging buffer of `dev` (at least nbytes), once its previous upload has left it.  Caller holds _stage_lock.
    kind: "" coefficient slots, "bits" bitstream slots."""
    ent = stage(_staging, str(dev) + kind, (max(nbytes, 1 << 20),))
    ent.wait()                                       # the previous call's upload has left the buffer
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


def _entropy_on_device(jobs, plan, datas, geoms, up, dev, pool) -> set:
    """The device entropy pass for the frames of `jobs` it takes, into their coefficient slots in `up` -> the frames it decoded.
    One upload of the bitstream slots, one call per (geometry, window) group, one read-back of the status words."""
    first = next((j[2] for j in jobs if geoms[j[2]][5] == 0), None)
    if first is None or not entropy_route_ok(datas[first], dev):
        return set()
    layout, total = [], 0                            # per group: (offset of its bitstream slots, their stride)
    for g5, crop, idx, off, sb in plan:
        stride = max(entropy_slot_bytes(len(datas[i])) for i in idx)
        layout.append((total, stride))
        total += stride * len(idx)
    ent = _pinned_slots(dev, total, "bits")
    host = ent.host

    def prep(job):
        i, g5, at, stride = job
        st = prepare_entropy(datas[i], g5, host[at:at + stride]) if geoms[i][5] == 0 else UNSUPPORTED
        if st != DECODED:
            host[at:at + 4] = 0                      # no magic word: the kernel leaves the frame at once
        return st
    pjobs = [(i, g5, at + k * stride, stride) for (g5, crop, idx, off, sb), (at, stride) in zip(plan, layout) for k, i in enumerate(idx)]
    prepared = list(pool.map(prep, pjobs)) if pool and len(pjobs) > 1 else [prep(j) for j in pjobs]
    bits = torch.empty(total, dtype=torch.uint8, device=dev)
    bits.copy_(ent.pinned[:total], non_blocking=True)
    ent.mark()
    status = torch.empty(len(pjobs), 2, dtype=torch.int32, device=dev)
    row = 0
    for (g5, crop, idx, off, sb), (at, stride) in zip(plan, layout):
        decode_coefs_device(bits[at:at + stride * len(idx)].view(len(idx), stride), g5, crop,
                            up[off:off + sb * len(idx)].view(len(idx), sb), status[row:row + len(idx)])
        row += len(idx)
    status = status.cpu()
    return {j[0] for k, j in enumerate(pjobs) if prepared[k] == DECODED and int(status[k, 0]) == DECODED}


def _decode_many(srcs: Sequence, dev, window=None, entropy: Optional[str] = None, info: dict = None) -> Tuple[list, list, int]:
    """-> (per source: an (h, w, 3) uint8 tensor on `dev` or None, per source: the exception Pillow raised or None, frames
    decoded on the device).  The work of decode_jpeg, without raising; the current stream is used.  `info`, when given,
    receives "entropy_device": the frames whose Huffman pass ran on the GPU."""
    from . import preprocess as pp
    mode = entropy_mode(entropy)
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
        host_all = ent.host if ent else None

        def entropy(job):
            g5, crop, i, off, sb = job
            return decode_coefs(datas[i], g5, crop, host_all[off:off + sb])

        jobs = [(g5, crop, i, off + k * sb, sb) for g5, crop, idx, off, sb in plan for k, i in enumerate(idx)]
        up = torch.empty(total, dtype=torch.uint8, device=dev) if total else None
        by_kernel = _entropy_on_device(jobs, plan, datas, geoms, up, dev, pool) if mode == "device" and jobs else set()
        if info is not None:
            info["entropy_device"] = len(by_kernel)
        todo = [j for j in jobs if j[2] not in by_kernel] if by_kernel else jobs
        status = list(pool.map(entropy, todo)) if pool and len(todo) > 1 else [entropy(j) for j in todo]
        on_dev = {i: True for i in by_kernel}
        on_dev.update({j[2]: st == DECODED for j, st in zip(todo, status)})
        if total:
            if not by_kernel:
                up.copy_(ent.pinned[:total], non_blocking=True)
            else:                                    # only the slots the host pass filled: the kernel's are in place
                for j, st in zip(todo, status):
                    if st == DECODED:
                        up[j[3]:j[3] + j[4]].copy_(ent.pinned[j[3]:j[3] + j[4]], non_blocking=True)
            ent.mark()
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
                stats: dict = None, entropy: Optional[str] = None) -> Union[torch.Tensor, List[torch.Tensor]]:
    """Image files (paths or bytes) -> uint8 RGB on the device, each equal to ``np.asarray(Image.open(p).convert("RGB"))``
    (cut to ``window`` = (x0, y0, w, h) when given).  Returns an (n, h, w, 3) tensor when every frame has one size, else a list
    of (h, w, 3) tensors, in the order of `sources`.  Files this decoder does not take are decoded by Pillow on the host and
    uploaded; a file Pillow cannot open raises Pillow's error (the first in order).  `stats`, when given, receives the number
    of frames per route ("device", "host").  `entropy`: where the Huffman pass of the device route runs, "host" or "device";
    None reads HMM_JPEG_ENTROPY (default "host").  With "device", `stats` also receives "entropy_device", the frames whose
    Huffman pass ran on the GPU; pixels, errors and routes are the same either way.  Safe to call from several threads."""
    dev = torch.device(device) if device is not None else _lib.require_gpu()
    srcs = list(sources)
    if not srcs:
        return torch.empty(0, 0, 0, 3, dtype=torch.uint8, device=dev)
    mode, info = entropy_mode(entropy), {}
    results, errors, n_dev = _decode_many(srcs, dev, window, mode, info)
    for exc in errors:
        if exc is not None:
            raise exc
    if stats is not None:
        stats.update(device=n_dev, host=len(srcs) - n_dev)
        if mode == "device":
            stats["entropy_device"] = info.get("entropy_device", 0)
    if len({tuple(r.shape) for r in results}) == 1:
        return torch.stack(results)
    return results
