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

Encoding goes the other way (hippomm_amd/csrc/jpeg_encode.hip): ``encode_jpeg`` turns uint8 frames, resident or on the host,
into complete baseline files on the GPU -- colour transform, chroma downsampling, islow forward DCT, quantisation, the Huffman
pass, padding and byte stuffing -- each, byte for byte, the file ``Image.fromarray(x).save(buf, "JPEG", quality=q,
subsampling=s)`` writes.  The same self-check guards it, and a frame the kernel does not report as encoded is encoded by Pillow.

``encode_jpeg(..., return_decoded=True)`` also returns what ``decode_jpeg`` would make of those files, without the files: the
quantised blocks and tables the encoder leaves on the device are all a decoder recovers from a file (hmm_jpeg_encoded_pixels in
jpeg.hip).  ``segmentation.save_frames(cache=, tower_inputs=)`` hands those pixels to the readers' caches.
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


# ---------------------------------------------------------------------------------------------------------------------------------
# encoding (hippomm_amd/csrc/jpeg_encode.hip): frames -> baseline files, byte for byte Pillow's
# ---------------------------------------------------------------------------------------------------------------------------------
ENCODED, ENCODE_OVERFLOW = 0, 1
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
CHANNEL_ORDER = {"RGB": 0, "BGR": 1}
ENCODE_SLOT_AT_BOUND = 1 << 20                 # geometries whose proven bound is at most this get slots of the bound itself
_QT_BYTES = 256                                # two tables of 64 uint16 in front of the header in the uploaded table block

_encode_route = {"on": True}                   # private A/B switch for measurements (False: Pillow encodes); no user option
_encode_check = {"ok": None}                   # None: not verified in this process yet; False: this Pillow disagrees, route off
_encode_counts = {"device": 0, "host": 0, "overflow": 0}
_encode_tables = {}                            # (device, geometry, quality) -> u8 tensor [quantisation tables | header]


def encode_geometry(h: int, w: int, channels: int, subsampling: str = "4:2:0") -> Tuple[int, ...]:
    """The geometry words of frames of (h, w, channels): sampling 1 x 1 for grey, whatever `subsampling` says."""
    hs, vs = SAMPLING[subsampling] if channels == 3 else (1, 1)
    return (int(w), int(h), int(channels), hs, vs, 0)


def encode_header(geometry, quality: int) -> Tuple[bytes, np.ndarray]:
    """-> (the bytes FF D8 .. SOS of every file of `geometry` at `quality`, the two quantisation tables (2, 64) uint16 in
    natural order).  Host only."""
    g = _geom_array(geometry)
    head = np.zeros(1024, dtype=np.uint8)
    qt = np.zeros((2, 64), dtype=np.uint16)
    n = _lib.load().hmm_jpeg_encode_header(g.ctypes.data, int(quality), head.ctypes.data, head.nbytes, qt.ctypes.data)
    if n < 0:
        _lib.check(n, "hmm_jpeg_encode_header")
    return head[:n].tobytes(), qt


def encode_bound(geometry) -> int:
    """A proven upper bound on the bytes of one file of `geometry`; 0: the device route does not take the geometry."""
    g = _geom_array(geometry)
    return int(_lib.load().hmm_jpeg_encode_bound(g.ctypes.data))


def encode_workspace_bytes(geometry, n: int) -> int:
    g = _geom_array(geometry)
    return max(int(_lib.load().hmm_jpeg_encode_workspace_bytes(g.ctypes.data, int(n))), 16)


def encode_tables(geometry, quality: int, dev) -> torch.Tensor:
    """The quantisation tables and the header of (geometry, quality) on `dev`, uploaded once per process."""
    key = (str(dev), tuple(int(v) for v in geometry[:5]), int(quality))
    block = _encode_tables.get(key)
    if block is None:
        head, qt = encode_header(geometry, quality)
        host = np.concatenate([qt.reshape(-1).view(np.uint8), np.frombuffer(head, dtype=np.uint8)])
        block = _encode_tables[key] = torch.from_numpy(host).to(dev)
    return block


def encode_device(frames: torch.Tensor, geometry, quality: int, channel_order: str, out: torch.Tensor, status: torch.Tensor,
                  workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames (n, h, w, channels) u8, contiguous, on the GPU -> the file of frame i in out[i] (out: (n, stride) u8) and
    status (n, 2) int32 = (ENCODED or ENCODE_OVERFLOW, bytes), on the current stream; nothing is synchronised.  workspace: a u8
    tensor of at least encode_workspace_bytes(geometry, n); allocated here when not given."""
    lib = _lib.load()
    g = _geom_array(geometry)
    n = frames.shape[0]
    tables = encode_tables(geometry, quality, frames.device)
    ws = workspace if workspace is not None else torch.empty(encode_workspace_bytes(geometry, n), dtype=torch.uint8,
                                                             device=frames.device)
    _lib.check(lib.hmm_jpeg_encode(frames.data_ptr(), n, g.ctypes.data, int(geometry[2]), CHANNEL_ORDER[channel_order],
                                   tables.data_ptr(), tables.data_ptr() + _QT_BYTES, tables.numel() - _QT_BYTES, out.data_ptr(),
                                   out.stride(0), status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()),
               "hmm_jpeg_encode")
    return status


def encoded_pixels_workspace_bytes(geometry, n: int, window) -> int:
    g = _geom_array(geometry)
    return max(int(_lib.load().hmm_jpeg_encoded_pixels_workspace_bytes(g.ctypes.data, int(n), *map(int, window))), 16)


def encoded_pixels_device(encode_workspace: torch.Tensor, n: int, geometry, quality: int, window, out: torch.Tensor,
                          workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decoded pixels of the n frames an ``encode_device`` call of the same geometry and quality has just encoded, from the
    workspace tensor that call used (given to it as ``workspace=``): out (n, h, w, 3) u8 = the window (x0, y0, w, h) of
    ``Image.open(file_i).convert("RGB")``, on the current stream, which must be the stream of the encode.  Nothing is
    synchronised and the encoder's workspace is only read.  workspace: a u8 tensor of at least
    encoded_pixels_workspace_bytes(geometry, n, window); allocated here when not given."""
    if int(n) == 0:
        return out                                   # an empty tensor has no address to hand over
    lib = _lib.load()
    g = _geom_array(geometry)
    x0, y0, w, h = map(int, window)
    tables = encode_tables(geometry, quality, encode_workspace.device)
    ws = workspace if workspace is not None else torch.empty(encoded_pixels_workspace_bytes(geometry, n, window), dtype=torch.uint8,
                                                             device=encode_workspace.device)
    _lib.check(lib.hmm_jpeg_encoded_pixels(encode_workspace.data_ptr(), int(n), g.ctypes.data, tables.data_ptr(), x0, y0, w, h,
                                           out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "hmm_jpeg_encoded_pixels")
    return out


def pillow_encode(frame: np.ndarray, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "RGB") -> bytes:
    """The file the device route reproduces: Pillow's, for an (h, w, 3) frame in `channel_order` or an (h, w) grey frame."""
    from PIL import Image
    buf = io.BytesIO()
    if frame.ndim == 3 and frame.shape[2] == 1:
        frame = frame[..., 0]
    if frame.ndim == 2:
        Image.fromarray(np.ascontiguousarray(frame), "L").save(buf, "JPEG", quality=int(quality))
    else:
        rgb = frame[..., ::-1] if channel_order == "BGR" else frame
        Image.fromarray(np.ascontiguousarray(rgb), "RGB").save(buf, "JPEG", quality=int(quality), subsampling=subsampling)
    return buf.getvalue()


def encode_stats() -> dict:
    """Frames encoded per route since the process started: "device", "host" (Pillow) and, among the latter, "overflow" (frames
    the kernel reported as not fitting their slot)."""
    return dict(_encode_counts)


def _encode_slot_bytes(geometry) -> int:
    """Bytes of an output slot: the proven bound where that is small; else the raw frame's size plus the header, which a file
    exceeds only for noise at the highest qualities -- such a frame is reported as overflowing and Pillow encodes it."""
    bound = encode_bound(geometry)
    if bound <= ENCODE_SLOT_AT_BOUND:
        return bound
    return min(bound, geometry[0] * geometry[1] * geometry[2] + 4096)


def _as_batches(frames) -> List[Tuple[object, List[int]]]:
    """frames -> [(a (n, h, w, c) uint8 numpy array or CUDA tensor, the positions of its frames in the result)], validated."""
    def check(a):
        if isinstance(a, torch.Tensor):
            if a.dtype != torch.uint8:
                raise TypeError(f"encode_jpeg takes uint8 frames, got a {a.dtype} tensor")
            if not a.is_cuda:
                raise TypeError("encode_jpeg takes numpy arrays or CUDA tensors, got a CPU tensor")
        elif isinstance(a, np.ndarray):
            if a.dtype != np.uint8:
                raise TypeError(f"encode_jpeg takes uint8 frames, got a {a.dtype} array")
        else:
            raise TypeError(f"encode_jpeg takes uint8 numpy arrays or CUDA tensors, got {type(a).__name__}")
        shape = tuple(a.shape)
        if len(shape) == 2:
            a = a[None, :, :, None]
        elif len(shape) == 3 and shape[2] == 3:
            a = a[None]
        elif not (len(shape) == 4 and shape[3] in (1, 3)):
            raise ValueError(f"encode_jpeg takes frames of shape (h, w, 3), (n, h, w, 3), (h, w) or (n, h, w, 1), got {shape}")
        if not (1 <= a.shape[1] <= 65535 and 1 <= a.shape[2] <= 65535):
            raise ValueError(f"encode_jpeg: a frame of {a.shape[2]} x {a.shape[1]} pixels (sides of 1..65535 are encoded)")
        return a

    if not isinstance(frames, (list, tuple)):
        a = check(frames)
        return [(a, list(range(a.shape[0])))]
    groups, at = {}, 0                               # (on the device?, its device, h, w, channels) -> [(positions, frames)]
    for f in frames:
        a = check(f)
        key = (isinstance(a, torch.Tensor), str(a.device) if isinstance(a, torch.Tensor) else "", *a.shape[1:])
        groups.setdefault(key, []).append((list(range(at, at + a.shape[0])), a))
        at += a.shape[0]
    out = []
    for key, members in groups.items():
        stack = torch.cat if key[0] else np.concatenate
        out.append((members[0][1] if len(members) == 1 else stack([a for _, a in members]), [i for where, _ in members for i in where]))
    return out


def _decoded_from_files(files: Sequence[bytes], dev, window) -> List[torch.Tensor]:
    """The existing decode of the bytes (decode_jpeg's work, per frame), raising the first error."""
    results, errors, _ = _decode_many(list(files), dev, window)
    for exc in errors:
        if exc is not None:
            raise exc
    return results


def _encode_batch(batch, quality: int, subsampling: str, channel_order: str, dev, slot_bytes: Optional[int],
                  want_decoded: bool = False, window=None):
    """One geometry -> (the files, how many the device encoded, how many overflowed their slot, the decoded frames -- an
    (n, h, w, 3) tensor or a list of (h, w, 3) tensors; None unless want_decoded --, how many of them never left the device)."""
    n, h, w, c = batch.shape
    geometry = encode_geometry(h, w, c, subsampling)
    resident = isinstance(batch, torch.Tensor)
    host = None if resident else batch
    crop = (0, 0, w, h) if window is None else tuple(int(v) for v in window)
    if want_decoded and not (crop[0] >= 0 and crop[1] >= 0 and crop[2] > 0 and crop[3] > 0 and crop[0] + crop[2] <= w
                             and crop[1] + crop[3] <= h):
        raise ValueError(f"window {tuple(window)} does not fit a {w} x {h} frame")

    def by_pillow(i):
        nonlocal host
        if host is None:
            host = batch.cpu().numpy()
        return pillow_encode(host[i], quality, subsampling, channel_order)

    def all_by_pillow():
        files = [by_pillow(i) for i in range(n)]
        return files, 0, 0, (_decoded_from_files(files, batch.device if resident else dev, window) if want_decoded else None), 0

    if not _encode_route["on"] or _encode_check["ok"] is False or encode_bound(geometry) == 0:
        return all_by_pillow()
    dev = batch.device if resident else dev
    stride = int(slot_bytes) if slot_bytes else (_encode_slot_bytes(geometry) + 15) // 16 * 16
    pixels = None
    with torch.cuda.device(dev):
        if resident:
            frames = batch.contiguous()              # a contiguous tensor is encoded where it lies
        else:
            with _stage_lock:
                ent = _pinned_slots(dev, batch.size, "frames")
                ent.host[:batch.size].reshape(batch.shape)[...] = batch
                frames = torch.empty(batch.shape, dtype=torch.uint8, device=dev)
                frames.view(-1).copy_(ent.pinned[:batch.size], non_blocking=True)
                ent.mark()
        out = torch.empty(n, stride, dtype=torch.uint8, device=dev)
        ws = torch.empty(encode_workspace_bytes(geometry, n), dtype=torch.uint8, device=dev)
        status = encode_device(frames, geometry, quality, channel_order, out, torch.empty(n, 2, dtype=torch.int32, device=dev), ws)
        if want_decoded and _route["on"] and _check["ok"] is not False:
            # the quantised blocks are still in ws: the pixels a decoder would recover from the files, before the files exist.
            # Queued behind the encode, ahead of the read-back; kept only for frames whose file is the device's (below).
            pixels = encoded_pixels_device(ws, n, geometry, quality, crop, torch.empty(n, crop[3], crop[2], 3, dtype=torch.uint8, device=dev))
        status = status.cpu()
        done = [i for i in range(n) if int(status[i, 0]) == ENCODED]
        sizes = [int(status[i, 1]) for i in done]
        packed = torch.cat([out[i, :size] for i, size in zip(done, sizes)]).cpu().numpy() if done else np.zeros(0, np.uint8)
    files, at = [None] * n, 0
    for i, size in zip(done, sizes):
        files[i] = packed[at:at + size].tobytes()
        at += size
    if done and _encode_check["ok"] is None:
        with _check_lock:
            if _encode_check["ok"] is None:
                ok = files[done[0]] == by_pillow(done[0])
                if not ok:
                    _log.warning("hippomm_amd.jpeg: the device JPEG encoder disagrees with this Pillow's encoder; "
                                 "every frame is encoded by Pillow in this process")
                _encode_check["ok"] = ok
    if _encode_check["ok"] is False:
        return all_by_pillow()
    for i in range(n):
        if files[i] is None:
            files[i] = by_pillow(i)
    if not want_decoded:
        return files, len(done), n - len(done), None, 0
    # the device decoder is guarded as everywhere: its first frame in this process is compared with Pillow's decode
    if pixels is None or not done or not route_ok(files[done[0]], dev):
        return files, len(done), n - len(done), _decoded_from_files(files, dev, window), 0
    if len(done) == n:
        return files, n, 0, pixels, n
    rest = sorted(set(range(n)) - set(done))
    decoded = list(pixels)
    for i, frame in zip(rest, _decoded_from_files([files[i] for i in rest], dev, window)):   # Pillow wrote these files
        decoded[i] = frame
    return files, len(done), n - len(done), decoded, len(done)


def encode_jpeg(frames, quality: int = 95, subsampling: str = "4:2:0", channel_order: str = "RGB", device=None,
                stats: dict = None, _slot_bytes: Optional[int] = None, return_decoded: bool = False, window=None):
    """Frames -> baseline JPEG files, encoded on the GPU; element i is, byte for byte, what
    ``Image.fromarray(rgb_i).save(buf, "JPEG", quality=quality, subsampling=subsampling)`` writes ("L" mode for grey input): the
    whole file, FF D8 to FF D9, no ``optimize``, no ``progressive``, no extra markers.

    frames: a uint8 numpy array or CUDA tensor of shape (h, w, 3), (n, h, w, 3), (h, w) or (n, h, w, 1) (grey), or a list of
    such arrays, which may differ in size and are grouped by geometry; the result follows the list's order.  A CUDA tensor is encoded where it lies; numpy frames
    are uploaded through the package's pinned staging.  The read-back is the lengths, then one copy of the used bytes.
    quality: 1..100.  subsampling: "4:4:4", "4:2:2" or "4:2:0"; ignored for grey.  channel_order: "RGB", or "BGR" (cv2 frames): the
    kernel swaps.  Other dtypes raise ``TypeError``; other shapes, a side of 0 or above 65535 and other options ``ValueError``.

    The first frame a process encodes on the device is compared with Pillow's bytes for the same input; on a mismatch (another
    Pillow or libjpeg build) the device route is off for the process, a warning is logged and Pillow encodes.  A frame the kernel
    does not report as encoded (its file would not fit its slot: noise at the highest qualities in large frames) is encoded by
    Pillow too, so every call returns Pillow's bytes.  `stats`, when given, receives the frames per route: "device", "host" and,
    among the latter, "overflow".

    return_decoded=True: -> (files, decoded), where decoded[i] is, bit for bit, ``decode_jpeg([files[i]], window=window)[0]`` --
    Pillow's decode of the file just written, uint8 RGB (grey: R = G = B) on the device, cut to ``window`` = (x0, y0, w, h) when
    given (it must fit every frame: ``ValueError``) -- without the file being read or even written: the quantised blocks the
    encoder left on the device and its tables are all a decoder recovers from the file (hmm_jpeg_encoded_pixels: dequantise, islow
    IDCT, upsampling, colour).  One (n, h, w, 3) tensor when the sizes agree, else a list, as decode_jpeg returns.  Frames whose
    file Pillow wrote (the route off, the first-frame check failed, a slot overflowed) take their pixels from the existing decode
    of those bytes, and so do all frames when the device decoder's own first-frame check (``route_ok``) does not pass.  `stats`
    then also receives "decoded_resident": the frames whose pixels never left the device."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"encode_jpeg: quality must be an integer in 1..100, not {quality!r}")
    if subsampling not in SAMPLING:
        raise ValueError(f"encode_jpeg: subsampling must be one of {sorted(SAMPLING)}, not {subsampling!r}")
    if channel_order not in CHANNEL_ORDER:
        raise ValueError(f"encode_jpeg: channel_order must be 'RGB' or 'BGR', not {channel_order!r}")
    batches = _as_batches(frames)
    total = sum(len(where) for _, where in batches)
    files, on_device, overflow = [None] * total, 0, 0
    decoded, resident, whole = [None] * total, 0, None
    if total:
        dev = torch.device(device) if device is not None else _lib.require_gpu()
        for batch, where in batches:
            if not where:
                continue
            got, n_dev, n_over, pixels, n_res = _encode_batch(batch, int(quality), subsampling, channel_order, dev, _slot_bytes,
                                                              return_decoded, window)
            for i, data in zip(where, got):
                files[i] = data
            if return_decoded:
                if isinstance(pixels, torch.Tensor) and where == list(range(total)):
                    whole = pixels                   # one geometry, in order: the kernel's output is the result
                for i, frame in zip(where, pixels):
                    decoded[i] = frame
                resident += n_res
            on_device += n_dev
            overflow += n_over
    _encode_counts["device"] += on_device
    _encode_counts["host"] += total - on_device
    _encode_counts["overflow"] += overflow
    if stats is not None:
        stats.update(device=on_device, host=total - on_device, overflow=overflow)
        if return_decoded:
            stats["decoded_resident"] = resident
    if not return_decoded:
        return files
    if not total:
        return files, torch.empty(0, 0, 0, 3, dtype=torch.uint8)
    if whole is not None:
        return files, whole
    return files, (torch.stack(decoded) if len({tuple(d.shape) for d in decoded}) == 1 else decoded)
