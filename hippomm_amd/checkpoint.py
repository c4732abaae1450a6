"""Formation checkpoints: the reference's file, written with its two large encodings formed ON THE GPU (opt-in), and a loader
that returns what was saved.

The reference writes one checkpoint per video it forms (hippomm/core/hippocampal_memory.py:1269-1270 -> ``_save_checkpoint``,
:1486-1524): ``json.dump({'video_id', 'memories': [...], 'timestamp'}, f, indent=2)``, every memory the dict of
``ShortTermMemory.to_dict`` (:56-92) with each feature block replaced by ``base64(np.array(v.tolist()).tobytes())`` (:1506) --
the fp32 block widened to float64, flattened, no shape and no dtype in the text -- and every segment's raw waveform as
``audio_data.tolist()`` (:81-82), one sample per three lines of text.  That file is kept byte for byte.  What this module adds:

* ``features_base64``    a feature block as that base64 text, encoded on the device (``hmm_base64_encode_device``);
* ``checkpoint_bytes`` / ``save_checkpoint(matrices="device")``  the whole file with the feature blocks through ``features_base64``
                         and the 2-D waveforms through the matrix writer of the event files (``hmm_json_write_matrix_device`` at
                         ``close_indent=8``) -- from the resident ``AudioTrack`` with no upload when one is handed over.  The file
                         is streamed piece by piece: the device route never holds more than one segment's text on the host;
* ``load_checkpoint``    the memories of such a file, with the waveforms cut out of the text before ``json.loads`` sees them and
                         the feature blocks back in the shape and dtype they were saved from (a deliberate deviation, see there);
* ``_save_checkpoint`` / ``save_short_term_buffer`` / ``_load_checkpoint``  drop-ins for assignment on the reference's class.

``matrices="host"`` is the reference's own expression and needs no GPU.
"""
from __future__ import annotations

import base64
import json
import logging
import os
import time
import uuid
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, Iterator, List, Mapping, Optional, Tuple

import numpy as np

from .event_store import (_cuda_tensor, _device_lock, _device_stages, _device_text_agrees, _host_library, _on_host)

_log = logging.getLogger(__name__)

FEATURE_DIM = 1024                   # HMM_FEATURE_DIM: the loader's row width
WAVEFORM_CLOSE_INDENT = 8            # where the "]" of a memory's "audio_data" sits in the file
_DTYPE_F32, _DTYPE_F64, _DTYPE_U8 = 0, 1, 2                       # HMM_BASE64_DTYPE_*
_REPORT_WORDS = 5                    # HMM_BASE64_REPORT_WORDS: status, offset, inexact, values, reserved
KINDS = ("features", "waveform")
_route = {k: True for k in KINDS}    # False: that kind is written by the host expression
_check = {k: None for k in KINDS}    # None: not compared yet in this process; False: the comparison failed, the route is off
_counts = {"features_device": 0, "features_host": 0, "waveform_resident": 0, "waveform_upload": 0, "waveform_host": 0}


def _bump(counts: dict, key: str) -> None:
    counts[key] += 1
    _counts[key] += 1


def checkpoint_stats() -> dict:
    """Pieces written per route and kind since the process started."""
    return dict(_counts)


@dataclass
class SequenceSegment:
    """The reference's ``SequenceSegment`` (:35-42), field for field."""
    start_time: float
    end_time: float
    frames: Optional[List[str]] = None
    audio_data: Optional[np.ndarray] = None
    frame_times: Optional[List[float]] = None


@dataclass
class ShortTermMemory:
    """The reference's ``ShortTermMemory`` (:45-54), field for field: what ``load_checkpoint`` returns."""
    features: Dict[str, Any]
    content: Dict[str, Any]
    timestamp: float
    source_time: float
    modalities: List[str]
    segment_info: SequenceSegment
    transcription: List[Dict[str, Any]]


def _getter(obj):
    return (lambda k, d=None: obj.get(k, d)) if isinstance(obj, Mapping) else (lambda k, d=None: getattr(obj, k, d))


# ---- the reference's expressions, on the host ----
def _features_base64_host(v) -> str:
    """``_numpy_to_base64(np.array(to_dict's value))`` (:59, :1506, :310).  A CUDA tensor is read back first."""
    v = _on_host(v)
    return base64.b64encode(np.array(v.tolist() if isinstance(v, np.ndarray) else v).tobytes()).decode("utf-8")


def _content_dict(content) -> dict:
    out = {}
    for k, v in content.items():
        if k == "audio" and isinstance(v, dict):
            v = v.copy()
            if isinstance(v.get("data"), np.ndarray):
                v["data"] = v["data"].tolist()
        out[k] = v
    return out


def _memory_dict(memory, feature_entry, waveform_entry) -> dict:
    """The dict of ``ShortTermMemory.to_dict`` in its key order, from such an object or a mapping with its fields;
    ``feature_entry(k, v)`` and ``waveform_entry(a)`` say what stands for a feature block and for a waveform."""
    get = _getter(memory)
    seg = _getter(get("segment_info"))
    segment = {"start_time": seg("start_time"), "end_time": seg("end_time"), "frames": seg("frames"), "frame_times": seg("frame_times")}
    if seg("audio_data") is not None:
        segment["audio_data"] = waveform_entry(seg("audio_data"))
    return {"features": {k: feature_entry(k, v) for k, v in get("features").items()}, "content": _content_dict(get("content")),
            "timestamp": get("timestamp"), "source_time": get("source_time"), "modalities": get("modalities"),
            "segment_info": segment, "transcription": get("transcription")}


def _host_object(video_id, memories, timestamp) -> dict:
    return {"video_id": video_id,
            "memories": [_memory_dict(m, lambda k, v: _features_base64_host(v), lambda a: np.asarray(_on_host(a)).tolist()) for m in memories],
            "timestamp": timestamp}


# ---- the device routes ----
def _float_block(a) -> bool:
    """What the device encoder takes: a non-empty fp32 / fp64 numpy array or CUDA tensor of any shape."""
    if _cuda_tensor(a):
        import torch
        return a.numel() > 0 and a.dtype in (torch.float32, torch.float64)
    return isinstance(a, np.ndarray) and a.size > 0 and a.dtype in (np.float32, np.float64)


def _device_of(a, device):
    import torch
    from . import _lib as L
    dev = a.device if _cuda_tensor(a) else (torch.device(device) if device is not None else L.require_gpu())
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _upload_bytes(b: np.ndarray, dev):
    """A 1-D uint8 array -> a fresh device tensor (allocator-aligned), through pinned staging.  Call with ``_device_lock`` held."""
    import torch
    from ._pinned import stage
    n = b.shape[0]
    up = stage(_device_stages, ("up", dev.index), (n,))
    up.wait()
    up.host[:n] = b
    raw = torch.empty(n, dtype=torch.uint8, device=dev)
    raw.copy_(up.pinned[:n], non_blocking=True)
    up.mark()
    return raw


def _upload(a: np.ndarray, dev):
    """An fp32 / fp64 numpy array -> a flat device tensor of its dtype.  Call with ``_device_lock`` held."""
    import torch
    a = np.ascontiguousarray(a)
    return _upload_bytes(a.reshape(-1).view(np.uint8), dev).view(torch.float64 if a.dtype == np.float64 else torch.float32)


def _download(t, n: int, what: str, dev) -> np.ndarray:
    """The first n bytes of a device uint8 tensor -> a view of the pinned staging buffer `what` (valid until the next call that uses
    it).  Synchronises the current stream.  Call with ``_device_lock`` held."""
    import torch
    from ._pinned import stage
    down = stage(_device_stages, (what, dev.index), (n,))
    down.pinned[:n].copy_(t[:n], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return down.host[:n]


def _base64_device(a, dev) -> bytes:
    import torch
    from . import _lib as L
    lib = L.load()
    with torch.cuda.device(dev), _device_lock:
        m = a.detach().contiguous().reshape(-1) if _cuda_tensor(a) else _upload(a, dev)      # a contiguous tensor is read where it lies
        n = lib.hmm_base64_encoded_length(8 * m.numel())
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        L.check(lib.hmm_base64_encode_device(m.data_ptr(), _DTYPE_F64 if m.dtype == torch.float64 else _DTYPE_F32, m.numel(), out.data_ptr(), n,
                                             L.stream_ptr()), "hmm_base64_encode_device")
        return _download(out, n, "b64", dev).tobytes()


def _settle(kind: str, agrees) -> bool:
    """The once-per-process comparison of `kind`: True when the device route may answer."""
    if _check[kind] is None:
        ok = bool(agrees())
        if not ok:
            _log.warning("hippomm_amd.checkpoint: the device route for %s disagrees with the host expression; "
                         "the host expression writes them in this process", kind)
        _check[kind] = ok
    return _check[kind]


def features_base64(a, device=None, stats: dict = None) -> bytes:
    """The bytes of ``base64.b64encode(np.array(a.tolist()).tobytes())`` -- what a checkpoint holds for the feature block `a`
    (:1506) -- encoded ON THE GPU (``hmm_base64_encode_device``: fp32 is widened to float64 there, 24 source bytes -> 32
    characters per thread, one launch).

    a: a non-empty fp32 / fp64 numpy array or CUDA tensor of any shape; a tensor is read where it lies (made contiguous if it is
    not), an array goes up through pinned staging.  Any other input takes the reference's expression on the host.  The first
    block a process encodes this way is compared with that expression; on a mismatch the route is off for the process, a
    warning is logged and the host answers.  `stats`, when given, receives "route": "device" or "host"."""
    def by_host() -> bytes:
        _counts["features_host"] += 1
        if stats is not None:
            stats["route"] = "host"
        return _features_base64_host(a).encode("ascii")

    if not _float_block(a) or not _route["features"] or _check["features"] is False:
        return by_host()
    text = _base64_device(a, _device_of(a, device))
    if not _settle("features", lambda: text == _features_base64_host(a).encode("ascii")):
        return by_host()
    _counts["features_device"] += 1
    if stats is not None:
        stats["route"] = "device"
    return text


def _waveform_device(m, dev) -> np.ndarray:
    """A (rows, cols) fp32 / fp64 device tensor -> its text at ``WAVEFORM_CLOSE_INDENT`` as a view of pinned staging."""
    import torch
    from . import _lib as L
    lib = L.load()
    rows, cols = int(m.shape[0]), int(m.shape[1])
    cap = lib.hmm_json_matrix_text_bound(rows, cols, WAVEFORM_CLOSE_INDENT)
    ws_bytes = lib.hmm_json_write_matrix_device_workspace_bytes(rows, cols)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.int64, device=dev)
    written = torch.empty(1, dtype=torch.int64, device=dev)
    L.check(lib.hmm_json_write_matrix_device(m.data_ptr(), 1 if m.dtype == torch.float64 else 0, rows, cols, WAVEFORM_CLOSE_INDENT, out.data_ptr(),
                                             cap, written.data_ptr(), ws.data_ptr(), ws_bytes, L.stream_ptr()), "hmm_json_write_matrix_device")
    return _download(out, int(written.item()), "waveform", dev)


def _waveform_host(a) -> bytes:
    """``json.dumps(a.tolist(), indent=2)`` as it stands inside the file: every line after the first 8 spaces deeper."""
    return json.dumps(np.asarray(_on_host(a)).tolist(), indent=2).replace("\n", "\n" + " " * WAVEFORM_CLOSE_INDENT).encode("ascii")


def _matrix2d(a) -> bool:
    return _float_block(a) and len(a.shape) == 2


def _resident_span(a, track, span) -> Optional[Tuple[int, int]]:
    """(start, stop) when the track's own samples may stand for the memory's waveform `a`, else None."""
    if track is None or span is None or _cuda_tensor(a):
        return None
    shape = getattr(track, "source_shape", None)
    if shape is None or not (len(shape) == 1 or (len(shape) == 2 and shape[1] == 1)) or track.source_dtype not in (np.float32, np.float64):
        return None
    start, stop = int(span[0]), int(span[1])
    if not 0 <= start < stop <= track.n_samples or tuple(a.shape) != (stop - start, 1) or a.dtype != track.source_dtype:
        return None
    return start, stop


def _waveform_piece(a, track, span, device, counts):
    """The text of one memory's 2-D waveform: bytes, or a view of pinned staging that holds until the next piece is formed."""
    import torch
    if not _route["waveform"] or _check["waveform"] is False:
        _bump(counts, "waveform_host")
        return _waveform_host(a)
    resident = _resident_span(a, track, span)
    dev = track.device if resident else _device_of(a, device)
    with torch.cuda.device(dev), _device_lock:
        if resident and getattr(track, "pcm", False):                # int16 samples: x * 2^-15 in float64 is the array's value, exactly
            m = track.samples[resident[0]:resident[1]].to(torch.float64).mul_(2.0 ** -15).view(-1, 1)
        elif resident:
            m = track.samples[resident[0]:resident[1]].view(-1, 1)
        elif _cuda_tensor(a):
            m = a.detach().contiguous()
        else:
            m = _upload(a, dev).view(a.shape)
        text = _waveform_device(m, dev)
        rows = int(a.shape[0])
        if not _settle("waveform", lambda: _device_text_agrees(text.tobytes(), np.asarray(_on_host(a[0])), np.asarray(_on_host(a[rows - 1])), rows,
                                                                WAVEFORM_CLOSE_INDENT)):
            _bump(counts, "waveform_host")
            return _waveform_host(a)
    _bump(counts, "waveform_resident" if resident else "waveform_upload")
    return text


def _pieces(video_id, memories, timestamp, matrices, audio_track, audio_spans, device, stats) -> Iterator[Any]:
    """The file as a sequence of bytes-like pieces.  A piece may be a view of a pinned staging buffer: use it before the next."""
    if matrices not in ("host", "device"):
        raise ValueError(f"matrices must be 'host' or 'device', not {matrices!r}")
    memories = list(memories)
    if matrices == "host":
        yield json.dumps(_host_object(video_id, memories, timestamp), indent=2).encode("ascii")
        return
    if audio_spans is not None and len(audio_spans) != len(memories):
        raise ValueError(f"audio_spans has {len(audio_spans)} entries for {len(memories)} memories")
    salt = uuid.uuid4().hex
    holes = {}                                                       # the quoted token -> a function giving the piece
    counts = {k: 0 for k in _counts}

    def feature_piece(v):
        one = {}
        text = features_base64(v, device, one)
        counts["features_" + one["route"]] += 1
        return b'"' + text + b'"'

    dicts = []
    for i, memory in enumerate(memories):
        span = audio_spans[i] if audio_spans is not None else None

        def feature_entry(k, v, i=i):
            if not _float_block(v):
                _bump(counts, "features_host")
                return _features_base64_host(v)
            token = f"@@hmm_ckpt_{i}_{len(holes)}_{salt}@@"
            holes[f'"{token}"'] = lambda v=v: feature_piece(v)
            return token

        def waveform_entry(a, i=i, span=span):
            if not _matrix2d(a):                                     # 1-D, empty, integer, a list: json's own text
                return np.asarray(_on_host(a)).tolist()
            token = f"@@hmm_ckpt_{i}_{len(holes)}_{salt}@@"
            holes[f'"{token}"'] = lambda a=a: _waveform_piece(a, audio_track, span, device, counts)
            return token

        dicts.append(_memory_dict(memory, feature_entry, waveform_entry))
    text = json.dumps({"video_id": video_id, "memories": dicts, "timestamp": timestamp}, indent=2)
    if any(text.count(quoted) != 1 for quoted in holes):             # the token also occurs in the memories' own strings
        yield json.dumps(_host_object(video_id, memories, timestamp), indent=2).encode("ascii")
        return
    pos = 0
    for at, quoted in sorted((text.index(quoted), quoted) for quoted in holes):
        yield text[pos:at].encode("ascii")
        yield holes[quoted]()
        pos = at + len(quoted)
    yield text[pos:].encode("ascii")
    if stats is not None:
        stats.update(counts)


def checkpoint_bytes(video_id, memories, timestamp, matrices: str = "host", audio_track=None, audio_spans=None, device=None,
                     stats: dict = None) -> bytes:
    """The exact text of ``json.dump({'video_id': video_id, 'memories': [...], 'timestamp': timestamp}, f, indent=2)`` as
    ``_save_checkpoint`` writes it (:1500-1516): each memory the dict of ``ShortTermMemory.to_dict()`` with every feature block
    replaced by its base64 text.  memories: objects or mappings with the fields of ``ShortTermMemory`` (``segment_info`` likewise).

    matrices="host": the reference's expression.  matrices="device": feature blocks that are non-empty fp32 / fp64 numpy arrays
    or CUDA tensors go through ``features_base64``; a 2-D, non-empty fp32 / fp64 ``segment_info.audio_data`` goes through the
    device matrix writer at ``close_indent=8``; everything else -- strings, frame lists, transcriptions (``ensure_ascii`` is on),
    1-D waveforms, anything unusual -- through ``json.dumps(indent=2)`` with one unique token per hole.  A token that also occurs
    in the memories' own strings sends the whole file through the host expression.

    audio_track (an ``AudioTrack``) with audio_spans (one ``(start, stop)`` in samples, or None, per memory): that memory's text is
    formed from the resident samples ``[start, stop)`` with no upload -- only when the track's source was ``(n,)`` or ``(n, 1)``
    float32 / float64 and the memory's ``audio_data`` has shape ``(stop - start, 1)`` in that dtype; the caller vouches that it IS
    that slice.  Otherwise the memory's own array is uploaded.

    The first feature block and the first waveform a process writes on the device are compared with the host expression (the
    waveform by its first and last row); on a mismatch that kind is written by the host from then on and a warning is logged.
    `stats`, when given, receives the pieces per route and kind: "features_device", "features_host", "waveform_resident",
    "waveform_upload", "waveform_host"."""
    return b"".join(bytes(p) for p in _pieces(video_id, memories, timestamp, matrices, audio_track, audio_spans, device, stats))


def _write_file(path, video_id, memories, timestamp, matrices, audio_track, audio_spans, device, stats) -> None:
    if matrices == "host":
        with open(path, "w") as f:                                   # the reference's own lines (:1511-1516)
            json.dump(_host_object(video_id, list(memories), timestamp), f, indent=2)
        return
    if audio_track is not None and audio_spans is None:
        from .audio_track import spans_of
        audio_spans = spans_of([_SegmentTimes(m) for m in memories], audio_track.sample_rate)
    with open(path, "wb") as f:
        for piece in _pieces(video_id, memories, timestamp, matrices, audio_track, audio_spans, device, stats):
            f.write(piece)                                           # a waveform's text leaves from the pinned staging view


class _SegmentTimes:
    def __init__(self, memory):
        seg = _getter(_getter(memory)("segment_info"))
        self.start_time, self.end_time = seg("start_time"), seg("end_time")


def save_checkpoint(storage_dir, video_id, memories, matrices: str = "host", audio_track=None, audio_spans=None, now=time.time,
                    device=None, stats: dict = None) -> Optional[str]:
    """``_save_checkpoint`` (:1486-1524): writes ``<storage_dir>/checkpoints/checkpoint_{video_id}_{int(now())}.json`` and returns
    its path as ``str``; on any error logs it and returns None, as the reference does.  ``now`` is called twice, as there: for the
    file's name, then for its 'timestamp'.

    The file is streamed: the pieces of ``checkpoint_bytes`` go to the file as they are formed, a waveform's text straight from the
    pinned staging view, so the device route holds one segment's text on the host at a time and never the whole file.  With an
    `audio_track` and no `audio_spans` the spans are ``audio_track.spans_of`` of the memories' segments."""
    try:
        memories = list(memories)
        checkpoint_dir = Path(storage_dir) / "checkpoints"
        checkpoint_dir.mkdir(parents=True, exist_ok=True)
        path = checkpoint_dir / f"checkpoint_{video_id}_{int(now())}.json"
        _write_file(path, video_id, memories, now(), matrices, audio_track, audio_spans, device, stats)
        _log.info("Successfully saved checkpoint to %s", path)
        return str(path)
    except Exception as e:
        _log.error("Error saving checkpoint: %s", e)
        _log.exception("Full traceback:")
        return None


def _save_checkpoint(self, video_id, memories) -> Optional[str]:
    """Drop-in for ``HippocampalMemory._save_checkpoint``: the same file on the device route.  Optional attributes of the object:
    ``checkpoint_matrices`` ("device" unless set), ``checkpoint_audio_track`` (the video's resident ``AudioTrack``)."""
    return save_checkpoint(self.storage_dir, video_id, memories, getattr(self, "checkpoint_matrices", "device"),
                           getattr(self, "checkpoint_audio_track", None))


def save_short_term_buffer(self, temp_dir=None) -> Dict[str, str]:
    """Drop-in for ``HippocampalMemory.save_short_term_buffer`` (:1526-1560): the same serialisation under
    ``short_term_{video_id}_{int(time.time())}.json``; errors propagate, as there."""
    if temp_dir is None:
        temp_dir = os.path.join(self.storage_dir, "temp_short_term")
    os.makedirs(temp_dir, exist_ok=True)
    file_paths = {}
    for video_id, memories in self.short_term_buffer.items():
        temp_file = os.path.join(temp_dir, f"short_term_{video_id}_{int(time.time())}.json")
        _write_file(temp_file, video_id, list(memories), time.time(), getattr(self, "checkpoint_matrices", "device"), None, None, None, None)
        file_paths[video_id] = temp_file
    return file_paths


# ---- loading ----
def _block_from_doubles(f64: np.ndarray):
    """The loader's shape and dtype rule on a 1-D float64 array."""
    if f64.size == 0 or f64.size % FEATURE_DIM:
        return f64
    with np.errstate(all="ignore"):
        f32 = f64.astype(np.float32)
        exact = np.array_equal(f32.astype(np.float64).view(np.uint64), f64.view(np.uint64))
    return (f32 if exact else f64).reshape(-1, FEATURE_DIM)


def _features_from_base64_host(s: str):
    data = base64.b64decode(s)
    if len(data) % 8:
        return np.frombuffer(data, dtype=np.float32)                 # not whole doubles: not this writer's; the reference's own reading
    return _block_from_doubles(np.frombuffer(data, dtype=np.float64))


def _features_from_base64_device(s: str, dev):
    """The decode kernel's fp32 block as a CUDA tensor when it applies (strictly valid text, a multiple of 1024 values, every one
    narrowing exactly); else what the host gives."""
    import torch
    from . import _lib as L
    lib = L.load()
    try:
        raw = s.encode("ascii")
    except UnicodeEncodeError:
        return _features_from_base64_host(s)
    n_values = len(raw) // 4 * 3 // 8
    if len(raw) % 4 or n_values == 0 or n_values % FEATURE_DIM:
        return _features_from_base64_host(s)
    with torch.cuda.device(dev), _device_lock:
        text = _upload_bytes(np.frombuffer(raw, np.uint8), dev)
        out = torch.empty(n_values, dtype=torch.float32, device=dev)
        report = torch.empty(_REPORT_WORDS, dtype=torch.int64, device=dev)
        L.check(lib.hmm_base64_decode_device(text.data_ptr(), len(raw), _DTYPE_F32, out.data_ptr(), n_values, report.data_ptr(), L.stream_ptr()),
                "hmm_base64_decode_device")
        status, _, inexact, values, _ = (int(v) for v in report.cpu().numpy().view(np.uint64))
    if status != 0 or inexact or values != n_values:
        return _features_from_base64_host(s)
    return out.view(-1, FEATURE_DIM)


def _cut_waveforms(raw: bytes) -> Tuple[bytes, dict]:
    """`raw` with every ``[[numbers], ...]`` span outside string literals replaced by a unique token -> (text, {token: span's
    bytes}).  None in place of the dict when the spans cannot be cut (no library, or a token collides): `raw` comes back whole."""
    lib = _host_library()
    if lib is None:
        return raw, None
    from .event_store import _find_by_host
    spans = _find_by_host(raw, 1)
    salt = uuid.uuid4().hex
    pieces, cut, pos = [], {}, 0
    for i, (begin, end, _, _) in enumerate(spans):
        token = f"@@hmm_ckpt_{i}_{salt}@@"
        cut[token] = (begin, end)
        pieces += [raw[pos:begin], b'"' + token.encode() + b'"']
        pos = end
    pieces.append(raw[pos:])
    reduced = b"".join(pieces)
    if any(reduced.count(t.encode()) != 1 for t in cut):
        return raw, None
    return reduced, cut


def load_checkpoint(path, features: str = "host", device=None) -> List[ShortTermMemory]:
    """The memories of a checkpoint file, as ``ShortTermMemory`` objects (this module's dataclass, the reference's fields).

    The ``[[numbers], ...]`` spans of the text are found outside string literals (``hmm_json_find_matrices``) and cut out before
    ``json.loads`` runs: the one under a memory's ``segment_info.audio_data`` is dropped -- ``audio_data`` is None, as in the
    reference (:1463) -- so the waveforms, nearly all of the file, are never parsed; a span anywhere else is parsed on its own and
    put back.  Every feature string is decoded as float64, which is what the writer encoded (:1506):

    * a count that is a multiple of 1024 becomes ``(-1, 1024)``; when every value narrows to fp32 exactly (features written from
      fp32 always do) the block is fp32 -- with features="device" a CUDA tensor, decoded and narrowed by
      ``hmm_base64_decode_device`` -- and float64 otherwise;
    * any other count stays a 1-D float64 array;
    * bytes that are not whole doubles are read as the reference reads them.

    DEVIATION from the reference, on purpose: its ``_load_checkpoint`` (:1438-1484) reads the float64 bytes as float32 with no
    shape (``_base64_to_numpy``, :312-318), so a saved ``(2, 1024)`` block comes back as ``(4096,)`` float32 whose every other
    value is the low half of a double, and consolidation drops every such row.  This loader returns what was saved.

    Raises on a file it cannot read; ``_load_checkpoint`` is the drop-in that logs and returns None."""
    if features not in ("host", "device"):
        raise ValueError(f"features must be 'host' or 'device', not {features!r}")
    raw = Path(path).read_bytes()
    reduced, cut = _cut_waveforms(raw)
    data = json.loads(reduced)
    dev = _device_of(None, device) if features == "device" else None

    def put_back(v):
        if isinstance(v, str) and cut and v in cut:
            return json.loads(raw[cut[v][0]:cut[v][1]])
        if isinstance(v, dict):
            return {k: put_back(x) for k, x in v.items()}
        if isinstance(v, list):
            return [put_back(x) for x in v]
        return v

    memories = []
    for mem in data["memories"]:
        seg = mem["segment_info"]
        seg.pop("audio_data", None)                                  # not parsed, not kept
        mem = put_back(mem)
        feats = {k: (_features_from_base64_device(s, dev) if dev is not None else _features_from_base64_host(s))
                 for k, s in mem["features"].items()}
        seg = mem["segment_info"]
        memories.append(ShortTermMemory(
            features=feats, content=mem["content"], timestamp=mem["timestamp"], source_time=mem["source_time"], modalities=mem["modalities"],
            segment_info=SequenceSegment(start_time=seg["start_time"], end_time=seg["end_time"], frames=seg.get("frames"),
                                         frame_times=seg.get("frame_times"), audio_data=None),
            transcription=mem["transcription"]))
    _log.info("Successfully loaded %d memories from checkpoint %s", len(memories), path)
    return memories


def _load_checkpoint(self, checkpoint_path) -> Optional[List[ShortTermMemory]]:
    """Drop-in for ``HippocampalMemory._load_checkpoint``: ``load_checkpoint`` (see its deviation), None on any error.  Optional
    attribute of the object: ``checkpoint_features`` ("host" unless set)."""
    try:
        return load_checkpoint(checkpoint_path, getattr(self, "checkpoint_features", "host"))
    except Exception as e:
        _log.error("Error loading checkpoint %s: %s", checkpoint_path, e)
        _log.exception("Full traceback:")
        return None
