"""memory_store event files: fast path beside the reference's JSON.

The reference stores every consolidated event as ``events/<video_id>/<event_id>.json`` written by
``json.dump(event.to_dict(), f, indent=2)`` (hippomm/core/hippocampal_memory.py:110-133, :331-335) and reads
it back with ``json.load`` + ``np.array(list)`` (:369-395): one Python float per line, ~20 bytes of text per
stored fp32, float64 arrays after loading.  That file format is the contract with the unmodified
``load_theta_event`` and is kept byte for byte.  What this module adds:

* ``save_event``     writes the same JSON **plus** an fp32 ``.npy`` sidecar per feature matrix and a manifest
                     holding the JSON's size and mtime;
* ``load_event_features``  returns the fp32 matrices from the sidecars when they are fresh (same size+mtime
                     as recorded), else parses the JSON once and (re)writes the sidecars.  Values are
                     identical either way: the JSON holds fp32 values printed as doubles, and
                     ``float32(float64(text))`` round-trips them exactly;
* ``build_event_store``  reads ``event_index.json`` (:338-346) and returns an ``EventStore`` with one modality's
                     matrices of all events resident in HBM, ready for ``top_k_per_event``;
* ``refresh_event_store``  appends the events the index gained since to that resident store, and drops the ones it lost.

* ``matrix_json_bytes`` / ``event_json_bytes`` / ``save_event(matrices="device")``  write the text of the feature matrices ON THE
                     GPU (opt-in; the same bytes), so that embeddings that are still on the device reach the file without
                     becoming Python floats.

* ``parse_matrix_device`` / ``parse_event_features(matrices="device")`` / ``build_event_store(parse="device")``  read the feature
                     matrices back from that text ON THE GPU (opt-in; the same bits), so that a cold store without sidecars
                     reaches HBM without a host fp32 matrix in between.

* ``find_matrices_device`` / ``parse_event_features(matrices="device", find="device")`` / ``build_event_store(parse="device",
                     find="device")``  also decide ON THE GPU where those matrices lie in the text (opt-in; the same spans), so
                     that the host no longer walks the file before the parser's kernels start.

Nothing here touches the GPU except ``build_event_store``, ``refresh_event_store`` and the ``matrices="device"`` / ``parse="device"`` routes.
"""
from __future__ import annotations

import json
import logging
import os
import re
import sys
import threading
import uuid
from pathlib import Path
from typing import Any, Dict, Iterable, Mapping, Optional, Tuple

import numpy as np

SIDECAR_VERSION = 1
_EVENT_KEYS = ("frames", "frame_times", "frame_captions", "audio_times", "audio_transcription",
               "holistic_audio_transcription", "summary", "start_time", "end_time")


def event_to_dict(event: Any) -> Dict[str, Any]:
    """The dict ``ThetaEvent.to_dict`` builds (:110-133), from a ThetaEvent-like object or a mapping with the
    same fields.  Keys ending in ``_times`` inside ``features`` move to ``feature_times``; arrays become lists."""
    get = (lambda k, d=None: event.get(k, d)) if isinstance(event, Mapping) else (lambda k, d=None: getattr(event, k, d))
    features_dict, times_dict = {}, {}
    for modality, features in get("features").items():
        (times_dict if modality.endswith("_times") else features_dict)[modality] = np.asarray(features).tolist()
    return _event_dict(get, features_dict, times_dict)


def _event_dict(get, features_dict, times_dict) -> Dict[str, Any]:
    """The keys of ``ThetaEvent.to_dict`` in its order, around the two feature dicts."""
    return {
        "features": features_dict, "feature_times": times_dict,
        "frames": get("frames"), "frame_times": get("frame_times"), "frame_captions": get("frame_captions"),
        "audio_times": get("audio_times"), "audio_transcription": get("audio_transcription"),
        "holistic_audio_transcription": get("holistic_audio_transcription"), "summary": get("summary"),
        "start_time": get("start_time"), "end_time": get("end_time"),
    }


def event_json_text(event: Any, fast: bool = True) -> str:
    """Exactly the text ``save_theta_event`` writes (:334-335): ``json.dumps(event.to_dict(), indent=2)``.

    ``indent`` forces Python's pure-Python encoder (~1 us per float; 0.6 s for a 600-frame event).  With ``fast`` the
    2-D feature matrices -- 99.9 % of the text -- are written by the library (``_matrix_text``: the same bytes -- same
    ``float.__repr__`` digits and notation, same separators and indentation); everything else, and any matrix that is not a non-empty list of equally long rows of Python floats (EVERY row is
    checked), goes through ``json.dumps(indent=2)`` itself.  The hole a matrix leaves in the outer text is a fresh random
    token; if the token turns up anywhere else in the text the whole event goes through ``json.dumps(indent=2)``."""
    d = event.to_dict() if hasattr(event, "to_dict") else event_to_dict(event)
    if not fast or not isinstance(d.get("features"), dict):
        return json.dumps(d, indent=2)
    feats, holes, salt = dict(d["features"]), {}, uuid.uuid4().hex
    for i, (modality, rows) in enumerate(list(feats.items())):
        if (isinstance(rows, list) and rows and isinstance(rows[0], list) and rows[0]
                and all(type(r) is list and len(r) == len(rows[0]) and set(map(type, r)) == {float} for r in rows)):   # every value a float
            token = f"@@hmm_matrix_{i}_{salt}@@"
            holes[f'"{token}"'] = rows
            feats[modality] = token
    text = json.dumps(dict(d, features=feats), indent=2)
    if any(text.count(quoted) != 1 for quoted in holes):         # the token also occurs in the event's own strings
        return json.dumps(d, indent=2)
    for quoted, rows in holes.items():
        # features -> modality -> row -> value: rows sit at indent 6, values at indent 8, the closing bracket at indent 4
        text = text.replace(quoted, _matrix_text(rows), 1)
    return text


def _host_library():
    """The library for its HOST-side JSON routines, or None when it is not built / too old: reading and saving an event file is
    plain host work and keeps working on json alone (the GPU paths have no such fallback and raise)."""
    from . import _lib as L
    try:
        return L.load()
    except (L.HippoMMHipError, AttributeError, OSError):
        return None


def _matrix_text(rows, native: bool = True) -> str:
    """``json.dumps(rows, indent=2)`` of a non-empty list of equally long lists of floats whose closing bracket sits at indent 4.
    ``native``: written by the library (``hmm_json_write_matrix_f64``: float.__repr__ digits and notation, byte for byte --
    tests/test_cpu_event_store.py); otherwise row by row with the C encoder of ``json`` and re-indented."""
    lib = _host_library() if native else None
    if lib is not None:
        import ctypes as C
        from . import _lib as L
        m = np.array(rows, dtype=np.float64)
        cap = lib.hmm_json_matrix_text_bound(m.shape[0], m.shape[1], 4)
        buf = C.create_string_buffer(cap)
        n = C.c_size_t(0)
        L.check(lib.hmm_json_write_matrix_f64(m.ctypes.data_as(C.c_void_p), m.shape[0], m.shape[1], 4, C.cast(buf, C.c_void_p), cap, C.byref(n)),
                "hmm_json_write_matrix_f64")
        return C.string_at(buf, n.value).decode("ascii")          # only the written bytes (buf.raw would copy the whole bound first)
    body = ",\n".join("      [\n        " + json.dumps(r)[1:-1].replace(", ", ",\n        ") + "\n      ]" for r in rows)
    return "[\n" + body + "\n    ]"


def _sidecar_paths(json_path: Path, modality: str) -> Tuple[Path, Path]:
    stem = json_path.with_suffix("")
    return Path(f"{stem}.{modality}.f32.npy"), Path(f"{stem}.sidecar.json")


def _as_feature_matrix(a) -> np.ndarray:
    """One rule for both paths (JSON parse and sidecar): fp32, C-contiguous, and the reference's shape fix-up when a
    matrix arrives as (1024, N) (:413-417) -- so that an event loads with the same shape whichever path serves it."""
    if _cuda_tensor(a):                                  # a matrix the device parser left in HBM: the same rule, no host trip
        import torch
        if a.dim() > 1 and a.shape[1] != 1024 and a.shape[0] == 1024:
            a = a.T
        return a.to(torch.float32).contiguous()
    a = np.asarray(a)
    if a.ndim > 1 and a.shape[1] != 1024 and a.shape[0] == 1024:
        a = a.T
    return np.ascontiguousarray(a, dtype=np.float32)


def _write_sidecars(json_path: Path, features: Mapping[str, np.ndarray]) -> None:
    st = json_path.stat()
    shapes = {}
    for modality, arr in features.items():
        a = _as_feature_matrix(arr)
        npy, _ = _sidecar_paths(json_path, modality)
        tmp = npy.with_suffix(".tmp.npy")
        np.save(tmp, a)
        os.replace(tmp, npy)
        shapes[modality] = list(a.shape)
    _, manifest = _sidecar_paths(json_path, "x")
    tmp = manifest.with_suffix(".tmp")
    tmp.write_text(json.dumps({"version": SIDECAR_VERSION, "json_size": st.st_size, "json_mtime_ns": st.st_mtime_ns,
                               "modalities": shapes}))
    os.replace(tmp, manifest)


def save_event(event: Any, json_path, write_sidecars: bool = True, matrices: str = "host", device=None, stats: dict = None) -> Path:
    """Write the reference's JSON (byte-identical) and, optionally, the fp32 sidecars next to it.

    matrices="device": the text of the feature matrices is written on the GPU (``event_json_bytes``) -- the file is the same
    bytes; features may then be CUDA tensors, and the sidecars come from one fp32 read-back of each.  `device` and `stats` as in
    ``event_json_bytes``."""
    json_path = Path(json_path)
    json_path.parent.mkdir(parents=True, exist_ok=True)
    if matrices == "host":
        json_path.write_text(event_json_text(event))
    else:
        json_path.write_bytes(event_json_bytes(event, matrices, device, stats))
    if write_sidecars:
        feats = event.features if hasattr(event, "features") else event["features"]
        _write_sidecars(json_path, {m: _on_host(f, fp32=True) for m, f in feats.items() if not m.endswith("_times")})
    return json_path


# ---- the feature matrices as JSON text, written on the device (csrc/event_json.hip) ----
_log = logging.getLogger(__name__)
MAX_CLOSE_INDENT = 32                # HMM_JSON_MAX_INDENT
_device_route = {"on": True}         # False: every matrix is written by the host writer
_device_check = {"ok": None}         # None: not compared yet in this process; False: the comparison failed, the route is off
_device_counts = {"device": 0, "host": 0}
_device_lock = threading.Lock()
_device_stages: dict = {}            # (what, device index) -> PinnedStage


def matrix_json_stats() -> dict:
    """Matrices written per route by ``matrix_json_bytes`` since the process started: "device" and "host"."""
    return dict(_device_counts)


def _cuda_tensor(a) -> bool:
    torch = sys.modules.get("torch")             # a tensor cannot exist before torch is imported
    return torch is not None and isinstance(a, torch.Tensor) and a.is_cuda


def _on_host(a, fp32: bool = False):
    """A CUDA tensor as a numpy array (one read-back; as fp32 when asked); anything else as it is."""
    if not _cuda_tensor(a):
        return a
    import torch
    return (a.detach().to(torch.float32) if fp32 else a.detach()).cpu().numpy()


def _is_device_matrix(a) -> bool:
    """What the device writer takes: a 2-D, non-empty fp32 / fp64 numpy array or CUDA tensor."""
    if _cuda_tensor(a):
        import torch
        return a.dim() == 2 and a.numel() > 0 and a.dtype in (torch.float32, torch.float64)
    return isinstance(a, np.ndarray) and a.ndim == 2 and a.size > 0 and a.dtype in (np.float32, np.float64)


def _matrix_bytes_host(m: np.ndarray, close_indent: int) -> bytes:
    """The host writer (``hmm_json_write_matrix_f64``) on a numpy matrix, at any indentation."""
    import ctypes as C
    from . import _lib as L
    lib = L.load()
    m = np.ascontiguousarray(m, dtype=np.float64)
    cap = lib.hmm_json_matrix_text_bound(m.shape[0], m.shape[1], close_indent)
    buf = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    L.check(lib.hmm_json_write_matrix_f64(m.ctypes.data_as(C.c_void_p), m.shape[0], m.shape[1], close_indent, C.cast(buf, C.c_void_p), cap,
                                          C.byref(n)), "hmm_json_write_matrix_f64")
    return C.string_at(buf, n.value)


def _row_text(row, close_indent: int) -> bytes:
    """One row as ``json.dumps`` writes it inside the matrix: from the newline in front of its indentation to its "]"."""
    pad = " " * (close_indent + 4)
    return ("\n" + " " * (close_indent + 2) + "[" + ",".join("\n" + pad + json.dumps(float(v)) for v in row)
            + "\n" + " " * (close_indent + 2) + "]").encode("ascii")


def _device_text_agrees(text: bytes, first_row, last_row, rows: int, close_indent: int) -> bool:
    """The self-check's comparison: does `text` open with ``json.dumps``'s first row and close with its last?"""
    head = b"[" + _row_text(first_row, close_indent)
    tail = (b"," if rows > 1 else b"[") + _row_text(last_row, close_indent) + b"\n" + b" " * close_indent + b"]"
    return text.startswith(head) and text.endswith(tail)


def _matrix_bytes_device(features, close_indent: int, dev) -> bytes:
    """One launch sequence, one 8-byte read-back of the length, one read-back of exactly that many bytes through pinned staging."""
    import torch
    from . import _lib as L
    from ._pinned import stage
    lib = L.load()
    with torch.cuda.device(dev), _device_lock:
        if _cuda_tensor(features):
            m = features.detach().contiguous()               # a contiguous tensor is read where it lies
        else:
            a = np.ascontiguousarray(features)
            up = stage(_device_stages, ("up", dev.index), (a.nbytes,))
            up.wait()
            up.host[:a.nbytes] = a.reshape(-1).view(np.uint8)
            raw = torch.empty(a.nbytes, dtype=torch.uint8, device=dev)
            raw.copy_(up.pinned[:a.nbytes], non_blocking=True)
            up.mark()
            m = raw.view(torch.float64 if a.dtype == np.float64 else torch.float32).view(a.shape)
        rows, cols = int(m.shape[0]), int(m.shape[1])
        cap = lib.hmm_json_matrix_text_bound(rows, cols, close_indent)
        ws_bytes = lib.hmm_json_write_matrix_device_workspace_bytes(rows, cols)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        ws = torch.empty(max(ws_bytes, 8) // 8, dtype=torch.int64, device=dev)
        written = torch.empty(1, dtype=torch.int64, device=dev)
        L.check(lib.hmm_json_write_matrix_device(m.data_ptr(), 1 if m.dtype == torch.float64 else 0, rows, cols, close_indent, out.data_ptr(),
                                                 cap, written.data_ptr(), ws.data_ptr(), ws_bytes, L.stream_ptr()),
                "hmm_json_write_matrix_device")
        n = int(written.item())
        down = stage(_device_stages, ("down", dev.index), (n,))
        down.pinned[:n].copy_(out[:n], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return down.host[:n].tobytes()


def matrix_json_bytes(features, close_indent: int = 4, device=None, stats: dict = None) -> bytes:
    """A feature matrix as the text ``json.dumps(features.tolist(), indent=2)`` has for it when its closing bracket sits at
    `close_indent` spaces (4 inside an event file: what ``_matrix_text`` returns), formed ON THE GPU
    (``hmm_json_write_matrix_device``: shortest round-trip digits per value, a prefix sum over the lengths, the text put together
    in LDS) -- the values never become Python floats, nor a list.

    features: a 2-D, non-empty fp32 or fp64 numpy array or CUDA tensor (``TypeError`` / ``ValueError`` otherwise; fp32 is widened,
    as ``.tolist()`` does; a non-contiguous one is made contiguous).  A CUDA tensor is read where it lies, a numpy array is
    uploaded through pinned staging.  close_indent: 0 .. 32.  One launch sequence, one 8-byte read-back of the length, one
    read-back of exactly that many bytes.

    The first matrix a process writes this way has its first and last row compared with ``json.dumps``; on a mismatch the route
    is off for the process, a warning is logged and the host writer (``hmm_json_write_matrix_f64``) answers, as it does from then
    on.  `stats`, when given, receives "route": "device" or "host".

    Measured on one MI355X (profiles/event_json_device.json): the kernels take 51 us for 600 x 1024 fp32 and
    155 us for 3600 x 1024; ``save_event`` without sidecars 63 -> 5.7 ms at 600 rows and 435 -> 83 ms at 3600 against the host
    route, from a numpy array or a device tensor alike -- what is left is the read-back, two host copies of the text and the file
    write."""
    if not (_cuda_tensor(features) or isinstance(features, np.ndarray)):
        raise TypeError(f"matrix_json_bytes takes a numpy array or a CUDA tensor, got {type(features).__name__}")
    if len(features.shape) != 2 or features.shape[0] * features.shape[1] == 0:
        raise ValueError(f"matrix_json_bytes takes a non-empty 2-D matrix, got shape {tuple(features.shape)}")
    if not _is_device_matrix(features):
        raise TypeError(f"matrix_json_bytes takes fp32 or fp64 values, got {features.dtype}")
    if isinstance(close_indent, bool) or not isinstance(close_indent, (int, np.integer)) or not 0 <= int(close_indent) <= MAX_CLOSE_INDENT:
        raise ValueError(f"matrix_json_bytes: close_indent must be an integer in 0..{MAX_CLOSE_INDENT}, not {close_indent!r}")
    close_indent = int(close_indent)

    def by_host() -> bytes:
        _device_counts["host"] += 1
        if stats is not None:
            stats["route"] = "host"
        return _matrix_bytes_host(_on_host(features), close_indent)

    if not _device_route["on"] or _device_check["ok"] is False:
        return by_host()
    import torch
    from . import _lib as L
    # a tensor is written where it lies; `device` says where a numpy array goes
    dev = features.device if _cuda_tensor(features) else (torch.device(device) if device is not None else L.require_gpu())
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    text = _matrix_bytes_device(features, close_indent, dev)
    if _device_check["ok"] is None:
        with _device_lock:
            if _device_check["ok"] is None:
                rows = int(features.shape[0])
                ok = _device_text_agrees(text, _on_host(features[0]), _on_host(features[rows - 1]), rows, close_indent)
                if not ok:
                    _log.warning("hippomm_amd.event_store: the device JSON writer disagrees with this Python's json.dumps; "
                                 "every matrix is written by the host writer in this process")
                _device_check["ok"] = ok
    if _device_check["ok"] is False:
        return by_host()
    _device_counts["device"] += 1
    if stats is not None:
        stats["route"] = "device"
    return text


def event_json_bytes(event: Any, matrices: str = "device", device=None, stats: dict = None) -> bytes:
    """``event_json_text(event).encode("ascii")``, byte for byte -- the file ``save_theta_event`` writes.

    matrices="device": every entry of ``features`` that is a 2-D, non-empty fp32 / fp64 numpy array or CUDA tensor is written by
    ``matrix_json_bytes`` and never becomes a list (CUDA tensors are accepted on this route only).  Everything around the
    matrices goes through ``json.dumps(indent=2)`` with the unique-token holes of ``event_json_text``, and so does every other
    entry inside this same call: lists, 1-D, empty or integer arrays, and the ``*_times`` entries (lists of equally long rows of
    floats keep the host writer).  A token that also occurs in the event's own strings sends the whole event through
    ``json.dumps(indent=2)``.  The matrix bytes are spliced in as bytes.  matrices="host": ``event_json_text`` as it stands.
    `stats`, when given, receives "device" and "host": the matrices each route wrote."""
    if matrices == "host":
        return event_json_text(event).encode("ascii")
    if matrices != "device":
        raise ValueError(f"matrices must be 'host' or 'device', not {matrices!r}")
    get = (lambda k, d=None: event.get(k, d)) if isinstance(event, Mapping) else (lambda k, d=None: getattr(event, k, d))
    salt = uuid.uuid4().hex
    features_dict, times_dict, holes = {}, {}, {}                 # holes: the quoted token -> a function giving the matrix's bytes
    counts = {"device": 0, "host": 0}

    def on_device(f):
        one = {}
        text = matrix_json_bytes(f, 4, device, one)
        counts[one["route"]] += 1
        return text

    for i, (modality, f) in enumerate(get("features").items()):
        if modality.endswith("_times"):
            times_dict[modality] = np.asarray(_on_host(f)).tolist()
            continue
        token = f"@@hmm_matrix_{i}_{salt}@@"
        if _is_device_matrix(f):
            holes[f'"{token}"'] = lambda f=f: on_device(f)
            features_dict[modality] = token
            continue
        rows = np.asarray(_on_host(f)).tolist()
        if (isinstance(rows, list) and rows and isinstance(rows[0], list) and rows[0]
                and all(type(r) is list and len(r) == len(rows[0]) and set(map(type, r)) == {float} for r in rows)):
            holes[f'"{token}"'] = lambda rows=rows: _matrix_text(rows).encode("ascii")
            features_dict[modality] = token
        else:
            features_dict[modality] = rows
    text = json.dumps(_event_dict(get, features_dict, times_dict), indent=2)
    if any(text.count(quoted) != 1 for quoted in holes):         # the token also occurs in the event's own strings
        feats = {m: np.asarray(_on_host(f)).tolist() for m, f in get("features").items() if not m.endswith("_times")}
        return json.dumps(_event_dict(get, feats, times_dict), indent=2).encode("ascii")
    pieces, pos = [], 0
    for at, quoted in sorted((text.index(quoted), quoted) for quoted in holes):
        pieces += [text[pos:at].encode("ascii"), holes[quoted]()]
        pos = at + len(quoted)
    pieces.append(text[pos:].encode("ascii"))
    if stats is not None:
        stats.update(counts)
    return b"".join(pieces)


def _fresh_manifest(json_path: Path) -> Optional[dict]:
    _, manifest = _sidecar_paths(json_path, "x")
    try:
        m = json.loads(manifest.read_text())
        st = json_path.stat()
        if m.get("version") == SIDECAR_VERSION and m["json_size"] == st.st_size and m["json_mtime_ns"] == st.st_mtime_ns:
            return m
    except (OSError, ValueError, KeyError):
        pass
    return None


# ---- the feature matrices read back from JSON text on the device (csrc/event_json_parse.hip) ----
FLAGGED_CAP = 256                    # entries of the flagged list a call brings; more flagged values than that: the host route
_PARSE_OK, _FLAG_RANGE = 0, 2        # HMM_JSON_PARSE_OK, HMM_JSON_FLAG_RANGE
_JSON_NUMBER = re.compile(rb"-?(?:0|[1-9][0-9]*)(?:\.[0-9]+)?(?:[eE][+-]?[0-9]+)?")
_parse_route = {"on": True}          # False: every matrix is parsed by the host route
_parse_check = {"ok": None}          # None: not compared yet in this process; False: the comparison failed, the route is off
_parse_counts = {"device": 0, "host": 0, "json": 0}


def matrix_parse_stats() -> dict:
    """Matrices read per route by ``parse_matrix_device`` and ``parse_event_features(matrices="device")`` since the process
    started: "device", "host" (``hmm_json_parse_matrix_f32``, then uploaded) and "json" (``json.loads``)."""
    return dict(_parse_counts)


class _EventText:
    """The text of one event file for the device route: the bytes, the uint8 tensor, or both -- each made from the other at most
    once (bytes go up through pinned staging in one copy; a tensor comes down only when the host route needs the characters)."""

    def __init__(self, raw, dev):
        self.dev = dev
        self.host = raw if isinstance(raw, (bytes, bytearray, memoryview)) else None
        self.tensor = None if self.host is not None else raw

    def __len__(self):
        return len(self.host) if self.host is not None else int(self.tensor.numel())

    def on_device(self):
        """Call with ``_device_lock`` held."""
        if self.tensor is None:
            import torch
            from ._pinned import stage
            n = len(self.host)
            up = stage(_device_stages, ("text", self.dev.index), (n,))
            up.wait()
            up.host[:n] = np.frombuffer(self.host, np.uint8)
            self.tensor = torch.empty(n, dtype=torch.uint8, device=self.dev)
            self.tensor.copy_(up.pinned[:n], non_blocking=True)
            up.mark()
        return self.tensor

    def bytes_of(self, begin: int, end: int) -> bytes:
        if self.host is not None:
            return bytes(self.host[begin:end])
        return self.tensor[begin:end].cpu().numpy().tobytes()

    def all_bytes(self) -> bytes:
        """The whole text on the host; a tensor is brought down once and kept."""
        if self.host is None:
            self.host = self.tensor.cpu().numpy().tobytes()
        return self.host if isinstance(self.host, bytes) else bytes(self.host)


def _span4(span) -> Tuple[int, int, int, int]:
    """(begin, end, rows, cols) of a span given as such a tuple or as an ``hmm_json_matrix``."""
    if isinstance(span, (tuple, list)) and len(span) == 4:
        return tuple(int(v) for v in span)
    return int(span.begin), int(span.end), int(span.rows), int(span.cols)


def _matrix_by_host(span_text: bytes, rows: int, cols: int) -> Optional[np.ndarray]:
    """``hmm_json_parse_matrix_f32`` on a span that is the whole of `span_text`; None when it declines."""
    from . import _lib as L
    a = np.empty((rows, cols), np.float32)
    if L.load().hmm_json_parse_matrix_f32(span_text, 0, len(span_text), rows, cols, a.ctypes.data) != 0:
        return None
    return a


def _matrix_on_device(text: _EventText, begin: int, end: int, rows: int, cols: int, f64: bool):
    """One launch sequence and one read-back of the report (with the flagged list behind it, one copy); flagged values are
    converted by ``float(token)`` and patched in with one small copy.  -> (tensor, report words) or (None, report words) when the
    matrix must go to the host route.  Call with ``_device_lock`` held, inside ``torch.cuda.device``."""
    import torch
    from . import _lib as L
    from ._pinned import stage
    lib, dev = L.load(), text.dev
    t = text.on_device()
    out = torch.empty((rows, cols), dtype=torch.float64 if f64 else torch.float32, device=dev)
    ws_bytes = lib.hmm_json_parse_matrix_device_workspace_bytes(end - begin)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    report = torch.empty(4 + 4 * FLAGGED_CAP, dtype=torch.int64, device=dev)          # hmm_json_parse_report, then hmm_json_flagged[]
    L.check(lib.hmm_json_parse_matrix_device(t.data_ptr(), begin, end, rows, cols, 1 if f64 else 0, out.data_ptr(), report.data_ptr(),
                                             report.data_ptr() + 32, FLAGGED_CAP, ws.data_ptr(), ws_bytes, L.stream_ptr()),
            "hmm_json_parse_matrix_device")
    nbytes = report.numel() * 8
    down = stage(_device_stages, ("report", dev.index), (nbytes,))
    down.pinned[:nbytes].view(torch.int64).copy_(report, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    words = down.host[:nbytes].view(np.uint64).copy()
    n_flagged, status = int(words[1]), int(words[3])
    if status != _PARSE_OK or n_flagged > FLAGGED_CAP:
        return None, words
    if n_flagged:
        entries = words[4:4 + 4 * n_flagged].reshape(-1, 4)
        values = []
        for _, b, e, flag in entries.tolist():
            token = text.bytes_of(b, e)
            # a literal outside the double range is the host parser's to decline; a token too long for the device was not checked
            # against the grammar there
            if flag == _FLAG_RANGE or _JSON_NUMBER.fullmatch(token) is None:
                return None, words
            v = float(token)
            if v == 0.0 or v in (float("inf"), float("-inf")):
                return None, words
            values.append(v)
        packed = np.stack([entries[:, 0].astype(np.int64), np.array(values, np.float64).view(np.int64)])
        packed = torch.from_numpy(packed).to(dev)
        out.view(-1).index_copy_(0, packed[0], packed[1].view(torch.float64).to(out.dtype))      # narrowed as (float)(double)
    return out, words


def _edge_rows_agree(text: _EventText, begin: int, end: int, cols: int, out) -> bool:
    """The self-check's comparison: the first and the last row of `out`, as bits, against the host parser's (fp32;
    ``json.loads`` for fp64 and where the host parser declines)."""
    import torch
    span = text.bytes_of(begin, end)
    first_open = span.index(b"[", 1)
    last_open = span.rindex(b"[")
    for open_at, got in ((first_open, out[0]), (last_open, out[-1])):
        row = b"[" + span[open_at:span.index(b"]", open_at) + 1] + b"]"
        want = _matrix_by_host(row, 1, cols) if out.dtype == torch.float32 else None
        if want is None:
            want = np.array(json.loads(row), np.float64).astype(np.float32 if out.dtype == torch.float32 else np.float64)
        if got.cpu().numpy().tobytes() != want.reshape(-1).tobytes():
            return False
    return True


def _parse_matrix_routes(text: _EventText, span, dtype, report: dict = None):
    """One matrix of `text` as a tensor on ``text.dev`` -> (tensor, "device" | "host"), or (None, None) when the device route and
    the host route both decline it (the caller then asks ``json``).  `report`, when given, receives the device's report."""
    import torch
    begin, end, rows, cols = span
    f64 = np.dtype(dtype) == np.float64
    if _parse_route["on"] and _parse_check["ok"] is not False:
        with torch.cuda.device(text.dev), _device_lock:
            out, words = _matrix_on_device(text, begin, end, rows, cols, f64)
            if report is not None:
                report.update(n_tokens=int(words[0]), n_flagged=int(words[1]), first_bad=int(words[2]), status=int(words[3]))
            if out is not None and _parse_check["ok"] is None:
                ok = _edge_rows_agree(text, begin, end, cols, out)
                if not ok:
                    _log.warning("hippomm_amd.event_store: the device JSON parser disagrees with the host parser; "
                                 "every matrix is parsed by the host route in this process")
                _parse_check["ok"] = ok
        if out is not None and _parse_check["ok"]:
            return out, "device"
    if f64:
        return None, None                                        # fp64 has no host parser: json.loads is its other route
    a = _matrix_by_host(text.bytes_of(begin, end), rows, cols)
    if a is None:
        return None, None
    return torch.from_numpy(a).to(text.dev), "host"


def _parse_device_of(raw, device):
    import torch
    from . import _lib as L
    dev = raw.device if _cuda_tensor(raw) else (torch.device(device) if device is not None else L.require_gpu())
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def parse_matrix_device(raw, span, dtype=np.float32, device=None, stats: dict = None):
    """One feature matrix of an event file, from its JSON text to a CUDA tensor of rows x cols, converted ON THE GPU
    (``hmm_json_parse_matrix_device``: token starts counted per 4 KiB of text, a prefix sum, every token converted with integer
    arithmetic -- Eisel-Lemire on its first 19 significant digits, exact for every such literal).  fp32 gives the bits of
    ``hmm_json_parse_matrix_f32``, i.e. ``np.array(json.load(f)).astype(np.float32)``; fp64 the bits of ``np.array(json.loads(span))``.

    raw: the file as ``bytes`` (uploaded once, through pinned staging) or as a 1-D uint8 CUDA tensor that already holds it.
    span: (begin, end, rows, cols) as ``hmm_json_find_matrices`` reports a matrix (its struct is taken as well).  One launch
    sequence and one read-back of the report.  Values the device flags (a literal of more than 19 significant digits whose two
    candidates round differently, a token above 64 bytes; at most ``FLAGGED_CAP``) are converted by ``float(token)`` on the host
    and patched in with one small copy.  Any other status -- a token count that is not rows x cols, a foreign byte, a token that is
    no JSON number --, more flagged values than that, or a literal outside the double range hands the whole matrix to the host
    route: ``hmm_json_parse_matrix_f32``, then one upload (fp32 only).  Where that declines as well, ``json.loads`` of the span
    answers, with whatever shape it finds, or raises as it does.  `stats`, when given, receives "route": "device", "host" or
    "json", and the device's report ("status", "n_tokens", "n_flagged", "first_bad") when the device ran.

    The first matrix a process parses this way has its first and last row compared, as bits, with the host parser's; on a
    mismatch a warning is logged and the host route answers, as it does from then on.

    Measured on one MI355X (profiles/event_json_parse.json): the kernels take 68 us for 600 x 1024 values
    (18.5 MB of text) and 336 us for 3600 x 1024; ``parse_event_features`` 23.4 -> 9.7 ms and 163.8 -> 79.3 ms against the host
    route -- what is left is the host's span finder (7.5 / 46 ms), the file read and the upload.  The route is opt-in."""
    if not (_cuda_tensor(raw) or isinstance(raw, (bytes, bytearray, memoryview))):
        raise TypeError(f"parse_matrix_device takes bytes or a uint8 CUDA tensor, got {type(raw).__name__}")
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"parse_matrix_device gives fp32 or fp64, not {np.dtype(dtype)}")
    if _cuda_tensor(raw):
        import torch
        if raw.dtype != torch.uint8 or raw.dim() != 1 or not raw.is_contiguous():
            raise TypeError("parse_matrix_device takes a contiguous 1-D uint8 tensor")
    begin, end, rows, cols = span = _span4(span)
    if not 0 <= begin < end <= len(raw) or rows < 1 or cols < 1:
        raise ValueError(f"parse_matrix_device: span [{begin}, {end}) of {rows} x {cols} values in a text of {len(raw)} bytes")
    import torch
    text = _EventText(raw, _parse_device_of(raw, device))
    report = {}
    out, route = _parse_matrix_routes(text, span, dtype, report)
    if stats is not None:
        stats.update(report)                                     # before json is asked: it may raise
    if out is None:
        a = np.array(json.loads(text.bytes_of(begin, end))).astype(dtype)
        out, route = torch.from_numpy(np.ascontiguousarray(a)).to(text.dev), "json"
    _parse_counts[route] += 1
    if stats is not None:
        stats["route"] = route
    return out


NATIVE_MIN_VALUES = 1024        # 2-D arrays of at least this many numbers are parsed by the library, the rest by json


# ---- where the matrices lie, found in the text on the device (csrc/event_json_find.hip) ----
FIND_FIRST = 16                      # entries of the list that come back with the report, in the one read-back
FIND_CAP = 4096                      # entries the device list holds; a text with more matrices is asked again with room for all
_FIND_OK = 0                         # HMM_JSON_FIND_OK
_find_route = {"on": True}           # False: the host finder answers
_find_check = {"ok": None}           # None: not compared yet in this process; False: the comparison failed, the route is off
_find_counts = {"device": 0, "declined": 0, "host": 0}


def matrix_find_stats() -> dict:
    """Texts searched per route by ``find_matrices_device`` and ``parse_event_features(find="device")`` since the process
    started: "device", "declined" (the device declined and the host finder answered) and "host" (the route is off)."""
    return dict(_find_counts)


def _find_by_host(raw, min_values: int):
    """``hmm_json_find_matrices`` -> [(begin, end, rows, cols)] in document order."""
    import ctypes as C
    from . import _lib as L
    lib = L.load()
    n, cap = C.c_int(0), FIND_FIRST
    while True:
        spans = (C.c_size_t * (4 * cap))()
        L.check(lib.hmm_json_find_matrices(bytes(raw), len(raw), min_values, C.cast(spans, C.c_void_p), cap, C.byref(n)), "hmm_json_find_matrices")
        if n.value <= cap:
            break
        cap = n.value
    return [tuple(spans[4 * i:4 * i + 4]) for i in range(n.value)]


def _find_on_device(text: _EventText, min_values: int):
    """One launch sequence and one read-back: the report with the first ``FIND_FIRST`` entries behind it; a second copy only when
    there are more.  -> (list or None when the device declined, report words).  Call with ``_device_lock`` held, inside
    ``torch.cuda.device``."""
    import torch
    from . import _lib as L
    from ._pinned import stage
    lib, dev = L.load(), text.dev
    t = text.on_device()
    ws_bytes = lib.hmm_json_find_matrices_device_workspace_bytes(len(text))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    cap = FIND_CAP
    while True:
        out = torch.empty(4 + 4 * cap, dtype=torch.int64, device=dev)                 # hmm_json_find_report, then hmm_json_matrix[]
        L.check(lib.hmm_json_find_matrices_device(t.data_ptr(), len(text), min_values, out.data_ptr() + 32, cap, out.data_ptr(), ws.data_ptr(),
                                                  ws_bytes, L.stream_ptr()), "hmm_json_find_matrices_device")
        nbytes = 8 * (4 + 4 * FIND_FIRST)
        down = stage(_device_stages, ("find", dev.index), (nbytes,))
        down.pinned[:nbytes].view(torch.int64).copy_(out[:4 + 4 * FIND_FIRST], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        words = down.host[:nbytes].view(np.uint64).copy()
        n_found, status = int(words[0]), int(words[2])
        if status != _FIND_OK:
            return None, words
        if n_found <= cap:
            break
        cap = n_found
    entries = words[4:4 + 4 * min(n_found, FIND_FIRST)]
    if n_found > FIND_FIRST:
        entries = np.concatenate([entries, out[4 + 4 * FIND_FIRST:4 + 4 * n_found].cpu().numpy().view(np.uint64)])
    return [tuple(int(v) for v in e) for e in entries.reshape(-1, 4)], words


def _find_routes(text: _EventText, min_values: int, report: dict = None):
    """Where the matrices of `text` lie -> (list, "device" | "host").  `report`, when given, receives the device's report."""
    import torch
    if len(text) == 0:
        return [], "host"
    if _find_route["on"] and _find_check["ok"] is not False:
        with torch.cuda.device(text.dev), _device_lock:
            found, words = _find_on_device(text, min_values)
            if report is not None:
                report.update(n_found=int(words[0]), n_candidates=int(words[1]), status=int(words[2]), first_declined=int(words[3]))
            if found is not None and _find_check["ok"] is None:
                ok = found == _find_by_host(text.all_bytes(), min_values)
                if not ok:
                    _log.warning("hippomm_amd.event_store: the device span finder disagrees with the host finder; "
                                 "every text is searched by the host finder in this process")
                _find_check["ok"] = ok
        if found is not None and _find_check["ok"]:
            _find_counts["device"] += 1
            return found, "device"
        _find_counts["declined" if found is None else "host"] += 1
    else:
        _find_counts["host"] += 1
    return _find_by_host(text.all_bytes(), min_values), "host"


def find_matrices_device(raw, min_values: int = NATIVE_MIN_VALUES, device=None, stats: dict = None):
    """Where the feature matrices of an event file lie, found ON THE GPU (``hmm_json_find_matrices_device``): every
    ``[[numbers], ...]`` with equally long rows and at least `min_values` numbers outside string literals, as
    [(begin, end, rows, cols)] in document order -- the list ``hmm_json_find_matrices`` gives for the same bytes, whatever they are.

    raw: the file as ``bytes`` (uploaded once, through pinned staging) or as a 1-D uint8 CUDA tensor that already holds it.  One
    launch sequence and one read-back: the report with the first 16 entries behind it; a second copy only for a text with more
    matrices.  The string state, the class of the last non-whitespace byte and the counts of tokens, rows and illegal bytes are
    prefix scans over groups of 4 KiB; a candidate ``[[`` is a matrix when the next ``]]``-or-``[[`` behind it is a ``]]`` with no
    illegal byte between and every row starts where equal rows put it.  The device declines -- and the host finder answers, on the
    bytes or on the tensor brought down -- for two reasons only: a candidate holds a number token above 64 bytes, or the text has
    more than 16384 candidates.  `stats`, when given, receives "route" ("device" or "host") and the device's report ("n_found",
    "n_candidates", "status", "first_declined") when the device ran.

    The first text a process searches this way has its list compared with the host finder's; on a mismatch a warning is logged
    and the host finder answers, as it does from then on.  Timings: profiles/event_json_find.json, DESIGN.md section 8.  Opt-in."""
    if not (_cuda_tensor(raw) or isinstance(raw, (bytes, bytearray, memoryview))):
        raise TypeError(f"find_matrices_device takes bytes or a uint8 CUDA tensor, got {type(raw).__name__}")
    if _cuda_tensor(raw):
        import torch
        if raw.dtype != torch.uint8 or raw.dim() != 1 or not raw.is_contiguous():
            raise TypeError("find_matrices_device takes a contiguous 1-D uint8 tensor")
    if int(min_values) < 0:
        raise ValueError(f"find_matrices_device: min_values {min_values!r} is negative")
    text = _EventText(raw, _parse_device_of(raw, device))
    report = {}
    found, route = _find_routes(text, int(min_values), report)
    if stats is not None:
        stats.update(report)
        stats["route"] = route
    return found


class _NativeMatrix:
    """Placeholder json.loads leaves where the library parsed a matrix."""
    __slots__ = ("array",)

    def __init__(self, array):
        self.array = array


def _load_json_native(raw: bytes, matrices: str = "host", device=None, counts: dict = None, find: str = "host"):
    """``json.loads(raw)`` with every large 2-D array of numbers parsed by the library (``hmm_json_find_matrices`` /
    ``hmm_json_parse_matrix_f32``: fp32, the value ``np.array(list).astype(float32)`` has) and left in the result as a
    ``_NativeMatrix``.  None when the library declines (a literal outside the double range) or a matrix sits where this module
    does not expect one -- the caller then uses plain ``json.loads``.  matrices="device": the text goes to `device` once and the
    spans are converted there (``_parse_matrix_routes``), each ``_NativeMatrix`` then holds a CUDA fp32 tensor.  `counts`, when
    given, counts the matrices per route.  find="device" (with matrices="device"): the spans are found in that same uploaded text
    on the device (``_find_routes``) instead of by ``hmm_json_find_matrices`` on the host."""
    import ctypes as C
    from . import _lib as L
    lib = _host_library() if matrices == "host" else L.load()       # the device route has no fallback: a missing library raises
    if lib is None:
        return None

    class Span(C.Structure):
        _fields_ = [("begin", C.c_size_t), ("end", C.c_size_t), ("rows", C.c_size_t), ("cols", C.c_size_t)]

    text = _EventText(raw, _parse_device_of(raw, device)) if matrices == "device" else None
    if find == "device":
        spans = [Span(*sp) for sp in _find_routes(text, NATIVE_MIN_VALUES)[0]]
        n = C.c_int(len(spans))
    else:
        n = C.c_int(0)
        cap = 16
        while True:
            spans = (Span * cap)()
            L.check(lib.hmm_json_find_matrices(raw, len(raw), NATIVE_MIN_VALUES, C.cast(spans, C.c_void_p), cap, C.byref(n)), "hmm_json_find_matrices")
            if n.value <= cap:
                break
            cap = n.value
    if n.value == 0:
        return json.loads(raw)
    salt = uuid.uuid4().hex
    pieces, mats, pos = [], {}, 0
    for i in range(n.value):
        sp = spans[i]
        if text is not None:
            a, route = _parse_matrix_routes(text, _span4(sp), np.float32)
            if a is None:
                return None
        else:
            a, route = np.empty((sp.rows, sp.cols), np.float32), "host"
            if lib.hmm_json_parse_matrix_f32(raw, sp.begin, sp.end, sp.rows, sp.cols, a.ctypes.data_as(C.c_void_p)) != 0:
                return None
        if counts is not None:
            counts[route] += 1
        token = f"@@hmm_matrix_{i}_{salt}@@"
        mats[token] = a
        pieces += [raw[pos:sp.begin], b'"' + token.encode() + b'"']
        pos = sp.end
    pieces.append(raw[pos:])
    reduced = b"".join(pieces)
    if any(reduced.count(t.encode()) != 1 for t in mats):          # the token also occurs in the event's own strings
        return None

    def put_back(v):
        if isinstance(v, str) and v in mats:
            return _NativeMatrix(mats[v])
        if isinstance(v, dict):
            return {k: put_back(x) for k, x in v.items()}
        if isinstance(v, list):
            return [put_back(x) for x in v]
        return v
    return put_back(json.loads(reduced))


def _check_find(find: str, device_route: bool, needs: str) -> None:
    if find not in ("host", "device"):
        raise ValueError(f"find must be 'host' or 'device', not {find!r}")
    if find == "device" and not device_route:
        raise ValueError(f"find='device' searches the text the device parses: it needs {needs}")


def parse_event_features(json_path, native: bool = True, matrices: str = "host", device=None,
                         stats: dict = None, find: str = "host") -> Tuple[Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """An event file without sidecars, by the reference's own reading rules (:369-408): new format with ``feature_times``, and
    the old format where a modality maps to ``{'features': ..., 'times': ...}``.  Features come back as fp32.  With ``native`` the
    feature matrices -- 99.9 % of the text -- are converted by the library instead of ``json.load`` + ``np.array(list)`` (~10x
    faster, same values: tests/test_cpu_event_store.py); ``native=False`` is the reference's path as it stands.

    matrices="device" (opt-in, with ``native``): the file is uploaded once and every matrix the library finds among the feature
    values is converted ON THE GPU (``parse_matrix_device``) and comes back as a CUDA fp32 tensor on `device` -- the same bits;
    where the device declines a matrix the host parser converts it and it is uploaded.  The same rule says which matrices are
    taken (feature values only); times and metadata keep ``json``'s float64 lists, and features the library does not report
    (fewer than 1024 values, 1-D) stay numpy arrays.  Where the host parser declines as well, or a matrix is a stray, the whole
    file goes through ``json.loads`` exactly as on the host route, and every feature is a numpy array.
    `stats`, when given, receives "device", "host" and "json": the feature matrices each route read.

    find="device" (opt-in, with matrices="device" only): where the matrices lie is decided on the GPU as well
    (``find_matrices_device``), on the text that was uploaded for the parser -- the host no longer walks the file; it keeps the
    file read, one read-back of the span list and ``json.loads`` of the few KB around the matrices.  The same spans, so the same
    result; where the device declines a text the host finder answers."""
    if matrices not in ("host", "device"):
        raise ValueError(f"matrices must be 'host' or 'device', not {matrices!r}")
    _check_find(find, matrices == "device", "matrices='device'")
    raw = Path(json_path).read_bytes()
    counts = {"device": 0, "host": 0, "json": 0}
    data = _load_json_native(raw, matrices, device, counts, find) if native else None
    if data is not None:
        # matrices are expected as feature values only; anywhere else (times, metadata) keeps the reference's float64 lists
        feats_in = data.get("features") if isinstance(data, dict) else None
        allowed = set()
        if isinstance(feats_in, dict):
            for d in feats_in.values():
                if isinstance(d, _NativeMatrix):
                    allowed.add(id(d))
                elif isinstance(d, dict) and isinstance(d.get("features"), _NativeMatrix):
                    allowed.add(id(d["features"]))

        def stray(v):
            if isinstance(v, _NativeMatrix):
                return id(v) not in allowed
            if isinstance(v, dict):
                return any(stray(x) for x in v.values())
            if isinstance(v, list):
                return any(stray(x) for x in v)
            return False
        if stray(data):
            data = None
    by_json = data is None
    if by_json:
        data = json.loads(raw)
    unwrap = lambda v: v.array if isinstance(v, _NativeMatrix) else np.array(v)     # noqa: E731
    feats, times = {}, {}
    if "feature_times" in data:
        for modality, t in data["feature_times"].items():
            times[modality] = np.array(t)
        for modality, f in data["features"].items():
            feats[modality] = unwrap(f)
    else:
        for modality, d in data["features"].items():
            if isinstance(d, dict):
                if "features" in d:
                    feats[modality] = unwrap(d["features"])
                if "times" in d:
                    times[modality] = np.array(d["times"])
            else:
                feats[modality] = unwrap(d)
    if by_json:                                                  # whatever the routes had read before one of them declined is dropped
        counts = {"device": 0, "host": 0, "json": sum(1 for a in feats.values() if a.ndim == 2)}
    if matrices == "device":
        for route, n in counts.items():
            _parse_counts[route] += n
    if stats is not None:
        stats.update(counts)
    return {modality: _as_feature_matrix(a) for modality, a in feats.items()}, times


def load_event_features(json_path, use_sidecar: bool = True, write_sidecar: bool = True,
                        mmap: bool = False) -> Dict[str, np.ndarray]:
    """fp32 feature matrices of one event; sidecar when fresh, JSON otherwise."""
    json_path = Path(json_path)
    if use_sidecar:
        m = _fresh_manifest(json_path)
        if m is not None:
            try:
                out = {}
                for mod, shape in m["modalities"].items():
                    a = np.load(_sidecar_paths(json_path, mod)[0], mmap_mode="r" if mmap else None)
                    if a.dtype != np.float32 or list(a.shape) != list(shape):
                        raise ValueError(f"sidecar of {mod!r} is {a.dtype}{a.shape}, manifest says float32{tuple(shape)}")
                    out[mod] = a
                return out
            except (OSError, ValueError):            # missing, truncated or foreign .npy: fall back to the JSON
                pass
    feats, _ = parse_event_features(json_path)
    if write_sidecar:
        try:
            _write_sidecars(json_path, feats)
        except OSError:
            pass                                    # read-only store: keep working from the JSON
    return feats


def iter_event_files(memory_store_dir) -> Iterable[Tuple[str, Path]]:
    """(event_id, json path) in index order, from ``<base>/event_index.json`` (:338-346)."""
    base = Path(memory_store_dir)
    index = json.loads((base / "event_index.json").read_text())
    for event_id, info in index.items():
        p = Path(info["file_path"])
        if not p.is_absolute() and not p.exists():
            p = base / "events" / info["video_id"] / f"{event_id}.json"
        yield event_id, p


def _check_parse(parse: str) -> None:
    if parse not in ("host", "device"):
        raise ValueError(f"parse must be 'host' or 'device', not {parse!r}")


def _event_segment_device(json_path: Path, modality: str, device, write_sidecar: bool, find: str = "host"):
    """One event without fresh sidecars on the parse="device" route: its matrices are converted on the GPU and the ``modality``
    one stays there; the sidecars come from one read-back of each fp32 matrix."""
    feats, _ = parse_event_features(json_path, matrices="device", device=device, find=find)
    if write_sidecar:
        try:
            _write_sidecars(json_path, {m: _on_host(f, fp32=True) for m, f in feats.items()})
        except OSError:
            pass                                    # read-only store: keep working from the JSON
    return _modality_matrix(feats, modality)


def build_event_store(memory_store_dir, modality: str = "vision", device=None, workers: Optional[int] = None, parse: str = "host",
                      write_sidecar: bool = True, find: str = "host"):
    """All events' ``modality`` matrices of a memory_store, resident in HBM.  Returns (EventStore, event_ids);
    events that lack the modality or whose width is not 1024 get an empty segment (the reference skips them
    with a warning, :3135-3137).  Event files are read by ``workers`` threads (default: min(16, cores)): the sidecar reads and
    the library's matrix parser run outside the GIL, so a cold store loads in parallel; the order of the events is the index's.

    parse="device" (opt-in): events with fresh sidecars load as above; the others are read one after the other, their text
    converted on the GPU (``parse_event_features(matrices="device")``), and enter the store through ``EventStore.extend`` from
    the device tensors -- no host fp32 matrix, no second upload; the same rows, offsets and search results.  Their sidecars are
    still written, from one read-back of each fp32 matrix, unless ``write_sidecar=False``.  find="device" (opt-in, with
    parse="device" only): those texts are searched for their matrices on the GPU too (``parse_event_features(find="device")``)."""
    from concurrent.futures import ThreadPoolExecutor
    from .vector_ops import EventStore
    _check_parse(parse)
    _check_find(find, parse == "device", "parse='device'")
    files = list(iter_event_files(memory_store_dir))
    if workers is None:
        workers = min(16, os.cpu_count() or 1)
    cold = {i for i, (_, path) in enumerate(files) if _fresh_manifest(path) is None} if parse == "device" else set()
    warm = [f for i, f in enumerate(files) if i not in cold]
    if workers > 1 and len(warm) > 1:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            loaded = list(pool.map(lambda f: load_event_features(f[1]), warm))
    else:
        loaded = [load_event_features(path) for _, path in warm]
    loaded = iter(loaded)
    ids, mats = [], []
    for i, (event_id, path) in enumerate(files):
        ids.append(event_id)
        mats.append(_event_segment_device(path, modality, device, write_sidecar, find) if i in cold else _modality_matrix(next(loaded), modality))
    if parse == "host":
        return EventStore(mats, device), ids
    store = EventStore([], device)
    store.extend(mats)
    return store, ids


def _modality_matrix(feats: Mapping[str, np.ndarray], modality: str) -> np.ndarray:
    """One event's segment of an EventStore: its ``modality`` matrix (a numpy array, or a CUDA tensor from the device parser), a
    1-D feature as one row, and an empty segment when the modality is missing or its width is not 1024."""
    a = feats.get(modality)
    if a is not None and a.ndim == 1 and a.shape[0] == 1024:
        a = a.reshape(1, 1024)                       # top_k_cosine_similarity treats a 1-D feature as one row (vector_ops.py:173-174)
    if a is None or a.ndim != 2 or a.shape[1] != 1024:
        a = np.zeros((0, 1024), np.float32)
    return a


def refresh_event_store(store, ids, memory_store_dir, modality: str = "vision", parse: str = "host", write_sidecar: bool = True,
                        find: str = "host"):
    """Bring a resident EventStore up to date with ``event_index.json`` after ``save_theta_event`` wrote new events: the events
    of the index that are not in ``ids`` yet are appended on the device (``EventStore.extend``: the rows already resident are
    neither re-read nor re-uploaded, a shadow is kept current), events that vanished from the index are removed
    (``EventStore.remove_events``).  Returns the new id list; ``store`` and the list equal what ``build_event_store`` returns
    for the same index as long as the index only grew at its end or lost entries, which is how the reference writes it
    (hippocampal_memory.py:338-346).  A missing modality, a 1-D feature and a wrong width are handled as there.  An event whose
    file changed under an id that stays is not noticed: use ``EventStore.replace_event``.  parse="device" and ``write_sidecar``:
    and ``find``: as in ``build_event_store``, on the store's own device."""
    _check_parse(parse)
    _check_find(find, parse == "device", "parse='device'")
    files = list(iter_event_files(memory_store_dir))
    in_index = {event_id for event_id, _ in files}
    gone = [pos for pos, event_id in enumerate(ids) if event_id not in in_index]
    if gone:
        store.remove_events(gone)
    new_ids = [event_id for event_id in ids if event_id in in_index]
    have = set(new_ids)
    fresh = [(event_id, path) for event_id, path in files if event_id not in have]
    if fresh:
        store.extend([_event_segment_device(path, modality, store.rows.device, write_sidecar, find)
                      if parse == "device" and _fresh_manifest(path) is None else _modality_matrix(load_event_features(path), modality)
                      for _, path in fresh])
        new_ids += [event_id for event_id, _ in fresh]
    return new_ids
