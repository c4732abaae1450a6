"""Consolidation similarity on MI355X -- host-side mirror of
``HippocampalMemory._select_key_frames`` (hippomm/core/hippocampal_memory.py:944-967),
bound to ``hmm_gram_select`` (fp32 normalise, fp64-accumulated gram via f64 MFMA, greedy scan).  ``KeyFrameSelector`` is the
same selection grown batch by batch (``hmm_keyframe_extend``): each frame is decided when its embedding arrives.
``consolidate_short_term_memory`` is the caller around the selection (:754-927): the rows of every segment's block stacked in time
order by one gather launch on the device (``hmm_rows_gather``), selected there, and returned as numpy or as device tensors.
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


# ---- the caller around the selection: consolidate_short_term_memory and its two helpers (hippocampal_memory.py:754-927) ----
#
# The reference walks every segment's memory, picks one row per frame out of the segment's own feature block
# (_extract_frame_feature, :929-942 -- with tensor features a .cpu() of the whole block per frame), sorts the rows by time, stacks
# them on the host (:842) and selects.  Here the walk is a PLAN on the host (which row of which block goes where: shapes and times
# only, no feature value is touched) and the stack is one launch of hmm_rows_gather over the blocks where they lie on the device.

def _is_block(a) -> bool:
    return isinstance(a, (np.ndarray, torch.Tensor))


def _flat_width(shape) -> int:
    """``feature.flatten().shape[0]`` for more than one dimension, ``feature.shape[0]`` otherwise (:827-829, :885-887)."""
    return int(np.prod(shape)) if len(shape) > 1 else shape[0]


def plan_vision_rows(memories):
    """The loop of ``_process_vision_features`` (:818-838) without the features: -> (entries, skipped).  ``entries`` has one
    ``(memory index, row index or None, frame, frame_time)`` per row the reference stacks, in the order it stacks them; a row index
    of None means "the whole block, flattened".  ``skipped`` counts the rows the reference drops with its warning.  Pure host.

    ``_extract_frame_feature``'s rules (:929-942): a block with more than one row and ``idx < rows`` gives row ``idx``; a block of
    one row, or a 1-D block, gives itself to every frame of its memory; ``idx >= rows`` on a block of several rows gives the whole
    matrix, whose flattened width is wrong, so it is skipped; frames beyond ``len(frame_times)`` are ignored; a block that is
    neither an array nor a tensor gives nothing.  The order is Python's own stable ``sort(key=time)`` on the collected list, as
    :838 -- ties stay in collection order, and a ``None`` time raises the ``TypeError`` it raises there."""
    entries, skipped = [], 0
    for mi, memory in enumerate(memories):
        if 'vision' in memory.modalities and 'frames' in memory.content:
            for idx, frame in enumerate(memory.content['frames']):
                if idx < len(memory.content.get('frame_times', [])):
                    frame_time = memory.content['frame_times'][idx]
                    block = memory.features.get('vision')
                    if not _is_block(block):                                  # None, or a type :937 does not know
                        continue
                    shape, row = tuple(block.shape), None
                    if len(shape) > 1 and shape[0] > 1 and idx < shape[0]:    # :938
                        shape, row = shape[1:], idx
                    if _flat_width(shape) != FEATURE_DIM:                     # :829
                        skipped += 1
                        continue
                    entries.append((mi, row, frame, frame_time))
    entries.sort(key=lambda e: e[3])                                          # :838
    return entries, skipped


def _walk_audio(memories):
    entries, skipped, transcriptions = [], 0, []
    for mi, memory in enumerate(memories):
        if 'audio' in memory.modalities and 'audio' in memory.content:
            if 'audio' in memory.features:
                start = memory.content['audio'].get('start_time')
                block = memory.features['audio']
                if _flat_width(tuple(block.shape)) != FEATURE_DIM:            # :887: the memory's transcription is dropped with it
                    skipped += 1
                    continue
                if _is_block(block):                                          # :903
                    entries.append((mi, None, None, start))
            if memory.transcription:
                transcriptions.extend(memory.transcription)
    return entries, skipped, transcriptions


def plan_audio_rows(memories):
    """The loop of ``_process_audio_features`` (:875-905) without the features: -> (entries, skipped), entries as
    ``plan_vision_rows`` gives them with ``(memory index, None, None, start_time)``.  Memory order is kept (the reference does not
    sort here), a tensor or a 2-D (1,1024) block counts flattened, a block of another width is skipped with the reference's
    warning, and the times are the ``start_time`` values of ``content['audio']`` as they are (None when absent).  Pure host."""
    entries, skipped, _ = _walk_audio(memories)
    return entries, skipped


def _f32(block) -> bool:
    return block.dtype == (torch.float32 if isinstance(block, torch.Tensor) else np.float32)


def _stack_host(blocks, entries) -> np.ndarray:
    """The reference's own expression (:824-842): every block on the host (one read-back per block, where the reference makes one
    per frame), the row or the flattened block per entry, ``np.stack``."""
    host = {mi: b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b for mi, b in blocks.items()}
    return np.stack([(host[mi] if row is None else host[mi][row]).reshape(-1) for mi, row, _, _ in entries])


def _gather_device(blocks, entries, dev, stat) -> torch.Tensor:
    """(n,1024) fp32 on `dev`: row i is what entry i names.  Resident blocks are read where they lie (a row of a 2-D view with
    unit column stride at its own address, whatever the row stride; anything else through a contiguous copy on the device); host
    blocks travel once each, together with the address table, in ONE pinned buffer and one copy; one ``hmm_rows_gather`` launch."""
    from ._pinned import stage
    from .event_store import _device_lock, _device_stages
    lib, n = _lib.load(), len(entries)
    table_bytes = (8 * n + 255) // 256 * 256
    resident, host, at, total = {}, {}, {}, table_bytes
    for mi, b in blocks.items():
        if isinstance(b, torch.Tensor) and b.is_cuda:
            resident[mi] = b.detach() if b.device == dev else b.detach().to(dev)
        else:
            host[mi] = np.ascontiguousarray(b.detach().numpy() if isinstance(b, torch.Tensor) else b)
            at[mi], total = total, total + (host[mi].nbytes + 255) // 256 * 256
    stat["resident"], stat["uploaded"] = len(resident), len(host)

    def address(mi, row) -> int:
        if mi in host:
            return raw.data_ptr() + at[mi] + (0 if row is None else row * 4 * FEATURE_DIM)
        t = resident[mi]
        if row is not None and t.dim() == 2 and t.stride(1) == 1:
            return t.data_ptr() + row * t.stride(0) * 4
        if not t.is_contiguous():
            t = resident[mi] = t.contiguous()
        return t.data_ptr() + (0 if row is None else row * 4 * FEATURE_DIM)

    with torch.cuda.device(dev), _device_lock:
        raw = torch.empty(total, dtype=torch.uint8, device=dev)
        up = stage(_device_stages, ("up", dev.index), (total,))
        up.wait()
        up.host[: 8 * n].view(np.int64)[:] = [address(mi, row) for mi, row, _, _ in entries]
        for mi, a in host.items():
            up.host[at[mi]: at[mi] + a.nbytes] = a.reshape(-1).view(np.uint8)
        raw.copy_(up.pinned[:total], non_blocking=True)
        up.mark()
        out = torch.empty(n, FEATURE_DIM, dtype=torch.float32, device=dev)
        _lib.check(lib.hmm_rows_gather(raw.data_ptr(), n, FEATURE_DIM, out.data_ptr(), _lib.stream_ptr()), "hmm_rows_gather")
    # `raw` and `resident` (the contiguous copies among them) have lived until here: the gather is on the stream, and what the
    # allocator hands out again from now on is ordered behind it on that stream
    return out


def _kept_device(matrix: torch.Tensor, similarity_threshold: float) -> np.ndarray:
    """``hmm_gram_select`` on the gathered matrix; the count and the indices come back in one copy: the call's only read-back."""
    n = matrix.shape[0]
    if n <= 2:                                                                # :947-948
        return np.arange(n)
    lib = _lib.load()
    with torch.cuda.device(matrix.device):
        meta = torch.zeros(1 + n, dtype=torch.int64, device=matrix.device)    # the count (an int32 in the low half), then the indices
        ws = torch.empty(max(lib.hmm_gram_select_workspace_bytes(n), 256), dtype=torch.uint8, device=matrix.device)
        thr = float(np.float32(similarity_threshold))                         # the reference compares in float32 (:960)
        _lib.check(lib.hmm_gram_select(matrix.data_ptr(), n, FEATURE_DIM, thr, meta.data_ptr() + 8, meta.data_ptr(), ws.data_ptr(),
                                       ws.numel(), _lib.stream_ptr()), "hmm_gram_select")
        host = meta.cpu().numpy()
    return host[1: 1 + min(max(int(host[0]), 0), n)].copy()


def _stacked(memories, key, entries, features, device, stat, select, similarity_threshold):
    """-> (the stacked matrix as `features` asks for it, the kept indices or None when `select` is off)."""
    blocks = {mi: memories[mi].features[key] for mi, _, _, _ in entries}
    if all(_f32(b) for b in blocks.values()):
        stat["route"] = "device"
        matrix = _gather_device(blocks, entries, _target_device(device), stat)
        kept = _kept_device(matrix, similarity_threshold) if select else None
        return (matrix if features == "device" else matrix.cpu().numpy()), kept
    stat["route"] = "host"
    matrix = _stack_host(blocks, entries)
    kept = select_key_frames(matrix, None, similarity_threshold) if select else None
    if features == "device":
        matrix = torch.from_numpy(matrix).to(_target_device(device))
    return matrix, kept


def _target_device(device) -> torch.device:
    """`device` with an index (None, or "cuda" without one: the current device), once the GPU has been checked."""
    current = _lib.require_gpu()
    dev = current if device is None else torch.device(device)
    return dev if dev.index is not None else current


_EMPTY = {"route": None, "rows": 0, "skipped": 0, "resident": 0, "uploaded": 0}


def _vision_part(memories, similarity_threshold=0.9, features="host", device=None, stat=None):
    stat = {} if stat is None else stat
    entries, skipped = plan_vision_rows(memories)
    stat.update(_EMPTY, rows=len(entries), skipped=skipped)
    if not entries:
        return {'features': {}, 'content': {}}
    times = np.array([e[3] for e in entries])                                 # :843
    matrix, kept = _stacked(memories, 'vision', entries, features, device, stat, True, similarity_threshold)
    return {'features': {'vision': matrix, 'vision_times': times},
            'content': {'frames': [entries[i][2] for i in kept], 'frame_times': times[kept].tolist()}}


def _audio_part(memories, features="host", device=None, stat=None):
    stat = {} if stat is None else stat
    entries, skipped, transcriptions = _walk_audio(memories)
    stat.update(_EMPTY, rows=len(entries), skipped=skipped)
    if not entries:
        return {'features': {}, 'content': {}}
    times = np.array([e[3] for e in entries])                                 # :909
    matrix, _ = _stacked(memories, 'audio', entries, features, device, stat, False, None)
    return {'features': {'audio': matrix, 'audio_times': times},
            'content': {'audio_times': times.tolist(), 'transcription': transcriptions if transcriptions else None}}


def consolidate_short_term_memory(memories, similarity_threshold: float = 0.9, *, features: str = "host", device=None,
                                  stats: Optional[dict] = None):
    """``HippocampalMemory.consolidate_short_term_memory`` (:754-813) with its two helpers (:815-927): all short-term memories of a
    video combined into one ``checkpoint.ShortTermMemory``, filled as :773-802 fills it.  ``memories`` is sorted in place by
    ``segment_info.start_time`` (the reference sorts the caller's list); ``timestamp`` and ``source_time`` come from the first
    memory, ``segment_info`` is ``SequenceSegment(first.timestamp, last.timestamp)``, ``transcription`` is ``[]``; ``features`` holds
    'vision', 'vision_times', 'audio', 'audio_times' and ``content`` 'frames', 'frame_times', 'audio_times', 'transcription', in
    that order, each pair only when its modality has rows to stack.  An empty list returns None.  The times arrays are
    ``np.array(list)`` on the host, as in the reference.

    Device route, per modality, when every block the plan names (``plan_vision_rows`` / ``plan_audio_rows``) is float32, a numpy
    array or a tensor alike: blocks on the device are read where they lie, host blocks are uploaded once each -- all of them and
    the table of row addresses in one pinned buffer and one copy --, ``hmm_rows_gather`` builds the stacked, time-ordered matrix
    in one launch, ``hmm_gram_select`` runs on it, and the kept indices are the only read-back (one synchronisation; ``n <= 2``
    keeps all rows without any, :947-948).  ``features="device"`` returns the gathered CUDA tensors themselves, which
    ``event_store.event_json_bytes(..., matrices="device")``, ``EventStore.append_event`` and ``top_k_cosine_similarity`` take as
    they are; ``features="host"`` (the default, and what the drop-ins use) reads them back into numpy matrices, as the reference
    returns.  The stacked bytes are the blocks' bytes either way.

    Host route, per modality, when any named block has another dtype: the reference's numpy expression (``np.stack`` of the rows,
    numpy's own dtype promotion) followed by ``select_key_frames``; ``features="device"`` then uploads that matrix as it is.

    ``stats``, when given, receives per modality ('vision', 'audio') a dict: "route" ("device", "host", or None when nothing was
    stacked), "rows", "skipped" (rows dropped with the reference's wrong-width rule), "resident" and "uploaded" (blocks read where
    they lay / uploaded on the device route).

    One deviation: ``modalities`` is 'vision', then 'audio', then any other name in sorted order, each when some memory has it.
    The reference's ``list(set().union(...))`` has the iteration order of a set of strings, which varies between processes."""
    if features not in ("host", "device"):
        raise ValueError(f"features must be 'host' or 'device', not {features!r}")
    if not memories:
        return None
    from .checkpoint import SequenceSegment, ShortTermMemory
    memories.sort(key=lambda x: x.segment_info.start_time)                    # :769
    present = set().union(*(memory.modalities for memory in memories))        # :787
    out = ShortTermMemory(features={}, content={}, timestamp=memories[0].timestamp, source_time=memories[0].source_time,
                          modalities=[m for m in ('vision', 'audio') if m in present] + sorted(present - {'vision', 'audio'}),
                          segment_info=SequenceSegment(start_time=memories[0].timestamp, end_time=memories[-1].timestamp),
                          transcription=[])
    stats = {} if stats is None else stats
    if 'vision' in present:
        part = _vision_part(memories, similarity_threshold, features, device, stats.setdefault('vision', {}))
        out.features.update(part['features'])
        out.content.update(part['content'])
    if 'audio' in present:
        part = _audio_part(memories, features, device, stats.setdefault('audio', {}))
        out.features.update(part['features'])
        out.content.update(part['content'])
    return out


def _process_vision_features(self, memories, pool=None):
    """Drop-in for ``HippocampalMemory._process_vision_features`` (assign it on the class; ``self`` and ``pool`` are unused, the
    pool there as well): the reference's dict, ``{'features': {}, 'content': {}}`` when nothing can be stacked."""
    return _vision_part(memories)


def _process_audio_features(self, memories, pool=None):
    """Drop-in for ``HippocampalMemory._process_audio_features`` (assign it on the class)."""
    return _audio_part(memories)


def _consolidate_short_term_memory(self, memories):
    """Drop-in for ``HippocampalMemory.consolidate_short_term_memory`` (assign it on the class under that name; it starts no
    process pool -- the reference's two helpers never use theirs)."""
    return consolidate_short_term_memory(memories)
