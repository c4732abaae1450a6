"""The write side of the reference's ``batch_process.py`` on MI355X: the write of every frame the formation path keeps (the JPEG
is encoded on the GPU, byte for byte Pillow's file):

    save_frame, save_frames       <- hippomm/core/batch_process.py:73-114 (cv2.imwrite)

and the loop those two sit in, with the last saved frame, the cumulative difference and the time of the last save on the device
(``hmm_extract_walk``, hippomm_amd/csrc/extract_walk.hip: every candidate uploaded once, one read-back per batch):

    extract_frames, FrameExtractor, extraction_records   <- hippomm/core/batch_process.py:179-228
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib, jpeg, ssim
from ._pinned import PinnedStage
from .frame_cache import FrameCache
from .ssim import WIN, check_frame, compute_frame_difference, host_gray

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
    claimed to equal OpenCV's file.  It is ``save_frames`` for one frame: ``cache`` / ``tower_inputs`` as there, the same rules.

    Measured on one MI355X (profiles/jpeg_encode.json; the encode alone, without the file write): one
    1280 x 720 host frame 0.41 ms against 2.14 ms for Pillow on one thread, one 1920 x 1080 host frame 0.68 against 4.69 ms,
    upload and read-back included; a resident frame 0.29 and 0.44 ms.  ``save_frames`` on 32 host frames: 5.9 ms (720p) and
    12.6 ms (1080p) against 68 and 152 ms, bound by the upload.  No point measured was slower than Pillow on one thread; several
    Pillow threads, and a GPU busy with the tower at the same time, were not measured."""
    try:
        return save_frames([frame], [frame_path], cache=cache, tower_inputs=tower_inputs)[0]
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
            from . import preprocess as pp
            window = pp.needed_window(*next(iter(sizes))) if cache is None and len(sizes) == 1 else None
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
            if not results[i]:
                _save_log.error(f"Frame file not found after save: {paths[i]}")
                continue
            _save_log.debug("Successfully saved frame to %s", paths[i])
            if resident:
                written.append((paths[i], decoded[k], tuple(int(v) for v in frames[i].shape[:2])))
        except Exception as e:                       # noqa: BLE001
            _save_log.error(f"Error saving frame to {paths[i]}: {e}")
    if written:
        try:
            _fill_caches(written, cache, tower_inputs)
        except Exception as e:                       # noqa: BLE001
            _save_log.error(f"Error keeping {len(written)} decoded frames on the device: {e}")
    return results


CHECK_INTERVAL, MAX_DIFF_THRESHOLD = 30, 0.3   # extract_frames_from_video's defaults (batch_process.py:121-123)
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
    return _state_record(*(record[f] for f in ("has_anchor_after", "anchor_slot_after", "cumulative_after", "last_save_time_after")))


class _Walker:
    """The device buffers of the walk for one frame size: gray slots (slot 0: the anchor), records and state in one buffer (one
    read-back), workspace."""

    def __init__(self, h: int, w: int, capacity: int, dev):
        lib = _lib.load()
        self.h, self.w, self.capacity, self.dev = h, w, capacity, dev
        self._state_at = capacity * EXTRACT_RECORD.itemsize            # the state follows the records in `out`
        self.slots = torch.empty((capacity + 1, h, w), dtype=torch.uint8, device=dev)
        self.minmax = torch.empty((capacity + 1, 2), dtype=torch.int32, device=dev)
        self.out = torch.zeros(capacity * EXTRACT_RECORD.itemsize + EXTRACT_STATE.itemsize, dtype=torch.uint8, device=dev)
        self.ws = torch.empty(max(lib.hmm_extract_walk_workspace_bytes(h, w), 256), dtype=torch.uint8, device=dev)

    def set_state(self, record: np.ndarray) -> None:
        self.out[self._state_at:].copy_(torch.from_numpy(record.view(np.uint8).copy()))

    def fill(self, frames: torch.Tensor) -> None:
        """(n, H, W, 3) BGR or (n, H, W) gray on the device -> slots 1 .. n."""
        n = frames.shape[0]
        if frames.dim() == 4:
            ssim.gray_into(frames, ssim.ORDER["BGR"], self.slots[1:n + 1], self.minmax[1:n + 1])
        else:
            self.slots[1:n + 1].copy_(frames)

    def walk(self, first: int, counts, video_fps, check_interval, deny, threshold: float, min_gap: float) -> None:
        """Candidates first .. of the batch whose positions in the video are ``counts`` (0-based in the batch; slot = index + 1);
        record i lands at index i.  The loop's own ``current_time = frame_count / video_fps`` in Python floats (:184) and check
        flags ``frame_count % check_interval == 0``; ``deny[i]``: the save of candidate i failed."""
        times = np.array([c / video_fps for c in counts[first:]], dtype=np.float64)
        check = np.array([c % check_interval == 0 for c in counts[first:]], dtype=np.int32)
        deny = np.ascontiguousarray(deny[first:], dtype=np.int32)
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
    denied = np.zeros(n, np.int32)
    denied[list(deny)] = 1
    walker.fill(f.to(dev).contiguous())
    walker.walk(0, counts, video_fps, check_interval, denied, max_diff_threshold, min_gap)
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
        frame = check_frame(frame, "frame")
        h, w = frame.shape[:2]
        if self._counts and self._stage.host.shape[1:] != frame.shape:
            self.flush()
            has_anchor = bool(self._state["has_anchor"][0])
        if h < WIN or w < WIN or (has_anchor and (self._walker.h, self._walker.w) != (h, w)):
            self.flush()
            self._decide_on_host(frame_count, frame)
            return
        if self._stage is None or self._stage.host.shape[1:] != frame.shape:
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
        deny = np.zeros(n, np.int32)
        snapshot, first = self._state.copy(), 0
        while True:
            wk.walk(first, counts, self.video_fps, self.check_interval, deny, self.max_diff_threshold, MIN_SAVE_GAP)
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
                wk.slots[0].copy_(torch.from_numpy(np.ascontiguousarray(host_gray(frame))))
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
