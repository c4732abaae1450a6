"""Frames by path on MI355X: decode, gray, a device cache, and the scorer of image-file pairs behind

    _compute_frame_similarity     <- hippomm/core/hippocampal_memory.py:980-991

The GPU scorer decodes a frame only when the walk of ``_segment_sequence`` first consults a pair that needs it, keeps decoded
gray frames in a byte-bounded device cache keyed by path (boundary frames are shared between windows), scores the last pair of a
window on its own and, when that one does not break, the rest of the window in one launch.  Errors -- an unreadable file (an
``OSError`` naming the path where the reference raises ``cv2.error``), frames of different shapes, a side under 7 pixels -- are
raised only when the walk consults the pair they belong to, which is where the reference raises them.
"""
from __future__ import annotations

import os
import threading
from collections import OrderedDict
from functools import partial
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, jpeg, ssim

CACHE_BYTES = 512 << 20                   # device cache of gray frames (1080p: 2 MiB per frame)
UPLOAD_FRAMES = 32                        # frames per pinned staging round
ADJACENT_CHUNK = 64                       # frames per load-and-score round of PathScorer.score_adjacent


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
        ssim.gray_into(up, 0, gray, minmax)
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

    def _read_one(self, path):
        """-> (key, the file's bytes), or (None, the OSError to raise when the walk consults this frame)."""
        try:
            k = self.key(path)
            with open(path, "rb") as fh:
                return k, fh.read()
        except Exception as exc:                       # noqa: BLE001 - raised later, when the walk consults this frame
            return None, OSError(f"cannot read image file {path!r}: {exc}")

    def _store_groups(self, decoded, size_of: Callable, to_device: Callable, dev, out: dict) -> None:
        """decoded [(path, key, frame or the exception its decode raised)] -> out[path]: the exception, or (slab, slot).  The frames
        of one size (``size_of(frame)`` -> (h, w)) become one (n, h, w, 3) RGB tensor on the device by ``to_device(h, w, frames,
        dev)`` and are stored together; the slots of that size already in `out` are protected from them."""
        groups = {}
        for p, k, frame in decoded:
            if isinstance(frame, Exception):
                out[p] = frame
            else:
                groups.setdefault(size_of(frame), []).append((p, k, frame))
        for (h, w), members in groups.items():
            up = to_device(h, w, [frame for _, _, frame in members], dev)
            protect = sum(1 for v in out.values() if isinstance(v, tuple) and v[0].h == h and v[0].w == w)
            slab, slots = self._store(h, w, [k for _, k, _ in members], up, dev, protect)
            out.update((p, (slab, slot)) for (p, _, _), slot in zip(members, slots))

    def _decode_on_device(self, files, dev, out: dict) -> set:
        """files [(path, key, bytes)] -> the paths the JPEG device route (hippomm_amd/jpeg.py) took: stored, or their error in `out`."""
        jpegs = [(p, k, data) for p, k, data in files if jpeg.takes(jpeg.parse(data))]
        if not (jpegs and jpeg.route_ok(jpegs[0][2], dev)):
            return set()
        frames, errors, n_dev = jpeg._decode_many([d for _, _, d in jpegs], dev)
        self.device_decodes += n_dev
        decoded = [(p, k, frame if exc is None else OSError(f"cannot read image file {p!r}: {exc}"))
                   for (p, k, _), frame, exc in zip(jpegs, frames, errors)]
        self._store_groups(decoded, lambda f: (f.shape[0], f.shape[1]), lambda h, w, frames, dev: torch.stack(frames), dev, out)
        return {p for p, _, _ in jpegs}

    @staticmethod
    def _open_one(item):
        """(path, key, bytes) -> (path, key, the loaded RGB Pillow image or the OSError for the walk to raise)."""
        from . import preprocess as pp
        try:
            return item[0], item[1], pp._open_rgb_bytes(item[2])
        except Exception as exc:                       # noqa: BLE001 - raised later, when the walk consults this frame
            return item[0], item[1], OSError(f"cannot read image file {item[0]!r}: {exc}")

    @staticmethod
    def _upload_images(pool, h: int, w: int, images, dev) -> torch.Tensor:
        """Pillow images of one size -> (n, h, w, 3) RGB on the device: packed into the staging buffer on the pool, one copy."""
        from . import preprocess as pp
        lib = _lib.load()
        return ssim.upload(dev, (len(images), h, w, 3),
                           lambda host: list(pool.map(lambda it: pp._pack_into(it[1], host[it[0]], lib), enumerate(images))))

    def _decode_with_pillow(self, files, pool, dev, out: dict) -> None:
        """files [(path, key, bytes)] -> opened by Pillow on the decode pool and stored, or their error in `out`."""
        opened = list(pool.map(self._open_one, files)) if len(files) > 1 else [self._open_one(item) for item in files]
        self._store_groups(opened, lambda im: (im.size[1], im.size[0]), partial(self._upload_images, pool), dev, out)

    def load(self, paths: Sequence[str], dev) -> dict:
        """Decode the paths that are not cached; -> {path: (slab, slot) or the exception its decode raised}.  The frames of one
        call are never evicted by that call."""
        from . import preprocess as pp
        out = {p: hit for p in dict.fromkeys(paths) if (hit := self.lookup(p)) is not None}
        todo = [p for p in dict.fromkeys(paths) if p not in out]
        pool = pp._decode_pool(pp.decode_workers())
        for c0 in range(0, len(todo), UPLOAD_FRAMES):
            chunk = todo[c0:c0 + UPLOAD_FRAMES]
            read = list(pool.map(self._read_one, chunk)) if len(chunk) > 1 else [self._read_one(chunk[0])]
            self.decodes += len(chunk)
            files = [(p, k, data) for p, (k, data) in zip(chunk, read) if k is not None]
            taken = self._decode_on_device(files, dev, out)       # the device-route sizes first, then the Pillow groups
            out.update((p, err) for p, (k, err) in zip(chunk, read) if k is None)
            self._decode_with_pillow([item for item in files if item[0] not in taken], pool, dev, out)
        return out


_default_cache = None


def default_cache() -> FrameCache:
    global _default_cache
    if _default_cache is None:
        _default_cache = FrameCache()
    return _default_cache


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
            return ValueError(f"Input images must have the same dimensions. {p1!r} is {s1.h}x{s1.w}, {p2!r} is {s2.h}x{s2.w}")
        if s1.h < ssim.WIN or s1.w < ssim.WIN:
            return ValueError(f"win_size exceeds image extent. {p1!r} and {p2!r} are {s1.h}x{s1.w}; the window is {ssim.WIN}x{ssim.WIN}")
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
                scores = ssim.ssim_launch(slab.gray, idx, -1.0, slab.minmax).cpu().numpy()
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
                        ssim.ssim_launch(slab.gray, idx, -1.0, slab.minmax, out=scores[first:first + m])
                    else:
                        where = torch.tensor([i for i, _, _ in items], dtype=torch.int64).to(self.dev)
                        scores.index_copy_(0, where, ssim.ssim_launch(slab.gray, idx, -1.0, slab.minmax))
                    self.pairs_scored += m
        return scores, problems
