"""Host model of the reference's frame-extraction loop (hippomm/core/batch_process.py:179-228) as a pure function of the frame
counts, the frame rate, a difference function and the outcomes of the saves -- what hmm_extract_walk and FrameExtractor restate."""
from __future__ import annotations

from typing import Callable, Iterable, List, NamedTuple, Tuple


class Walk(NamedTuple):
    kept: List[int]                          # frame counts whose save succeeded
    frame_times: List[float]
    failed_saves: int
    consulted: List[Tuple[int, float]]       # (frame count, diff) of every compute_frame_difference call, in order
    records: List[tuple]                     # per frame looked at: (frame count, compared, saved, diff, cumulative, last_save_time)


def walk(n_frames: int, fps: float, diff: Callable[[int, int], float], save_ok: Callable[[int], bool] = lambda i: True, *,
         check_interval: int = 30, max_diff_threshold: float = 0.3, min_gap: float = 1.0) -> Walk:
    """``diff(frame, anchor)`` is asked exactly where the reference calls compute_frame_difference(frame, last_saved_frame);
    ``save_ok(frame)`` where it calls save_frame."""
    kept, times, consulted, records = [], [], [], []
    anchor, cumulative, last_save_time, failed = None, 0.0, 0.0, 0
    for i in range(n_frames):
        t = i / fps
        if anchor is not None and i % check_interval != 0:
            continue                                         # the reference does nothing with these frames
        save, compared, saved, d = False, 0, 0, 0.0
        if anchor is None:
            save = True
        elif t - last_save_time >= min_gap:
            d = diff(i, anchor)
            compared = 1
            consulted.append((i, d))
            cumulative += d
            save = d > max_diff_threshold or cumulative > max_diff_threshold
        if save:
            if save_ok(i):
                kept.append(i)
                times.append(t)
                anchor, cumulative, last_save_time, saved = i, 0.0, t, 1
            else:
                failed += 1
        records.append((i, compared, saved, d, cumulative, last_save_time))
    return Walk(kept, times, failed, consulted, records)


def recorded_diffs(consulted: Iterable) -> Callable[[int, int], float]:
    """A diff function that replays a golden case's consulted list, and insists on being asked in its order."""
    queue = [(int(i), float(d)) for i, d in consulted]

    def diff(frame: int, anchor: int) -> float:
        i, d = queue.pop(0)
        assert i == frame, f"the walk consults frame {frame}, the reference consulted {i}"
        return d
    diff.left = queue
    return diff
