"""The plan and decide steps of hmm_segment_walk (hippomm_amd/csrc/segment_walk.hip) as a numpy model: a pure function of the
adjacent-pair scores, the flags, the frame times and the per-window sums of squares -- what the kernels restate.  Python floats
are IEEE doubles, so the arithmetic on times is the kernel's operation by operation; the level of a window is taken as far as the
rms in the track's dtype (the division in fp64) and compared with rms_cut, never turned into dB.

``mutant`` plants one of five mistakes, for the test that shows the planted cases notice each of them."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

DONE, FLAGGED, BOUND = 1, 2, 3
MUTANTS = ("audio_does_not_override", "le_for_lt", "offset_zero_included", "clamp_before_audio", "unclipped_length_in_mean")


@dataclass
class Params:
    total: float
    max_dur: float
    min_dur: float
    sim_threshold: float
    rate: int = 0                      # 0: no audio
    track_len: int = 0
    dtype: type = np.float64           # the track's
    rms_cut: float = 0.0
    silent_without_rms: bool = False

    @property
    def window(self) -> int:
        return int(0.5 * self.rate)


def step_span(p: Params, start: float, mutant: Optional[str] = None) -> Tuple[float, int, int, int]:
    """-> (current_end, S, first offset, number of windows): window k starts at S + first_off - k * window."""
    end = min(start + p.max_dur, p.total)
    if not p.rate:
        return end, 0, 0, 0
    S, E = int(start * p.rate), int(end * p.rate)
    first_off = E - S - p.window
    if mutant == "offset_zero_included":
        n = first_off // p.window + 1 if first_off >= 0 else 0
    else:
        n = -(-first_off // p.window) if first_off > 0 else 0
    return end, S, first_off, n


def window_rows(p: Params, start: float, mutant: Optional[str] = None) -> List[Tuple[int, int]]:
    """The (start, length) table the plan step writes for the step that begins at `start`: numpy's clipping of [lo, lo + window)."""
    _, S, first_off, n = step_span(p, start, mutant)
    rows = []
    for k in range(n):
        at = S + first_off - k * p.window
        lo = min(at, p.track_len)
        rows.append((lo, min(at + p.window, p.track_len) - lo))
    return rows


def silent(p: Params, total_sq, count: int) -> bool:
    """total_sq: the window's sum of squares, a scalar of the track's dtype."""
    T = p.dtype
    with np.errstate(all="ignore"):
        mean = T(np.float64(total_sq) / np.float64(count))
        rms = np.sqrt(mean)
    return bool(rms < p.rms_cut) if rms > 0 else p.silent_without_rms


def walk(p: Params, scores: Sequence[float], flags: Sequence[int], times: Sequence[float],
         window_sum: Optional[Callable[[int, int], object]], max_steps: int, mutant: Optional[str] = None):
    """-> (records, status, flagged_pair).  A record: (start, end, first_frame, last_frame, cut_pair, cut_window, pairs consulted,
    windows consulted).  window_sum(lo, count) gives the sum of squares of track[lo : lo + count] in the track's dtype."""
    times = np.asarray(times, dtype=np.float64)
    records, start = [], 0.0
    if not 0.0 < p.total:
        return records, DONE, -1
    below = (lambda a, b: a <= b) if mutant == "le_for_lt" else (lambda a, b: a < b)
    for _ in range(max_steps):
        end, S, first_off, n_windows = step_span(p, start, mutant)
        optimal_end = end
        first, last, cut_pair, pairs = 0, -1, -1, 0
        if len(times):
            first = int(np.searchsorted(times, start, "left"))
            last = int(np.searchsorted(times, end, "right")) - 1
            for k in range(last, first, -1):
                pairs += 1
                if flags[k - 1]:
                    return records, FLAGGED, k - 1
                if below(scores[k - 1], p.sim_threshold):
                    optimal_end, cut_pair = float(times[k]), k - 1
                    break
        if mutant == "clamp_before_audio" and optimal_end - start < p.min_dur:
            optimal_end = min(start + p.min_dur, p.total)
        cut_window, windows = -1, 0
        for k in range(n_windows):
            windows += 1
            at = S + first_off - k * p.window
            lo = min(at, p.track_len)
            count = min(at + p.window, p.track_len) - lo
            if silent(p, window_sum(lo, count), p.window if mutant == "unclipped_length_in_mean" else count):
                if not (mutant == "audio_does_not_override" and cut_pair >= 0):
                    optimal_end = at / p.rate
                cut_window = k
                break
        if mutant != "clamp_before_audio" and optimal_end - start < p.min_dur:
            optimal_end = min(start + p.min_dur, p.total)
        if len(times):
            last = max(int(np.searchsorted(times, optimal_end, "right")) - 1, first - 1)
        records.append((start, optimal_end, first, last, cut_pair, cut_window, pairs, windows))
        start = optimal_end
        if not start < p.total:
            return records, DONE, -1
    return records, BOUND, -1
