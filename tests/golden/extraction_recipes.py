"""Seeded videos for the frame-extraction golden (extraction_golden.json): make_extraction_golden.py runs the reference's
extract_frames_from_video on them, the tests regenerate the same frames.  Frames are gray-replicated BGR built on
segmentation_recipes.gray_frame, so OpenCV's BGR2GRAY of a frame is its channel 0 exactly."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import segmentation_recipes as R

N_FRAMES = 601
CUT_AT = 330                              # the drifting scene changes its picture here
THRESHOLD = 0.3                           # extract_frames_from_video's max_diff_threshold default

# name -> size, scene, fps, check_interval; fail_calls: the cv2.imwrite calls (counted from 1) that return False;
# existing: frame counts whose file is there before the run; n: frames in the video
CASES = {
    "drift_48x64_fps30": dict(h=48, w=64, kind="drift", fps=30.0),
    "drift_48x64_fps60": dict(h=48, w=64, kind="drift", fps=60.0),
    "drift_48x64_fps25": dict(h=48, w=64, kind="drift", fps=25.0),
    "drift_48x64_fps29.97": dict(h=48, w=64, kind="drift", fps=29.97),
    "drift_48x64_fps12": dict(h=48, w=64, kind="drift", fps=12.0),
    "drift_48x64_interval15": dict(h=48, w=64, kind="drift", fps=30.0, check_interval=15),
    "drift_43x263_fps30": dict(h=43, w=263, kind="drift", fps=30.0),
    "drift_7x7_fps30": dict(h=7, w=7, kind="drift", fps=30.0),
    "static_48x64_fps30": dict(h=48, w=64, kind="static", fps=30.0),
    "static_43x263_fps25": dict(h=43, w=263, kind="static", fps=25.0),
    "static_7x7_fps30": dict(h=7, w=7, kind="static", fps=30.0),
    "fail_first_write": dict(h=48, w=64, kind="drift", fps=30.0, fail_calls=(1,)),
    "fail_third_write": dict(h=48, w=64, kind="drift", fps=30.0, fail_calls=(3,)),
    "fail_two_in_a_row": dict(h=48, w=64, kind="drift", fps=30.0, fail_calls=(2, 3)),
    "fail_first_two_writes": dict(h=43, w=263, kind="drift", fps=30.0, fail_calls=(1, 2)),
    "existing_file": dict(h=48, w=64, kind="drift", fps=30.0, existing=(90,)),
    "single_frame": dict(h=48, w=64, kind="drift", fps=30.0, n=1),
}


def case(name: str) -> dict:
    c = dict(check_interval=30, fail_calls=(), existing=(), n=N_FRAMES)
    c.update(CASES[name])
    return c


@lru_cache(maxsize=None)
def _picture(kind: str, i: int, h: int, w: int) -> np.ndarray:
    if kind == "drift":                   # one picture per 30 frames, drifting by a column each; a cut at CUT_AT
        return R.gray_frame(700 + (i >= CUT_AT), i // 30, h, w, noise=2.0, shift=1)
    if kind == "static":                  # one picture, fresh noise on every frame
        return R.gray_frame(710, i, h, w, noise=1.0, shift=0)
    raise KeyError(kind)


def gray_frames(name: str) -> np.ndarray:
    """(n, h, w) uint8: the gray frames of the case's video."""
    c = case(name)
    return np.stack([_picture(c["kind"], i, c["h"], c["w"]) for i in range(c["n"])])


def frame_path(frames_dir, frame_count: int, fps: float):
    """The reference's path of a saved frame (batch_process.py:204-207)."""
    return frames_dir / f"t_{int(frame_count / fps):04d}" / f"frame_{frame_count:06d}.jpg"
