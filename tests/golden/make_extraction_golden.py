#!/usr/bin/env python3
"""Generate tests/golden/extraction_golden.json by running the UNMODIFIED reference loop with the real skimage 0.18.3.

Run in the build container only (it needs the reference checkout and the skimage 0.18.3 tree of a Python 3.9 install, neither of
which exists on the GPU box):

    python tests/golden/make_extraction_golden.py [--reference DIR] [--skimage DIR]

* batch_process.extract_frames_from_video (hippomm/core/batch_process.py:116-255) is imported behind the stub modules of
  make_golden.py, with the loaders of make_segmentation_golden.py, and called unchanged on every case of extraction_recipes.py.
* cv2.VideoCapture yields the recipe's frames, its fps and its frame count; cv2.cvtColor takes channel 0 (the frames are
  gray-replicated BGR, for which that is OpenCV's BGR2GRAY exactly); cv2.imwrite writes a stub file, or returns False on the calls
  the recipe names.
* The module's compute_frame_difference global is wrapped to record every diff it returns; the function itself is not changed.

A case whose consulted diff or running cumulative_diff comes within 1e-6 of the threshold is refused: the device's scores differ
from skimage's in the last bits (1.8e-11 at most in segmentation_golden.json), and no decision may hang on them.  Change the recipe
then, not the bound.  Only recipes, input hashes and the reference's outputs are written.
"""
from __future__ import annotations

import argparse
import json
import platform
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import extraction_recipes as X  # noqa: E402
import make_segmentation_golden as M  # noqa: E402
import segmentation_recipes as R  # noqa: E402

MARGIN = 1e-6
CAP_PROP_FPS, CAP_PROP_FRAME_COUNT = 5, 7


class FakeCv2(M.FakeCv2):
    """The cv2 of make_segmentation_golden.py plus the three calls of the extraction loop."""
    CAP_PROP_FPS, CAP_PROP_FRAME_COUNT = CAP_PROP_FPS, CAP_PROP_FRAME_COUNT

    def __init__(self):
        super().__init__()
        self.video, self.fps, self.fail_calls = None, 0.0, ()
        self.writes, self.failed_paths = 0, []

    def VideoCapture(self, path):             # noqa: N802 - cv2's name
        fake = self

        class Capture:
            def __init__(self):
                self.at = 0

            def isOpened(self):               # noqa: N802
                return True

            def get(self, prop):
                return {CAP_PROP_FPS: fake.fps, CAP_PROP_FRAME_COUNT: float(len(fake.video))}[prop]

            def read(self):
                if self.at >= len(fake.video):
                    return False, None
                self.at += 1
                return True, R.bgr(fake.video[self.at - 1])

            def release(self):
                pass
        return Capture()

    def imwrite(self, path, frame):
        self.writes += 1
        if self.writes in self.fail_calls:
            self.failed_paths.append(path)
            return False
        Path(path).write_bytes(b"stub")
        return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--skimage", default="/opt/conda/lib/python3.9/site-packages/skimage")
    a = ap.parse_args()
    ssim_fn, sk_version = M.load_skimage_ssim(a.skimage)
    cv2 = FakeCv2()
    M.import_reference(a.reference, ssim_fn, cv2)
    import hippomm.core.batch_process as bp
    metadata = {}                             # yaml.dump receives the loop's failed_saves; the file itself is not part of the golden
    bp.yaml = types.SimpleNamespace(dump=lambda data, *args, **kw: metadata.update(data), safe_load=lambda *args, **kw: {})
    diff_ref = bp.compute_frame_difference

    out = {"_generated_by": "tests/golden/make_extraction_golden.py",
           "_env": {"numpy": np.__version__, "python": platform.python_version(), "skimage": sk_version},
           "_reference": {"loop": "hippomm/core/batch_process.py:116-255"}, "_margin": MARGIN, "cases": {}}
    for name in X.CASES:
        c = X.case(name)
        video = X.gray_frames(name)
        cv2.video, cv2.fps, cv2.fail_calls = video, c["fps"], tuple(c["fail_calls"])
        cv2.writes, cv2.failed_paths = 0, []
        consulted = []

        def spy(frame1, frame2):
            with np.errstate(all="ignore"):
                d = diff_ref(frame1, frame2)
            consulted.append(float(d))
            return d

        bp.compute_frame_difference = spy
        try:
            with tempfile.TemporaryDirectory(prefix="hmm_extraction_golden_") as tmp:
                frames_dir = Path(tmp) / "frames" / "video"
                for count in c["existing"]:
                    p = X.frame_path(frames_dir, count, c["fps"])
                    p.parent.mkdir(parents=True, exist_ok=True)
                    p.write_bytes(b"there before")
                paths, times, duration = bp.extract_frames_from_video("video.mp4", Path(tmp), "video",
                                                                      check_interval=c["check_interval"])
                assert all(Path(p).exists() for p in paths)
        finally:
            bp.compute_frame_difference = diff_ref
        kept = [int(Path(p).stem.split("_")[1]) for p in paths]
        failed = [int(Path(p).stem.split("_")[1]) for p in cv2.failed_paths]
        assert [str(X.frame_path(frames_dir, k, c["fps"])) for k in kept] == list(paths)

        # which frames the diffs belong to, and the margin: the reference's own rules replayed over its recorded diffs
        counts, replayed, margin, cum, last_save, anchor, k = [], [], float("inf"), 0.0, 0.0, False, 0
        for i in range(len(video)):
            t = i / c["fps"]
            save = not anchor
            if anchor and t - last_save >= 1.0 and i % c["check_interval"] == 0:
                d = consulted[k]
                k += 1
                cum += d
                counts.append(i)
                margin = min(margin, abs(d - X.THRESHOLD), abs(cum - X.THRESHOLD))
                save = d > X.THRESHOLD or cum > X.THRESHOLD
            if save and i not in failed:
                anchor, cum, last_save = True, 0.0, t
                replayed.append(i)
        if k != len(consulted) or replayed != kept or metadata["failed_saves"] != len(failed):
            raise SystemExit(f"{name}: the replay of the recorded diffs does not give the reference's lists")
        if margin < MARGIN:
            raise SystemExit(f"{name}: a consulted diff or cumulative_diff is within {margin:.3e} of the threshold; change the recipe")
        out["cases"][name] = {"recipe": {k2: (list(v) if isinstance(v, tuple) else v) for k2, v in c.items()},
                              "input_sha256": R.sha256(video), "kept": kept, "frame_times": [float(t) for t in times],
                              "failed_saves": int(metadata["failed_saves"]), "failed_frames": failed,
                              "consulted": [[i, d] for i, d in zip(counts, consulted)],
                              "margin": None if margin == float("inf") else margin}
        print(f"{name:26s} kept={kept} failed={failed} consulted={len(consulted)} margin={margin:.3e}")
    (HERE / "extraction_golden.json").write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
