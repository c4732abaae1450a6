#!/usr/bin/env python3
"""Generate tests/golden/segmentation_golden.json by running the UNMODIFIED reference with the real skimage 0.18.3.

Run in the build container only (it needs the reference checkout and the skimage 0.18.3 tree of a Python 3.9 install, neither of
which exists on the GPU box):

    python tests/golden/make_segmentation_golden.py [--reference DIR] [--skimage DIR]

* HippocampalMemory._segment_sequence, _compute_frame_similarity and _compute_audio_level
  (hippomm/core/hippocampal_memory.py:980-1114) and batch_process.compute_frame_difference (hippomm/core/batch_process.py:32-69)
  are imported behind the stub modules of make_golden.py, and called unchanged.
* skimage.metrics.structural_similarity is the real 0.18.3 module file, loaded under this Python / NumPy 2 by registering its
  packages as empty namespaces and aliasing the NumPy names it still uses; the version is recorded.
* cv2.imread returns the recipe frame for a path and cv2.cvtColor takes channel 0: the recipes' frames are gray-replicated BGR,
  for which that is OpenCV's BGR2GRAY exactly.  A path with no recipe frame reads as None, as cv2.imread does for a missing file.

Only recipes, input hashes and the reference's outputs are written.
"""
from __future__ import annotations

import argparse
import json
import platform
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import segmentation_recipes as R  # noqa: E402
import ssim_oracle  # noqa: E402


def load_skimage_ssim(tree: str):
    root = Path(tree)
    src = root / "metrics" / "_structural_similarity.py"
    if not src.exists():
        raise SystemExit(f"skimage's structural_similarity not found at {src}")
    for alias, real in (("bool8", np.bool_), ("float_", np.float64), ("int_", np.int64), ("complex_", np.complex128)):
        if not hasattr(np, alias):
            setattr(np, alias, real)
    for name, sub in (("skimage", ""), ("skimage.metrics", "metrics"), ("skimage.util", "util"), ("skimage._shared", "_shared")):
        mod = types.ModuleType(name)
        mod.__path__ = [str(root / sub) if sub else str(root)]
        sys.modules[name] = mod
    import skimage.util.dtype as dtype
    sys.modules["skimage.util"].img_as_float = dtype.img_as_float
    import skimage.metrics._structural_similarity as mod
    version = next(line.split("=")[1].strip().strip("'\"") for line in (root / "__init__.py").read_text().splitlines()
                   if line.startswith("__version__"))
    return mod.structural_similarity, version


class FakeCv2(types.ModuleType):
    COLOR_BGR2GRAY = 6

    def __init__(self):
        super().__init__("cv2")
        self.images = {}

    def imread(self, path):
        img = self.images.get(path)
        return None if img is None else img.copy()

    def cvtColor(self, frame, code):
        assert code == self.COLOR_BGR2GRAY
        if frame is None:
            raise RuntimeError("cv2.error: (-215:Assertion failed) !_src.empty() in function 'cvtColor'")
        assert (frame[..., 0] == frame[..., 1]).all() and (frame[..., 0] == frame[..., 2]).all()
        return np.ascontiguousarray(frame[..., 0])


def import_reference(ref: str, ssim_fn, cv2):
    sys.modules["cv2"] = cv2
    import make_golden
    make_golden.REF = ref
    make_golden.import_reference()
    sys.modules["skimage.metrics"].structural_similarity = ssim_fn
    for name in ("tqdm", "yaml"):
        try:
            __import__(name)
        except ImportError:
            make_golden._stub(name)
    sys.modules.setdefault("tqdm", types.ModuleType("tqdm"))
    if not hasattr(sys.modules["tqdm"], "tqdm"):
        class _Bar:
            def __init__(self, *a, **k):
                pass

            def update(self, *a):
                pass

            def close(self):
                pass
        sys.modules["tqdm"].tqdm = _Bar
    import hippomm.core.hippocampal_memory as hm
    import hippomm.core.batch_process as bp
    hm.ssim = ssim_fn
    bp.ssim = ssim_fn
    hm.cv2 = cv2
    bp.cv2 = cv2
    return hm.HippocampalMemory, bp.compute_frame_difference


def _num(x):
    x = float(x)
    return None if np.isnan(x) else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--skimage", default="/opt/conda/lib/python3.9/site-packages/skimage")
    a = ap.parse_args()
    ssim_fn, sk_version = load_skimage_ssim(a.skimage)
    cv2 = FakeCv2()
    HM, diff_ref = import_reference(a.reference, ssim_fn, cv2)

    out = {"_generated_by": "tests/golden/make_segmentation_golden.py",
           "_env": {"numpy": np.__version__, "python": platform.python_version(), "skimage": sk_version},
           "_reference": {"similarity": "hippomm/core/hippocampal_memory.py:980-991",
                          "segment": "hippomm/core/hippocampal_memory.py:1002-1114",
                          "difference": "hippomm/core/batch_process.py:32-69"},
           "pairs": {}, "differences": {}, "segments": {}}

    sim = lambda p1, p2: HM._compute_frame_similarity(None, p1, p2)   # noqa: E731
    worst = 0.0
    for name in R.PAIR_CASES:
        g1, g2 = R.pair_case(name)
        cv2.images = {"a": R.bgr(g1), "b": R.bgr(g2)}
        with np.errstate(all="ignore"):
            s_range = sim("a", "b")
            d_bgr = diff_ref(R.bgr(g1), R.bgr(g2))
            d_gray = diff_ref(g1, g2)
        o = ssim_oracle.ssim(g1, g2)
        if np.isnan(s_range) != np.isnan(o) or (not np.isnan(o) and abs(o - s_range) > 1e-9):
            raise SystemExit(f"oracle disagrees with skimage on {name}: {o} vs {s_range}")
        if not np.isnan(o):
            worst = max(worst, abs(o - s_range))
        out["pairs"][name] = {"shape": list(g1.shape), "input_sha256": R.sha256(g1, g2), "range_of_a": int(g1.max()) - int(g1.min()),
                              "ssim_range_of_a": _num(s_range), "ssim_range_1_on_255": _num(1.0 - d_gray),
                              "difference_bgr": float(d_bgr), "difference_gray": float(d_gray)}
    for name in R.DIFF_FALLBACK_CASES:
        g1, g2 = R.diff_fallback_case(name)
        res = {}
        for form, (f1, f2) in (("gray", (g1, g2)), ("bgr", (R.bgr(g1), R.bgr(g2)))):
            try:
                with np.errstate(all="ignore"):
                    res[form] = {"value": float(diff_ref(f1, f2))}
            except Exception as exc:               # noqa: BLE001 - the reference's own exception is the expected output
                res[form] = {"raises": type(exc).__name__}
        out["differences"][name] = {"input_sha256": R.sha256(g1, g2), **res}

    for name in R.SEG_CASES:
        case = R.seg_case(name)
        frames, times, audio, sr = case["frames"], case["times"], case["audio"], case["sr"]
        names = [R.frame_name(i) for i in range(len(frames))] if frames is not None else None
        cv2.images = {n: R.bgr(f) for n, f in zip(names, frames)} if frames is not None else {}
        consulted = []
        mx, mn, thr, sil = case["params"]

        def spy(p1, p2):
            i, j = names.index(p1), names.index(p2)
            rec = {"pair": [i, j]}
            consulted.append(rec)
            with np.errstate(all="ignore"):
                s = sim(p1, p2)
            rec["score"] = _num(s)
            if not np.isnan(s) and abs(s - thr) < 1e-9:
                raise SystemExit(f"{name}: consulted score {s} within 1e-9 of the threshold")
            return s

        self = types.SimpleNamespace(max_segment_duration=mx, min_segment_duration=mn, frame_similarity_threshold=thr,
                                     audio_silence_threshold=sil, _compute_frame_similarity=spy,
                                     _compute_audio_level=lambda x, r: HM._compute_audio_level(None, x, r))
        entry = {"params": list(case["params"]), "n_frames": None if frames is None else len(frames),
                 "frame_shapes": None if frames is None else [list(f.shape) for f in frames],
                 "times": times, "sr": sr,
                 "input_sha256": R.sha256(*(frames or [])) if frames is not None else None,
                 "audio_sha256": None if audio is None else R.sha256(audio)}
        try:
            segs = HM._segment_sequence(self, video_frames=names, frame_times=times, audio_data=audio, audio_sample_rate=sr)
            entry["segments"] = [{"start": s.start_time, "end": s.end_time,
                                  "frames": None if s.frames is None else [names.index(f) for f in s.frames],
                                  "frame_times": s.frame_times,
                                  "audio": None if s.audio_data is None else [int(s.start_time * sr), int(s.end_time * sr),
                                                                             R.sha256(s.audio_data)]} for s in segs]
        except ValueError as exc:
            entry["raises"] = {"type": type(exc).__name__, "message": str(exc), "at_pair": consulted[-1]["pair"]}
            consulted[-1]["score"] = "raises"
        entry["consulted"] = consulted
        out["segments"][name] = entry
        print(f"{name:24s} segments={len(entry.get('segments', []))} consulted={len(consulted)} raises={'raises' in entry}")
    out["_oracle_vs_skimage_max_abs"] = worst
    (HERE / "segmentation_golden.json").write_text(json.dumps(out, indent=1))
    print("oracle vs skimage, worst |diff|:", worst)


if __name__ == "__main__":
    main()
