"""CPU: the segmentation window walk reproduces the reference's segments from its own scores, the SSIM oracle agrees with
skimage 0.18.3 as recorded in the golden, the new C-ABI entry points report argument errors without a GPU, and the public calls
refuse to run without one."""
import json
from pathlib import Path

import numpy as np
import pytest

import segmentation_recipes as R
import ssim_oracle

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "segmentation_golden.json").read_text())


def _score_window(entry, log):
    table = {tuple(c["pair"]): c["score"] for c in entry["consulted"]}

    def score_window(pairs):
        for pair in pairs:
            log.append(list(pair))
            s = table[tuple(pair)]                     # KeyError: the walk consulted a pair the reference did not
            if s == "raises":
                raise ValueError(entry["raises"]["message"])
            yield np.nan if s is None else s
    return score_window


@pytest.mark.parametrize("name", R.SEG_CASES)
def test_walk_segments_reproduces_the_golden(name):
    from hippomm_amd.segmentation import walk_segments
    entry = GOLDEN["segments"][name]
    case = R.seg_case(name)
    assert (R.sha256(*case["frames"]) if case["frames"] is not None else None) == entry["input_sha256"]
    names = [R.frame_name(i) for i in range(len(case["frames"]))] if case["frames"] is not None else None
    log = []
    mx, mn, thr, sil = entry["params"]
    args = (names, case["times"], case["audio"], case["sr"], _score_window(entry, log), mx, mn, thr, sil)
    if "raises" in entry:
        with pytest.raises(ValueError):
            walk_segments(*args)
    else:
        segs = walk_segments(*args)
        got = [{"start": s.start_time, "end": s.end_time,
                "frames": None if s.frames is None else [names.index(f) for f in s.frames], "frame_times": s.frame_times,
                "audio": None if s.audio_data is None else [int(s.start_time * case["sr"]), int(s.end_time * case["sr"]),
                                                           R.sha256(s.audio_data)]} for s in segs]
        assert got == entry["segments"]
    assert log == [c["pair"] for c in entry["consulted"]]


def test_walk_segments_refuses_to_loop_forever():
    from hippomm_amd.segmentation import walk_segments

    def score_window(pairs):
        for k, _ in enumerate(pairs):
            yield 1.0 if k == 0 else 0.0               # breaks at (2, 1): the end is frame 2's time, 0.0, the start again
    times = [0.0, 0.0, 0.0, 3.0]
    with pytest.raises(ValueError, match="loop forever"):
        walk_segments(["a", "b", "c", "d"], times, None, None, score_window, 10.0, 0.0, 0.95, -40)


def test_walk_segments_early_returns():
    from hippomm_amd.segmentation import walk_segments
    assert walk_segments(None, None, None, None, None) == []
    assert walk_segments([], [], None, None, None) == []
    assert walk_segments(None, None, np.zeros(10, np.float32), None, None) == []


@pytest.mark.parametrize("name", R.PAIR_CASES)
def test_oracle_matches_skimage_in_the_golden(name):
    entry = GOLDEN["pairs"][name]
    a, b = R.pair_case(name)
    assert R.sha256(a, b) == entry["input_sha256"]
    for key, rng in (("ssim_range_of_a", None), ("ssim_range_1_on_255", 255.0)):
        o = ssim_oracle.ssim(a, b, rng)
        want = entry[key]
        if want is None:
            assert np.isnan(o), (key, o)
        else:
            assert abs(o - want) <= 1e-9, (key, o, want)


def test_oracle_gray_rule_is_identity_on_gray_replicated_frames():
    v = np.arange(256, dtype=np.uint8)
    assert (ssim_oracle.gray_from_bgr(R.bgr(v[None, :]))[0] == v).all()


def test_ssim_argument_errors_are_reported_without_a_gpu():
    import ctypes as C
    from hippomm_amd import _lib
    lib = _lib.load()
    dummy = 16
    pairs = (C.c_int32 * 4)(0, 1, 1, 2)
    ws = lib.hmm_ssim_pairs_workspace_bytes(120, 160, 2)
    assert ws >= 2 * 8 and lib.hmm_ssim_pairs_workspace_bytes(6, 160, 2) == 0
    rc = lib.hmm_ssim_pairs(None, 3, 120, 160, pairs, 2, 255.0, None, dummy, dummy, ws, None)
    assert rc == -1 and b"null pointer" in lib.hmm_last_error()
    rc = lib.hmm_ssim_pairs(dummy, 3, 6, 160, pairs, 2, 255.0, None, dummy, dummy, ws, None)
    assert rc == -1 and b"win_size exceeds image extent" in lib.hmm_last_error()
    rc = lib.hmm_ssim_pairs(dummy, 2, 120, 160, pairs, 2, 255.0, None, dummy, dummy, ws, None)
    assert rc == -1 and b"outside the 2 frames" in lib.hmm_last_error()
    rc = lib.hmm_ssim_pairs(dummy, 3, 120, 160, pairs, 0, 255.0, None, dummy, dummy, ws, None)
    assert rc == -1 and b"n_pairs=0" in lib.hmm_last_error()
    rc = lib.hmm_ssim_pairs(dummy, 3, 120, 160, pairs, 2, -1.0, None, dummy, dummy, ws, None)
    assert rc == -1 and b"needs minmax_dev" in lib.hmm_last_error()
    rc = lib.hmm_ssim_pairs(dummy, 3, 120, 160, pairs, 2, 255.0, None, dummy, dummy, ws - 1, None)
    assert rc == -2 and b"workspace" in lib.hmm_last_error()
    rc = lib.hmm_gray_u8(dummy, 0, 10, 10, 0, dummy, dummy, None)
    assert rc == -1 and b"bad shape" in lib.hmm_last_error()
    rc = lib.hmm_gray_u8(dummy, 1, 10, 10, 7, dummy, dummy, None)
    assert rc == -1 and b"channel_order" in lib.hmm_last_error()
    rc = lib.hmm_gray_u8(dummy, 1, 10, 10, 0, None, dummy, None)
    assert rc == -1 and b"null gray output" in lib.hmm_last_error()


def test_frame_difference_rejects_other_dtypes():
    from hippomm_amd.ssim import compute_frame_difference
    with pytest.raises(TypeError):
        compute_frame_difference(np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float32))


def test_public_calls_have_no_cpu_fallback(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from hippomm_amd import _lib, segmentation as seg
    frame = np.zeros((16, 16, 3), np.uint8)
    calls = [lambda: seg.compute_frame_difference(frame, frame),
             lambda: seg._compute_frame_similarity(None, "a.png", "b.png"),
             lambda: seg.segment_sequence(["a.png", "b.png"], [0.0, 1.0]),
             lambda: seg.gray_frames(torch.zeros((1, 8, 8, 3), dtype=torch.uint8)),
             lambda: seg.ssim_pairs(torch.zeros((2, 8, 8), dtype=torch.uint8), [[0, 1]])]
    for call in calls:
        with pytest.raises(_lib.HippoMMHipError, match="no CPU fallback"):
            call()


def test_audio_only_segmentation_runs_on_the_host():
    from hippomm_amd.segmentation import segment_sequence
    entry = GOLDEN["segments"]["audio_only"]
    case = R.seg_case("audio_only")
    segs = segment_sequence(None, None, case["audio"], case["sr"])
    assert [[s.start_time, s.end_time] for s in segs] == [[s["start"], s["end"]] for s in entry["segments"]]


# the public names of the frame path's other stages, and the module each one lives in now: segmentation re-exports exactly these
RE_EXPORTS = {
    "ssim": ["WIN", "gray_frames", "ssim_pairs", "compute_frame_difference"],
    "resize": ["RESIZE_COEF_SCALE", "RESIZE_LINEAR", "RESIZE_AREA2X", "resize_linear_tables", "resize_mode", "resize_frames"],
    "retrieval": ["RECALL_SIZE", "RECALL_SIMILARITY_CUT", "walk_recall_window"],
    "frame_cache": ["CACHE_BYTES", "UPLOAD_FRAMES", "ADJACENT_CHUNK", "FrameCache", "default_cache", "PathScorer"],
    "frame_extraction": ["SAVE_QUALITY", "SAVE_SUBSAMPLING", "CHECK_INTERVAL", "MAX_DIFF_THRESHOLD", "MIN_SAVE_GAP", "EXTRACT_BATCH",
                         "EXTRACT_STATE", "EXTRACT_RECORD", "ExtractionState", "save_frame", "save_frames", "extraction_records",
                         "FrameExtractor", "extract_frames"],
}
OWN = ["MAX_SEGMENT_DURATION", "MIN_SEGMENT_DURATION", "FRAME_SIMILARITY_THRESHOLD", "AUDIO_SILENCE_THRESHOLD", "SEGMENT_RECORD",
       "SEGMENT_STATE", "WALK_DONE", "WALK_FLAGGED", "WALK_BOUND", "MAX_DEVICE_STEPS", "MAX_DEVICE_WINDOWS", "SequenceSegment",
       "audio_level", "walk_segments", "silence_cut", "segment_sequence"]


def test_the_old_import_paths_give_the_objects_of_the_new_home_modules():
    import importlib
    import types
    from hippomm_amd import segmentation
    for home, names in RE_EXPORTS.items():
        module = importlib.import_module(f"hippomm_amd.{home}")
        for name in names:
            assert getattr(segmentation, name) is getattr(module, name), (home, name)
    # the list is complete, and nothing private came along: every public name of the module is its own or one of the above
    public = {name for name, value in vars(segmentation).items()
              if not name.startswith("_") and not isinstance(value, types.ModuleType)}
    borrowed = {"annotations", "dataclass", "lru_cache", "Callable", "Iterable", "List", "Optional", "Tuple"}   # its own imports
    assert public - borrowed == set(OWN) | {name for names in RE_EXPORTS.values() for name in names}
    for home in RE_EXPORTS:
        module = importlib.import_module(f"hippomm_amd.{home}")
        private = {name for name, value in vars(module).items()
                   if name.startswith("_") and not name.startswith("__") and not isinstance(value, types.ModuleType)}
        assert not private & set(vars(segmentation)), (home, private & set(vars(segmentation)))
