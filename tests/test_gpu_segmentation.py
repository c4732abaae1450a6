"""GPU: hmm_gray_u8 / hmm_ssim_pairs and the segmentation drop-ins against the golden recorded from the reference with skimage
0.18.3 (tests/golden/segmentation_golden.json) and against the numpy oracle (tests/ssim_oracle.py)."""
import json
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import segmentation_recipes as R
import ssim_oracle

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "segmentation_golden.json").read_text())


def _close(got, want, tol=1e-9):
    if want is None:
        return np.isnan(got)
    return abs(float(got) - want) <= tol


def test_ssim_pairs_matches_the_golden_in_both_range_modes():
    from hippomm_amd.ssim import ssim_pairs
    for name in R.PAIR_CASES:
        a, b = R.pair_case(name)
        g = torch.from_numpy(np.stack([a, b])).cuda()
        entry = GOLDEN["pairs"][name]
        s_range = ssim_pairs(g, [[0, 1]]).cpu().numpy()[0]
        s_255 = ssim_pairs(g, [[0, 1]], data_range=255.0).cpu().numpy()[0]
        assert _close(s_range, entry["ssim_range_of_a"]), (name, s_range, entry["ssim_range_of_a"])
        assert _close(s_255, entry["ssim_range_1_on_255"]), (name, s_255, entry["ssim_range_1_on_255"])


def test_consecutive_1080p_pairs_match_the_oracle_and_are_deterministic():
    from hippomm_amd.ssim import ssim_pairs
    frames = R.consecutive_1080p(17)
    g = torch.from_numpy(frames).cuda()
    pairs = [[i + 1, i] for i in range(16)]
    got = ssim_pairs(g, pairs).cpu().numpy()
    want = np.array([ssim_oracle.ssim(frames[i + 1], frames[i]) for i in range(16)])
    assert np.abs(got - want).max() <= 1e-9, np.abs(got - want).max()
    again = ssim_pairs(g, pairs).cpu().numpy()
    assert again.tobytes() == got.tobytes()
    single = np.array([ssim_pairs(g, [p]).cpu().numpy()[0] for p in pairs[::5]])
    assert single.tobytes() == got[::5].tobytes()
    # more than one launch chunk of pairs (128 per launch): still the same bits per pair
    many = ssim_pairs(g, pairs * 9).cpu().numpy()
    assert many.tobytes() == np.tile(got, 9).tobytes()


def test_gray_kernel_is_exact_over_every_colour():
    from hippomm_amd.ssim import gray_frames
    c = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], axis=1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    want = ssim_oracle.gray_from_bgr(img)                       # channel 0 is B
    t = torch.from_numpy(img).cuda()
    got, mm = gray_frames(t, "BGR", return_minmax=True)
    assert np.array_equal(got.cpu().numpy(), want)
    assert mm.cpu().numpy().tolist() == [[int(want.min()), int(want.max())]]
    got_rgb = gray_frames(t.flip(-1), "RGB").cpu().numpy()      # the same pixels with the channels reversed
    assert np.array_equal(got_rgb, want)


def test_compute_frame_difference_matches_the_golden():
    from hippomm_amd.ssim import compute_frame_difference
    for name in R.PAIR_CASES:
        a, b = R.pair_case(name)
        entry = GOLDEN["pairs"][name]
        assert abs(compute_frame_difference(R.bgr(a), R.bgr(b)) - entry["difference_bgr"]) <= 1e-9, name
        assert abs(compute_frame_difference(a, b) - entry["difference_gray"]) <= 1e-9, name
        assert abs(compute_frame_difference(R.bgr(a), b) - entry["difference_gray"]) <= 1e-9, name
    for name in R.DIFF_FALLBACK_CASES:
        g1, g2 = R.diff_fallback_case(name)
        entry = GOLDEN["differences"][name]
        for form, (f1, f2) in (("gray", (g1, g2)), ("bgr", (R.bgr(g1), R.bgr(g2)))):
            want = entry[form]
            if "raises" in want:
                with pytest.raises(Exception) as info:
                    compute_frame_difference(f1, f2)
                assert type(info.value).__name__ == want["raises"], (name, form)
            else:
                assert compute_frame_difference(f1, f2) == want["value"], (name, form)


def _write_frames(folder, frames, ext="png"):
    from PIL import Image
    paths = []
    for i, f in enumerate(frames):
        p = str(folder / R.frame_name(i, ext))
        Image.fromarray(R.bgr(f)).save(p)
        paths.append(p)
    return paths


def test_compute_frame_similarity_matches_the_golden(tmp_path):
    from hippomm_amd.segmentation import _compute_frame_similarity
    for name in R.PAIR_CASES:
        if name.startswith("1080"):
            continue
        a, b = R.pair_case(name)
        (tmp_path / name).mkdir()
        pa, pb = _write_frames(tmp_path / name, [a, b])
        got = _compute_frame_similarity(types.SimpleNamespace(), pa, pb)
        assert _close(got, GOLDEN["pairs"][name]["ssim_range_of_a"]), name


def _segments_as_golden(segs, paths, sr):
    return [{"start": s.start_time, "end": s.end_time,
             "frames": None if s.frames is None else [paths.index(f) for f in s.frames], "frame_times": s.frame_times,
             "audio": None if s.audio_data is None else [int(s.start_time * sr), int(s.end_time * sr), R.sha256(s.audio_data)]}
            for s in segs]


@pytest.mark.parametrize("name", R.SEG_CASES)
def test_segment_sequence_matches_the_golden(name, tmp_path):
    from hippomm_amd.segmentation import _segment_sequence, segment_sequence
    entry = GOLDEN["segments"][name]
    case = R.seg_case(name)
    paths = _write_frames(tmp_path, case["frames"]) if case["frames"] is not None else None
    mx, mn, thr, sil = entry["params"]
    kw = dict(max_segment_duration=mx, min_segment_duration=mn, frame_similarity_threshold=thr, audio_silence_threshold=sil)
    if "raises" in entry:
        with pytest.raises(ValueError, match="same dimensions"):
            segment_sequence(paths, case["times"], case["audio"], case["sr"], **kw)
        return
    segs = segment_sequence(paths, case["times"], case["audio"], case["sr"], **kw)
    assert _segments_as_golden(segs, paths, case["sr"]) == entry["segments"]
    me = types.SimpleNamespace(**kw)                            # the method form, bound to any object with the four attributes
    segs = _segment_sequence(me, video_frames=paths, frame_times=case["times"], audio_data=case["audio"],
                             audio_sample_rate=case["sr"])
    assert _segments_as_golden(segs, paths, case["sr"]) == entry["segments"]


def test_unreadable_frames_raise_only_where_consulted(tmp_path):
    from hippomm_amd.segmentation import segment_sequence
    entry = GOLDEN["segments"]["cuts_default"]
    case = R.seg_case("cuts_default")
    paths = _write_frames(tmp_path, case["frames"])
    consulted = {i for c in entry["consulted"] for i in c["pair"]}
    unconsulted = min(set(range(len(paths))) - consulted)
    Path(paths[unconsulted]).write_bytes(b"not an image")
    segs = segment_sequence(paths, case["times"])
    assert _segments_as_golden(segs, paths, None) == entry["segments"]
    Path(paths[entry["consulted"][0]["pair"][0]]).write_bytes(b"not an image")
    with pytest.raises(OSError, match=R.frame_name(entry["consulted"][0]["pair"][0])):
        segment_sequence(paths, case["times"])


def test_jpeg_path_equals_tensor_path_on_the_same_decode(tmp_path):
    from PIL import Image
    from hippomm_amd.segmentation import _compute_frame_similarity
    from hippomm_amd.ssim import gray_frames, ssim_pairs
    rng = np.random.default_rng(5)
    paths, rgbs = [], []
    for i in range(2):
        img = rng.integers(0, 256, (90, 160, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(img).resize((640, 360), Image.BICUBIC))
        p = str(tmp_path / f"f{i}.jpg")
        Image.fromarray(img).save(p, quality=85)
        paths.append(p)
        rgbs.append(np.asarray(Image.open(p).convert("RGB")))
    got = _compute_frame_similarity(None, paths[0], paths[1])
    gray = gray_frames(torch.from_numpy(np.stack(rgbs)).cuda(), "RGB")
    want = ssim_pairs(gray, [[0, 1]]).cpu().numpy()[0]
    assert np.float64(got).tobytes() == np.float64(want).tobytes()


def test_back_to_back_uploads_do_not_overwrite_a_copy_in_flight():
    """The staging buffer is reused without a host synchronisation after each upload: the second call has to wait for the first
    call's copy before it rewrites the buffer (``PinnedStage.wait``).  Two uploads of 16 frames of 1080 x 1920 x 3 (about 100 MB
    each) with different contents, compared on the device after both calls have returned; then a 7 x 7 frame difference straight
    after a large upload, which shares the buffer, against its value on a quiet stream.  Measured on one MI355X host: the call
    returns after 4.3 ms with its copy still pending for another 1.8 ms, so the second call does meet a copy in flight."""
    from hippomm_amd import _lib
    from hippomm_amd.ssim import compute_frame_difference, upload_frames
    dev = _lib.require_gpu()
    rng = np.random.default_rng(1615)
    first = rng.integers(0, 256, (16, 1080, 1920, 3), dtype=np.uint8)
    second = rng.integers(0, 256, (16, 1080, 1920, 3), dtype=np.uint8)
    small = rng.integers(0, 256, (2, 7, 7, 3), dtype=np.uint8)
    torch.cuda.synchronize()
    quiet = compute_frame_difference(small[0], small[1])
    torch.cuda.synchronize()
    up1 = upload_frames(list(first), dev)
    up2 = upload_frames(list(second), dev)
    want1, want2 = torch.from_numpy(first).to(dev), torch.from_numpy(second).to(dev)
    assert torch.equal(up1, want1) and torch.equal(up2, want2)
    del want1, want2
    upload_frames(list(first), dev)
    busy = compute_frame_difference(small[0], small[1])
    assert busy == quiet and np.isfinite(quiet)
