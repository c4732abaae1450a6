"""GPU: the frame-extraction walk (hmm_extract_walk behind extraction_records, FrameExtractor and extract_frames) against the golden
made by the unmodified reference loop (tests/golden/extraction_golden.json): kept frames, times, failed saves and consulted frames
equal, diffs within 1e-9 of skimage's, files the bytes save_frames writes; every compared diff the bits of 1 - ssim_pairs; the
records those of the host loop built from compute_frame_difference; the same bits whatever the batch; and the frames it saves
resident for segment_sequence and extract_features."""
import json
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE / "golden"))
import extraction_model as model  # noqa: E402
import extraction_recipes as X  # noqa: E402
import segmentation_recipes as R  # noqa: E402
from oracle import imagebind_oracle as ib  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((HERE / "golden" / "extraction_golden.json").read_text())["cases"]
FIELDS = ["frame_count", "compared", "saved", "has_anchor_after", "diff", "cumulative_after", "last_save_time_after"]


@pytest.fixture(scope="module")
def dev():
    from hippomm_amd import _lib
    return _lib.require_gpu()


@lru_cache(maxsize=None)
def _video(name):
    video = X.gray_frames(name)
    video.setflags(write=False)
    return video


def _fail_saves(monkeypatch, failed):
    """save_frames answers False for these frame counts and writes nothing for them: the golden's failing cv2.imwrite calls."""
    from hippomm_amd import frame_extraction as seg             # the module whose FrameExtractor looks save_frames up
    real, names = seg.save_frames, {f"frame_{i:06d}.jpg" for i in failed}

    def patched(frames, paths, **kw):
        frames, paths = list(frames), [Path(p) for p in paths]
        go = [k for k, p in enumerate(paths) if p.name not in names]
        done = real([frames[k] for k in go], [paths[k] for k in go], **kw) if go else []
        out = [False] * len(paths)
        for k, ok in zip(go, done):
            out[k] = ok
        return out
    monkeypatch.setattr(seg, "save_frames", patched)
    return real


def _extract(name, frames_dir, monkeypatch, **kw):
    from hippomm_amd import segmentation as seg
    g, c = GOLDEN[name], X.case(name)
    for count in c["existing"]:
        p = X.frame_path(frames_dir, count, c["fps"])
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"there before")
    _fail_saves(monkeypatch, g["failed_frames"])
    ex = seg.FrameExtractor(c["fps"], frames_dir, check_interval=c["check_interval"], **kw)
    for i, gray in enumerate(_video(name)):
        ex.push(i, R.bgr(gray))
    ex.flush()
    return ex


def _bits(records):
    """The records without the slot numbers (those depend on the batch), floats as bit patterns."""
    return [tuple(v.hex() if isinstance(v, float) else int(v) for v in (r[f].item() for f in FIELDS)) for r in records]


# ---- 1, 4: the golden ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.CASES))
def test_golden_case(dev, name, tmp_path, monkeypatch):
    from hippomm_amd import extract_frames, segmentation as seg
    g, c = GOLDEN[name], X.case(name)
    video = _video(name)
    assert R.sha256(video) == g["input_sha256"]
    real_save = seg.save_frames
    ex = _extract(name, tmp_path / "a", monkeypatch)
    assert ex.frame_paths == [str(X.frame_path(tmp_path / "a", k, c["fps"])) for k in g["kept"]]
    assert ex.frame_times == g["frame_times"] and ex.failed_saves == g["failed_saves"]
    rec = ex.records
    consulted = [(int(r["frame_count"]), float(r["diff"])) for r in rec if r["compared"]]
    assert [i for i, _ in consulted] == [i for i, _ in g["consulted"]]
    for (i, d), (_, want) in zip(consulted, g["consulted"]):
        assert abs(d - want) <= 1e-9, (i, d, want)
    # the function: the same three results
    paths, times, failed = extract_frames((R.bgr(f) for f in video), c["fps"], tmp_path / "b", check_interval=c["check_interval"])
    assert [Path(p).name for p in paths] == [Path(p).name for p in ex.frame_paths]
    assert times == g["frame_times"] and failed == g["failed_saves"]
    # the files: what save_frames writes for those frames alone; nothing else was left behind
    alone = [tmp_path / "c" / f"{k}.jpg" for k in g["kept"]]
    assert real_save([R.bgr(video[k]) for k in g["kept"]], alone) == [True] * len(alone)
    for k, got, want in zip(g["kept"], ex.frame_paths, alone):
        assert Path(got).read_bytes() == (b"there before" if k in c["existing"] else want.read_bytes()), k
    assert sorted(str(p) for p in (tmp_path / "a").rglob("*.jpg")) == sorted(ex.frame_paths)


# ---- 2: the diff's bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(48, 64), (43, 263), (7, 7), (150, 530)])
def test_diffs_are_ssim_pairs_bits_and_records_the_host_loops(dev, shape):
    """(150, 530): 3 x 4 tiles, so the order of the sum over the tile partials shows in the last bits."""
    from hippomm_amd import segmentation as seg
    h, w = shape
    n, fps = 14, 2.0                                             # every frame is a check frame, half a second apart
    gray = np.stack([R.gray_frame(720 + i // 5, i, h, w, noise=3.0, shift=1) for i in range(n)])
    frames = np.stack([R.bgr(f) for f in gray])
    records, state = seg.extraction_records(frames, range(n), fps, check_interval=1, max_diff_threshold=0.3)
    gray_dev = torch.from_numpy(gray).to(dev)
    anchor, compared = None, 0
    for i, r in enumerate(records):
        if r["compared"]:
            score = seg.ssim_pairs(gray_dev, [(i, anchor)], 255.0).cpu().numpy()[0]
            assert float(r["diff"]).hex() == float(1.0 - score).hex(), i
            compared += 1
        else:
            assert r["diff"] == 0.0
        if r["saved"]:
            anchor = i
        assert r["anchor_slot_after"] == anchor + 1 and r["has_anchor_after"] == 1
    assert compared >= 5 and 2 <= int(records["saved"].sum()) < n
    assert state.record["anchor_slot"][0] == 0 and torch.equal(state.anchor.cpu(), torch.from_numpy(gray[anchor]))
    want = model.walk(n, fps, lambda i, a: seg.compute_frame_difference(frames[i], frames[a]), check_interval=1)
    got = [(i, int(r["compared"]), int(r["saved"]), float(r["diff"]), float(r["cumulative_after"]), float(r["last_save_time_after"]))
           for i, r in enumerate(records)]
    assert [tuple(v.hex() if isinstance(v, float) else v for v in r) for r in got] == \
        [tuple(float(v).hex() if isinstance(v, float) else v for v in r) for r in want.records]


# ---- 3: batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["drift_43x263_fps30", "fail_third_write", "fail_two_in_a_row", "fail_first_two_writes"])
def test_records_and_state_do_not_depend_on_the_batch(dev, name, tmp_path, monkeypatch):
    """A failed save in the middle of a batch (frame 180 is the 7th candidate of 16) is walked again from its record; with batch 1
    it is the single-candidate route."""
    runs = {}
    for batch in (1, 2, 5, 16, 601):
        ex = _extract(name, tmp_path / str(batch), monkeypatch, batch=batch)
        runs[batch] = (_bits(ex.records), ex._state.tobytes(), ex._walker.slots[0].cpu(), [Path(p).name for p in ex.frame_paths],
                       ex.failed_saves)
        monkeypatch.undo()
    for batch, run in runs.items():
        assert run[0] == runs[1][0] and run[1] == runs[1][1] and torch.equal(run[2], runs[1][2]) and run[3:] == runs[1][3:], batch
    assert runs[1][4] == GOLDEN[name]["failed_saves"]


def test_extraction_records_carries_the_state_across_calls(dev):
    from hippomm_amd import segmentation as seg
    name = "drift_43x263_fps30"
    video = _video(name)
    counts = [i for i in range(len(video)) if i % 30 == 0]
    frames = torch.from_numpy(np.stack([video[i] for i in counts]))              # gray frames, from the host
    deny = (3, 4)
    whole, end = seg.extraction_records(frames, counts, 30.0, deny=deny)
    assert whole["saved"][3] == 0 and whole["saved"][4] == 0 and whole["compared"].sum() >= 15
    for step in (1, 4, 7):
        state, parts = None, []
        for lo in range(0, len(counts), step):
            rec, state = seg.extraction_records(frames[lo:lo + step].to(dev), counts[lo:lo + step], 30.0, state=state,
                                                deny=[d - lo for d in deny if lo <= d < lo + step])
            parts.append(rec)
        got = np.concatenate(parts)
        for f in FIELDS[1:]:
            assert got[f].tobytes() == whole[f].tobytes(), (step, f)
        assert state.record.tobytes() == end.record.tobytes() and torch.equal(state.anchor, end.anchor)
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        seg.extraction_records(np.zeros((2, 6, 64), np.uint8), [0, 30], 30.0)
    with pytest.raises(ValueError, match="same dimensions"):
        seg.extraction_records(np.zeros((2, 48, 64), np.uint8), [0, 30], 30.0, state=end)


def test_a_frame_of_another_shape_is_decided_on_the_host(dev, tmp_path):
    """The reference's SSIM raises on a shape mismatch and its MSE expression then raises too (or broadcasts): whatever
    compute_frame_difference does is what the extractor does, and frames with a side under 7 take the MSE fallback."""
    from hippomm_amd import segmentation as seg
    small = [R.bgr(R.gray_frame(730 + i, 0, 5, 9, noise=30.0)) for i in range(4)]
    ex = seg.FrameExtractor(1.0, tmp_path / "small", check_interval=1)
    for i, f in enumerate(small):
        ex.push(i, f)
    ex.flush()
    want = model.walk(4, 1.0, lambda i, a: seg.compute_frame_difference(small[i], small[a]), check_interval=1)
    assert [Path(p).name for p in ex.frame_paths] == [f"frame_{k:06d}.jpg" for k in want.kept]
    assert [float(r["diff"]) for r in ex.records if r["compared"]] == [d for _, d in want.consulted] and len(want.consulted) == 3
    # a broadcastable row against a resident anchor: the reference's MSE of the broadcast
    a, b = R.diff_fallback_case("shape_broadcast")
    ex = seg.FrameExtractor(1.0, tmp_path / "mixed", check_interval=1, max_diff_threshold=0.1)
    ex.push(0, a)
    ex.push(1, b)                                                # saved: the anchor is now 1 x 30
    ex.push(2, a)
    ex.push(3, a)                                                # and 20 x 30 again: back on the device
    ex.flush()
    d1, d2 = seg.compute_frame_difference(b, a), seg.compute_frame_difference(a, b)
    assert d1 > 0.1 and d2 > 0.1
    assert [float(r["diff"]) for r in ex.records] == [0.0, d1, d2, 0.0] and list(ex.records["compared"]) == [0, 1, 1, 1]
    assert [Path(p).name for p in ex.frame_paths] == [f"frame_{k:06d}.jpg" for k in (0, 1, 2)] and ex.failed_saves == 0


# ---- 5: the saved frames stay resident -------------------------------------------------------------------------------------------
def test_saved_frames_are_resident_for_segmentation_and_the_tower(dev, tmp_path, monkeypatch):
    from hippomm_amd import extract_frames, preprocess as pp, segmentation as seg
    from hippomm_amd.encoder import ImageBind
    rng = np.random.default_rng(5)
    scenes = [np.kron(rng.integers(0, 256, (12, 16, 3)), np.ones((20, 20, 1))).astype(np.int16) + rng.integers(-20, 21, (240, 320, 3))
              for _ in range(4)]                                 # 240 x 320, textured: every check frame differs by more than 0.8
    video = [np.clip(scenes[i // 30] + (i % 3), 0, 255).astype(np.uint8) for i in range(120)]
    cache, tower = seg.FrameCache(), pp.TowerInputCache()
    paths, times, failed = extract_frames(video, 30.0, tmp_path / "resident", cache=cache, tower_inputs=tower, batch=3)
    assert [Path(p).name for p in paths] == [f"frame_{k:06d}.jpg" for k in (0, 30, 60, 90)] and failed == 0
    plain, _, _ = extract_frames(video, 30.0, tmp_path / "plain")
    assert [Path(p).read_bytes() for p in paths] == [Path(p).read_bytes() for p in plain]
    # segment_sequence: nothing decoded, the same segments and scores as from the files
    kw = dict(max_segment_duration=3.0, min_segment_duration=1.0)
    got = seg.segment_sequence(paths, times, scorer=seg.PathScorer(cache), **kw)
    assert cache.decodes == 0 and all(cache.lookup(p) is not None for p in paths)
    fresh = seg.FrameCache()
    want = seg.segment_sequence(plain, times, scorer=seg.PathScorer(fresh), **kw)
    assert fresh.decodes > 0
    assert [(s.start_time, s.end_time, s.frame_times) for s in got] == [(s.start_time, s.end_time, s.frame_times) for s in want]
    pairs = [(k, k - 1) for k in range(1, len(paths))]
    assert [float(s).hex() for s in seg.PathScorer(cache).score([(paths[a], paths[b]) for a, b in pairs])] == \
        [float(s).hex() for s in seg.PathScorer(fresh).score([(plain[a], plain[b]) for a, b in pairs])]
    assert cache.decodes == 0
    # extract_features: every path a hit, no file read, the bits of the file route
    vspec = ib.reduced(ib.VISION_HUGE, 2)
    weights = ib.synthetic_state(vspec, seed=77, init="rich")
    want = ImageBind(state_dict=weights, towers=("vision",), depth={"vision": 2}).extract_features(
        {"vision": plain}, ["vision"])["vision"].clone()
    cached_model = ImageBind(state_dict=weights, towers=("vision",), depth={"vision": 2}, tower_inputs=tower)
    with monkeypatch.context() as m:
        m.setattr(pp, "vision_pipeline", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the pipeline ran")))
        got = cached_model.extract_features({"vision": paths}, ["vision"])["vision"]
    assert (tower.hits, tower.misses) == (4, 0) and torch.equal(got, want)
