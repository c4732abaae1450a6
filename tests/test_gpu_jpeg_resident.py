"""GPU: the decoded pixels of frames that were just encoded, made from what the encoder left on the device
(hmm_jpeg_encoded_pixels), equal Pillow's decode of Pillow's file -- and decode_jpeg of the file -- to the bit for every case of
tests/jpeg_encode_cases.py, in batches, on windows, and next to a frame that overflowed its slot; save_frames hands them to the
SSIM frame cache and to the tower input cache, after which segment_sequence and extract_features over the saved paths decode
nothing and return the same bits as from the files."""
import numpy as np
import pytest
import torch

import jpeg_encode_cases as ec
import jpeg_resident_cases as rc
from oracle import imagebind_oracle as ib

pytestmark = pytest.mark.gpu
DEPTH = 2


@pytest.fixture(scope="module")
def dev():
    from hippomm_amd import _lib
    return _lib.require_gpu()


def _case(name):
    return next(c for c in ec.cases() if c.name == name)


def test_decoded_equals_decode_jpeg_and_pillow_for_every_case(dev):
    """Every sampling, grey, BGR, qualities 1 to 100, `extreme`, and the 216 x 200 frame whose 1092 blocks cross the 32-block
    workgroup many times."""
    import hippomm_amd
    names = {c.name for c in ec.cases()}
    assert {"extreme_16x16_q100_444", "noise_216x200_q75_420", "noise_31x33_q1_420_s1", "noise_128x96_q100_444"} <= names
    for c in ec.cases():
        for source in (c.frame, torch.from_numpy(c.frame).to(dev)):
            stats = {}
            files, decoded = hippomm_amd.encode_jpeg(source, c.quality, c.subsampling, c.channel_order, stats=stats, return_decoded=True)
            assert files == [ec.expected(c)], c.name
            h, w = c.frame.shape[:2]
            assert isinstance(decoded, torch.Tensor) and decoded.shape == (1, h, w, 3) and decoded.dtype == torch.uint8 and decoded.is_cuda
            assert np.array_equal(decoded[0].cpu().numpy(), rc.pillow_decoded(c)), c.name
            assert stats == {"device": 1, "host": 0, "overflow": 0, "decoded_resident": 1}, (c.name, stats)
        assert torch.equal(decoded, hippomm_amd.decode_jpeg(files)), c.name


@pytest.mark.parametrize("batch", ec.batches(), ids=["n1", "n3"])
def test_batches_keep_their_frames_apart(dev, batch):
    import hippomm_amd
    frames = np.stack([c.frame for c in batch])
    for source in (frames, torch.from_numpy(frames).to(dev), [c.frame for c in batch]):
        stats = {}
        files, decoded = hippomm_amd.encode_jpeg(source, batch[0].quality, batch[0].subsampling, stats=stats, return_decoded=True)
        assert files == [ec.expected(c) for c in batch] and stats["decoded_resident"] == len(batch)
        assert decoded.shape == (len(batch), 33, 31, 3)
        for i, c in enumerate(batch):
            assert np.array_equal(decoded[i].cpu().numpy(), rc.pillow_decoded(c)), (i, c.name)
        assert torch.equal(decoded, hippomm_amd.decode_jpeg(files))
    window = (5, 3, 20, 27)
    _, cut = hippomm_amd.encode_jpeg(frames, batch[0].quality, batch[0].subsampling, return_decoded=True, window=window)
    for i, c in enumerate(batch):
        assert np.array_equal(cut[i].cpu().numpy(), rc.cut(rc.pillow_decoded(c), window)), (i, c.name)


def test_frames_of_different_sizes_come_back_as_a_list_in_order(dev):
    import hippomm_amd
    cases = [_case("noise_17x15_q75_420"), _case("noise_40x24_q75_420"), _case("ramp_17x15_q95_420")]
    files, decoded = hippomm_amd.encode_jpeg([c.frame for c in cases], 75, "4:2:0", return_decoded=True)
    assert isinstance(decoded, list) and [tuple(d.shape) for d in decoded] == [(15, 17, 3), (24, 40, 3), (15, 17, 3)]
    again = hippomm_amd.decode_jpeg(files)
    for d, a in zip(decoded, again):
        assert torch.equal(d, a)
    with pytest.raises(ValueError):
        hippomm_amd.encode_jpeg([c.frame for c in cases], 75, "4:2:0", return_decoded=True, window=(0, 0, 18, 15))


def _windows(w, h):
    from hippomm_amd import preprocess as pp
    out = [(0, 0, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1), (w - 1, h - 1, 1, 1),      # 1 x 1 at each corner
           (0, h - 1, w, 1), (w - 1, 0, 1, h),                                              # the last row, the last column
           (1, 1, w - 2, h - 2), (3, 5, 9, 7), (15, 7, 2, 2)]                               # odd starts: the 4:2:0 halo is read
    if (w, h) == (40, 24):
        out.append(pp.needed_window(24, 40))
    return out


@pytest.mark.parametrize("size", [(31, 33), (40, 24)], ids=["31x33", "40x24"])
def test_windows_equal_the_decoders_windows(dev, size):
    import hippomm_amd
    w, h = size
    for tag in ("420", "422", "444", "grey", "420_bgr"):
        c = _case(f"noise_{w}x{h}_q75_{tag}")
        want = rc.pillow_decoded(c)
        for window in _windows(w, h):
            files, decoded = hippomm_amd.encode_jpeg(c.frame, c.quality, c.subsampling, c.channel_order, return_decoded=True, window=window)
            assert decoded.shape == (1, window[3], window[2], 3), (c.name, window)
            assert np.array_equal(decoded[0].cpu().numpy(), rc.cut(want, window)), (c.name, window)
            assert torch.equal(decoded, hippomm_amd.decode_jpeg(files, window=window)), (c.name, window)


def test_low_level_call_on_a_shared_workspace_leaves_the_encoders_blocks_alone(dev):
    from hippomm_amd import jpeg
    batch = ec.batches()[1]
    g = jpeg.encode_geometry(33, 31, 3, "4:2:0")
    frames = torch.from_numpy(np.stack([c.frame for c in batch])).to(dev)
    ws = torch.empty(jpeg.encode_workspace_bytes(g, 3), dtype=torch.uint8, device=dev)
    out = torch.empty(3, jpeg.encode_bound(g), dtype=torch.uint8, device=dev)
    jpeg.encode_device(frames, g, 95, "RGB", out, torch.empty(3, 2, dtype=torch.int32, device=dev), ws)
    before = ws.clone()
    pixels = jpeg.encoded_pixels_device(ws, 3, g, 95, (0, 0, 31, 33), torch.empty(3, 33, 31, 3, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert torch.equal(ws, before)
    for i, c in enumerate(batch):
        assert np.array_equal(pixels[i].cpu().numpy(), rc.pillow_decoded(c)), c.name
    assert jpeg.encoded_pixels_device(ws, 0, g, 95, (0, 0, 31, 33), torch.empty(0, 33, 31, 3, dtype=torch.uint8, device=dev)).shape[0] == 0


def test_a_frame_that_overflowed_its_slot_takes_its_pixels_from_pillows_bytes(dev):
    import hippomm_amd
    batch = ec.batches()[1]
    want = [ec.expected(c) for c in batch]
    sizes = sorted(len(w) for w in want)
    stride = (sizes[1] + 15) // 16 * 16                                  # the longest file does not fit, the two others do
    assert sizes[1] <= stride < sizes[2]
    frames = np.stack([c.frame for c in batch])
    stats = {}
    files, decoded = hippomm_amd.encode_jpeg(frames, batch[0].quality, batch[0].subsampling, stats=stats, _slot_bytes=stride,
                                             return_decoded=True)
    assert files == want and stats == {"device": 2, "host": 1, "overflow": 1, "decoded_resident": 2}
    for i, c in enumerate(batch):
        assert np.array_equal(decoded[i].cpu().numpy(), rc.pillow_decoded(c)), c.name
    stats = {}
    files, decoded = hippomm_amd.encode_jpeg(frames[:1], batch[0].quality, batch[0].subsampling, stats=stats, _slot_bytes=16,
                                             return_decoded=True, window=(1, 1, 7, 9))
    assert files == want[:1] and stats["decoded_resident"] == 0
    assert np.array_equal(decoded[0].cpu().numpy(), rc.cut(rc.pillow_decoded(batch[0]), (1, 1, 7, 9)))


def test_with_a_route_off_the_pixels_are_the_existing_decode_of_the_bytes(dev, monkeypatch):
    import hippomm_amd
    from hippomm_amd import jpeg
    c = _case("noise_31x33_q75_420")
    monkeypatch.setitem(jpeg._encode_route, "on", False)                 # Pillow writes the file
    stats = {}
    files, decoded = hippomm_amd.encode_jpeg(c.frame, c.quality, c.subsampling, stats=stats, return_decoded=True)
    assert files == [ec.expected(c)] and stats["decoded_resident"] == 0 and stats["device"] == 0
    assert np.array_equal(decoded[0].cpu().numpy(), rc.pillow_decoded(c))
    monkeypatch.setitem(jpeg._encode_route, "on", True)
    monkeypatch.setitem(jpeg._route, "on", False)                        # the device decoder is off: Pillow decodes the device's file
    stats = {}
    files, decoded = hippomm_amd.encode_jpeg(c.frame, c.quality, c.subsampling, stats=stats, return_decoded=True)
    assert files == [ec.expected(c)] and stats["decoded_resident"] == 0 and stats["device"] == 1
    assert np.array_equal(decoded[0].cpu().numpy(), rc.pillow_decoded(c))


# ---- the SSIM side ----------------------------------------------------------------------------------------------------------------
def _scenes(n_scenes, per_scene, h, w, seed):
    """BGR frames: smooth scenes that differ strongly, frames of a scene = the scene plus a little sensor noise."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    frames = []
    for s in range(n_scenes):
        base = np.random.default_rng(seed * 100 + s).uniform(0, 255, (5, 6, 3)).astype(np.uint8)
        scene = np.asarray(Image.fromarray(base).resize((w, h), Image.BICUBIC)).astype(np.float32)
        for _ in range(per_scene):
            frames.append(np.clip(scene + rng.normal(0, 1, (h, w, 3)), 0, 255).astype(np.uint8))
    return frames


class _Recording:
    """A PathScorer that keeps every score the walk consulted."""
    def __init__(self, cache):
        from hippomm_amd import segmentation as seg
        self.inner, self.seen = seg.PathScorer(cache), []

    def score(self, pairs):
        for pair, s in zip(pairs, self.inner.score(pairs)):
            self.seen.append((pair, float(s).hex()))
            yield s


def test_saved_frames_are_segmented_without_a_decode_and_with_the_same_bits(dev, tmp_path):
    from hippomm_amd import jpeg, segmentation as seg
    frames = _scenes(3, 4, 48, 64, seed=7)                               # a dozen 64 x 48 frames, two scene changes
    paths = [str(tmp_path / "frames" / f"frame_{k:06d}.jpg") for k in range(len(frames))]
    times = [float(k) for k in range(len(frames))]
    cache = seg.FrameCache()
    assert seg.save_frames(frames, paths, cache=cache) == [True] * len(frames)
    assert cache.decodes == 0 and all(cache.lookup(p) is not None for p in paths)
    kw = dict(max_segment_duration=6.0, min_segment_duration=1.0)
    resident = _Recording(cache)
    got = seg.segment_sequence(paths, times, scorer=resident, **kw)
    assert cache.decodes == 0 and resident.inner.pairs_scored > 0        # nothing was decoded
    fresh_cache = seg.FrameCache()
    fresh = _Recording(fresh_cache)
    want = seg.segment_sequence(paths, times, scorer=fresh, **kw)
    assert fresh_cache.decodes > 0
    assert resident.seen == fresh.seen and len(resident.seen) > 0        # every consulted score, bit for bit
    assert len(want) >= 2 and [(s.start_time, s.end_time, s.frames, s.frame_times) for s in got] == \
        [(s.start_time, s.end_time, s.frames, s.frame_times) for s in want]
    assert any(s.end_time in (4.0, 8.0) for s in want)                   # a scene change ended a segment
    # every pair, not only the consulted ones
    pairs = [(paths[k], paths[k - 1]) for k in range(1, len(paths))]
    a = [float(s).hex() for s in seg.PathScorer(cache).score(pairs)]
    b = [float(s).hex() for s in seg.PathScorer(fresh_cache).score(pairs)]
    assert a == b and cache.decodes == 0
    # a frame whose file existed is not put; a file rewritten afterwards is a miss and is decoded from the file
    other = seg.FrameCache()
    assert seg.save_frames(frames[:2], paths[:2], cache=other) == [True, True] and other.lookup(paths[0]) is None
    with open(paths[5], "wb") as fh:
        fh.write(jpeg.pillow_encode(frames[0], 90, "4:2:0", "BGR"))
    assert cache.lookup(paths[5]) is None and cache.lookup(paths[4]) is not None
    rewritten = next(iter(seg.PathScorer(cache).score([(paths[5], paths[4])])))
    assert cache.decodes == 1
    assert float(rewritten).hex() == float(next(iter(seg.PathScorer(seg.FrameCache()).score([(paths[5], paths[4])])))).hex()
    # save_frame with the cache, a CUDA frame
    single = str(tmp_path / "frames" / "single.jpg")
    assert seg.save_frame(torch.from_numpy(frames[3]).to(dev), single, cache=cache) is True and cache.lookup(single) is not None
    assert open(single, "rb").read() == open(paths[3], "rb").read()


# ---- the tower side ---------------------------------------------------------------------------------------------------------------
def test_extract_features_from_saved_paths_hits_the_tower_input_cache_with_the_same_bits(dev, tmp_path, monkeypatch):
    from hippomm_amd import preprocess as pp, segmentation as seg
    from hippomm_amd.encoder import ImageBind
    frames = _scenes(5, 1, 240, 320, seed=11)                            # five different 320 x 240 frames
    vspec = ib.reduced(ib.VISION_HUGE, DEPTH)
    model = ImageBind(state_dict=ib.synthetic_state(vspec, seed=77, init="rich"), towers=("vision",), depth={"vision": DEPTH})
    assert model.tower_inputs is None

    def saved(folder, **caches):
        paths = [str(tmp_path / folder / f"frame_{k:06d}.jpg") for k in range(len(frames))]
        assert seg.save_frames(frames, paths, **caches) == [True] * len(frames)
        return paths

    # all hits; the cache filled from the needed window alone
    tower = pp.TowerInputCache()
    paths = saved("a", tower_inputs=tower)
    want = model.extract_features({"vision": paths}, ["vision"])["vision"].clone()       # no cache: today's pipeline
    assert len(tower) == 5 and (tower.hits, tower.misses) == (0, 0)
    cached_model = ImageBind(state_dict=ib.synthetic_state(vspec, seed=77, init="rich"), towers=("vision",), depth={"vision": DEPTH},
                             tower_inputs=tower)
    with monkeypatch.context() as m:                                                     # no file is read on this route
        m.setattr(pp, "vision_pipeline", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the pipeline ran")))
        got = cached_model.extract_features({"vision": paths}, ["vision"])["vision"]
    assert (tower.hits, tower.misses) == (5, 0)
    assert got.shape == (5, 1024) and torch.equal(got, want)
    assert torch.equal(torch.stack([tower.get(p) for p in paths]), pp.load_and_transform_vision_data_device(paths, dev))
    assert torch.equal(cached_model.extract_features({"vision": paths[2:3]}, ["vision"])["vision"],
                       model.extract_features({"vision": paths[2:3]}, ["vision"])["vision"])          # a single path

    # 2 of 5 evicted (a budget of three inputs); the cache filled next to the SSIM cache, from whole frames.  Set as an attribute.
    small, frame_cache = pp.TowerInputCache(cache_bytes=3 * pp.TOWER_INPUT_BYTES), seg.FrameCache()
    paths_b = saved("b", tower_inputs=small, cache=frame_cache)
    assert len(small) == 3 and [small.get(p) is not None for p in paths_b] == [False, False, True, True, True]
    model.tower_inputs = small
    hits, misses = small.hits, small.misses
    mixed = model.extract_features({"vision": paths_b}, ["vision"])["vision"]
    assert (small.hits - hits, small.misses - misses) == (3, 2)
    assert torch.equal(mixed, want)                                                      # the same frames, hence the same files
    # a file rewritten afterwards is a miss: its embedding is the new file's
    from hippomm_amd import jpeg
    with open(paths_b[4], "wb") as fh:
        fh.write(jpeg.pillow_encode(frames[0], 95, "4:2:0", "BGR"))
    again = model.extract_features({"vision": paths_b}, ["vision"])["vision"]
    assert torch.equal(again[:4], want[:4]) and torch.equal(again[4], want[0])
    # no hit at all: today's pipeline
    model.tower_inputs = pp.TowerInputCache()
    assert torch.equal(model.extract_features({"vision": paths}, ["vision"])["vision"], want)
