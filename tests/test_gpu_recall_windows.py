"""GPU: the recall frame windows.  ``resize_frames`` (hmm_resize_linear_u8) is bit-equal to tests/resize_oracle.py at the
reference's geometries, at odd ones, at scale 1, on the 2 x 2 area path, over several frames and at the extremes of the int32
arithmetic; the call touches no byte it does not own (tests/arena.py); ``recall_window_frames`` gives the files and the kept
lists of the composed oracle route of tests/recall_window_cases.py."""
import numpy as np
import pytest
import torch

import arena as A
import recall_window_cases as rc
import resize_oracle as ro

pytestmark = pytest.mark.gpu

TARGET = (320, 180)                                                      # cv2's (width, height)
SHAPES = [((1080, 1920), TARGET), ((720, 1280), TARGET), ((1080, 1440), TARGET), ((181, 323), TARGET), ((400, 640), TARGET),
          ((360, 640), TARGET), ((180, 320), TARGET), ((14, 12), (6, 7)), ((11, 9), (5, 7))]


def _resize(frames: np.ndarray, size) -> np.ndarray:
    from hippomm_amd.resize import resize_frames
    got = resize_frames(torch.from_numpy(frames).cuda(), size)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
    return got.cpu().numpy()


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("src,size", SHAPES, ids=[f"{h}x{w}" for (h, w), _ in SHAPES])
def test_resize_is_bit_equal_to_the_oracle(src, size, channels):
    rng = np.random.default_rng(src[0] * 4099 + src[1] * 3 + channels)
    frames = rng.integers(0, 256, (2, *src, channels), dtype=np.uint8)
    got = _resize(frames, size)
    assert got.shape == (2, size[1], size[0], channels)
    assert np.array_equal(got, ro.resize(frames, size))


def test_the_area_path_is_taken_only_where_both_scales_are_two():
    """(14, 12) -> (7, 6) is the 2 x 2 mean, (11, 9) -> (7, 5) and (400, 640) -> (180, 320) are not: on a frame where the two
    rules differ, each result is its own rule's."""
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (1, 14, 12, 3), dtype=np.uint8)
    mean = ((frames[:, 0::2, 0::2].astype(int) + frames[:, 0::2, 1::2] + frames[:, 1::2, 0::2] + frames[:, 1::2, 1::2] + 2) >> 2)
    assert np.array_equal(_resize(frames, (6, 7)), mean.astype(np.uint8))
    assert ro.is_area((14, 12), (7, 6)) and not ro.is_area((11, 9), (7, 5)) and not ro.is_area((400, 640), (180, 320))


@pytest.mark.parametrize("channels", [1, 3])
def test_no_frames_and_five_distinct_frames(channels):
    from hippomm_amd.resize import resize_frames
    empty = resize_frames(torch.empty((0, 37, 53, channels), dtype=torch.uint8, device="cuda"), (17, 11))
    assert tuple(empty.shape) == (0, 11, 17, channels) and empty.is_cuda
    rng = np.random.default_rng(11 + channels)
    for src, size in (((37, 53), (17, 11)), ((22, 34), (17, 11))):       # linear, then 2 x 2 area: a wrong frame stride shows in both
        frames = rng.integers(0, 256, (5, *src, channels), dtype=np.uint8)
        want = ro.resize(frames, size)
        assert len({want[i].tobytes() for i in range(5)}) == 5
        assert np.array_equal(_resize(frames, size), want)


@pytest.mark.parametrize("src,size", [((1080, 1440), TARGET), ((400, 640), TARGET), ((180, 320), TARGET), ((11, 9), (5, 7)), ((14, 12), (6, 7))])
def test_extreme_frames_stay_inside_int32(src, size):
    """All 255, all 0 and both 0 / 255 checkerboards: the largest products of both passes (255 * 2048 * 2048 before the shifts)."""
    yy, xx = np.mgrid[0:src[0], 0:src[1]]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    planes = np.stack([np.full(src, 255, np.uint8), np.zeros(src, np.uint8), board, 255 - board])
    frames = np.repeat(planes[..., None], 3, axis=3)
    got = _resize(frames, size)
    assert np.array_equal(got, ro.resize(frames, size))
    assert (got[0] == 255).all() and (got[1] == 0).all()


def test_bad_input_is_refused_by_the_python_layer():
    from hippomm_amd.resize import resize_frames
    frames = torch.zeros((1, 90, 160, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="no larger than the source"):
        resize_frames(frames)                                            # (320, 180) would enlarge
    with pytest.raises(ValueError, match="no larger than the source"):
        resize_frames(torch.zeros((1, 360, 300, 3), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match=r"\(n, H, W, 1\) or \(n, H, W, 3\)"):
        resize_frames(torch.zeros((1, 360, 640, 2), dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        resize_frames(torch.zeros((1, 360, 640, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        resize_frames(torch.zeros((360, 640, 3), dtype=torch.uint8, device="cuda"))


# ---- the memory contract -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,size,channels", [((11, 9), (5, 7), 3), ((14, 12), (6, 7), 3), ((181, 323), TARGET, 1), ((180, 320), TARGET, 3)])
def test_guards_hold_inputs_stay_and_pixels_do_not_depend_on_the_poison(src, size, channels):
    from hippomm_amd import _lib
    from hippomm_amd.resize import RESIZE_AREA2X, resize_linear_tables, resize_mode
    dev = _lib.require_gpu()
    dw, dh = size
    n = 3
    rng = np.random.default_rng(src[0] + channels)
    frames = rng.integers(0, 256, (n, *src, channels), dtype=np.uint8)
    want = ro.resize(frames, size)
    mode = resize_mode(src, (dh, dw))
    (xofs, xcoef), (yofs, ycoef) = resize_linear_tables(src[1], dw), resize_linear_tables(src[0], dh)
    tables = {"xofs": xofs, "xcoef": xcoef, "yofs": yofs, "ycoef": ycoef}
    for pattern, word in A.PATTERNS.items():
        ar = A.GuardedArena(A.needed_bytes([frames.nbytes, want.nbytes] + [t.nbytes for t in tables.values()]), dev, word)
        v = {"src": ar.put(torch.from_numpy(frames), "src", align=16), "dst": ar.carve(want.nbytes, "dst", align=16)}
        for name, t in tables.items():
            v[name] = ar.put(torch.from_numpy(np.array(t)), name, align=16)
        for attempt in range(2):                                         # the second call finds a re-poisoned output
            ptrs = [0] * 4 if mode == RESIZE_AREA2X and attempt else [ar.address(v[k]) for k in tables]   # area: tables may be null
            st = _lib.load().hmm_resize_linear_u8(ar.address(v["src"]), n, src[0], src[1], channels, ar.address(v["dst"]), dh, dw,
                                                  *ptrs, mode, _lib.stream_ptr())
            torch.cuda.synchronize()
            assert st == 0, _lib.load().hmm_last_error()
            ar.check_guards()
            assert torch.equal(v["src"].cpu(), torch.from_numpy(frames).reshape(-1)), pattern
            for name, t in tables.items():
                assert v[name].cpu().numpy().tobytes() == np.array(t).tobytes(), (pattern, name)
            assert v["dst"].cpu().numpy().tobytes() == want.tobytes(), (pattern, attempt)
            ar.repoison(v["dst"])


def test_bad_arguments_are_refused_with_nothing_written():
    from hippomm_amd import _lib
    dev = _lib.require_gpu()
    ar = A.GuardedArena(A.needed_bytes([11 * 9 * 3, 7 * 5 * 3]), dev, A.PATTERNS["ones"])
    src, dst = ar.carve(11 * 9 * 3, "src"), ar.carve(7 * 5 * 3, "dst")
    lib = _lib.load()
    assert lib.hmm_resize_linear_u8(ar.address(src), 1, 11, 9, 3, ar.address(dst), 7, 5, None, None, None, None, 0, _lib.stream_ptr()) == -1
    assert b"resize_linear_u8" in lib.hmm_last_error()
    assert lib.hmm_resize_linear_u8(ar.address(src), 1, 11, 9, 3, ar.address(dst), 7, 5, None, None, None, None, 1, _lib.stream_ptr()) == -1
    assert lib.hmm_resize_linear_u8(ar.address(src), 1, 6, 9, 3, ar.address(dst), 7, 5, None, None, None, None, 0, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert ar.is_pattern(dst) and ar.is_pattern(src)
    ar.check_guards()


# ---- recall_window_frames ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recalled(tmp_path_factory):
    from hippomm_amd import recall_window_frames
    from hippomm_amd.frame_cache import FrameCache
    folder = tmp_path_factory.mktemp("recall")
    windows = [w for _, w in rc.windows()]
    paths = [[str(folder / f"w{k}" / f"frame_{int(t * 1000)}.jpg") for t, _ in w] for k, w in enumerate(windows)]
    cache = FrameCache()
    plain = recall_window_frames(windows)
    keyed = recall_window_frames(windows, size=rc.SIZE, similarity_cut=rc.CUT, quality=95, paths=paths, cache=cache)
    return plain, keyed, paths, cache


def test_recalled_windows_equal_the_composed_oracle_route(recalled):
    plain, keyed, paths, _ = recalled
    want = rc.expected()
    for w in want:                                                       # no decision hangs on the last digits of a score
        for i, j, s in w["consulted"]:
            assert np.isnan(s) or abs(s - rc.CUT) > rc.MARGIN, (w["name"], i, j, s)
    for got in (plain, keyed):
        assert got.kept == [w["kept"] for w in want]
        assert got.times == [w["times"] for w in want]
        assert got.files == [w["files"] for w in want]
        assert got.all_segment_times == [t for w in want for t in w["times"]]
        assert got.all_segment_files == [f for w in want for f in w["files"]]
    assert plain.all_segment_frames is None
    assert keyed.all_segment_frames == [paths[k][i] for k, w in enumerate(want) for i in w["kept"]]


def test_only_the_kept_files_are_written_and_the_cache_holds_them(recalled):
    import os
    from hippomm_amd.frame_cache import PathScorer
    import ssim_oracle as so
    _, keyed, paths, cache = recalled
    want = rc.expected()
    for k, w in enumerate(want):
        for i, path in enumerate(paths[k]):
            if i in w["kept"]:
                with open(path, "rb") as fh:
                    assert fh.read() == w["all_files"][i], (w["name"], i)
                assert cache.lookup(path) is not None, (w["name"], i)
            else:
                assert not os.path.exists(path), (w["name"], i)
    assert cache.decodes == 0
    k = [w["name"] for w in want].index("noise")                          # two kept files, scored by path: nothing is decoded
    score = next(iter(PathScorer(cache).score([(paths[k][0], paths[k][1])])))
    assert cache.decodes == 0
    grays = [rc.pillow_gray(f) for f in want[k]["all_files"][:2]]
    assert abs(score - so.ssim(grays[0], grays[1])) < 1e-9


def test_windows_of_eight_frames_are_taken():
    """The largest window the call accepts, at a small geometry: 8 frames, 28 pairs in the one SSIM launch, against the oracle."""
    from hippomm_amd import recall_window_frames
    rng = np.random.default_rng(8)
    base = [rng.integers(0, 256, (40, 64, 3), dtype=np.uint8) for _ in range(3)]
    order = [0, 0, 1, 1, 0, 2, 2, 1]
    window = [(float(t), base[b].copy()) for t, b in enumerate(order)]
    got = recall_window_frames([window], size=(32, 20))
    small = [ro.resize(f[None], (32, 20))[0] for _, f in window]
    files = [rc.pillow_file(s) for s in small]
    grays = [rc.pillow_gray(f) for f in files]
    import ssim_oracle as so
    kept, consulted = rc.reference_walk(lambda i, j: so.ssim(grays[i], grays[j]), 8)
    assert all(np.isnan(s) or abs(s - rc.CUT) > rc.MARGIN for _, _, s in consulted)
    assert kept == [0, 2, 4, 5, 7]
    assert got.kept == [kept] and got.files == [[files[i] for i in kept]] and got.all_segment_times == [float(i) for i in kept]
