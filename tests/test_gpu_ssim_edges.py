"""GPU: hmm_ssim_pairs, the walk's use of the same tile body and finish sum (hmm_extract_walk), and hmm_gray_u8 at every tile seam, at
every trip count of the finish sum, on frames of a low range and at the edges of the gray kernels, against the numpy oracle under
the derived bound of tests/ssim_cases.py, where the shapes, the frames, the reference and the comparison live;
tests/test_cpu_ssim_cases.py proves without a GPU that the same comparison on the same inputs rejects a subtly wrong kernel.

tests/test_gpu_segmentation.py keeps the goldens made by skimage itself and its 1e-9; this module runs the shapes at which the code
takes another path, with a tolerance that sees the order of the fp64 operations."""
import numpy as np
import pytest
import torch

import ssim_cases as C
import ssim_oracle as O

pytestmark = pytest.mark.gpu

POISON = 0xA5


def _seg():
    from hippomm_amd import segmentation as seg
    return seg


def _lib():
    from hippomm_amd import _lib as L
    return L, L.load()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.int64)


def _alone(gray, ia, ib, mode):
    """The pair scored alone, from a buffer that holds nothing but its frames."""
    seg = _seg()
    if ia == ib:
        return seg.ssim_pairs(gray[[ia]], [(0, 0)], mode).cpu().numpy()[0]
    return seg.ssim_pairs(gray[[ia, ib]], [(0, 1)], mode).cpu().numpy()[0]


# ---- every shape x every content ------------------------------------------------------------------------------------------------
TABLE = [(s, content) for s in C.SHAPES + C.LOW_SHAPES for content in C.CONTENTS]


@pytest.mark.parametrize("shape,content", TABLE, ids=[f"{s[0]}x{s[1]}-{c}" for s, c in TABLE])
def test_shape_and_content(shape, content):
    """Both R modes; ``self`` is 1.0 exactly, everything else within the bound of a sum of N terms in any order; and a score from
    the batched call has the bits of its pair scored alone."""
    seg = _seg()
    H, W = shape
    cases = C.cases(H, W, content)
    keys = []
    for c in cases:
        keys += [k for k in (c.a, c.b) if k not in keys]
    gray = torch.from_numpy(np.stack([C.frame(H, W, k) for k in keys])).cuda()
    pairs = [(keys.index(c.a), keys.index(c.b)) for c in cases]
    for mode in C.MODES:
        batched = seg.ssim_pairs(gray, pairs, mode).cpu().numpy()
        assert batched.shape == (len(cases),) and batched.dtype == np.float64
        for c, (ia, ib), got in zip(cases, pairs, batched):
            C.check_case(got, c, mode)
            alone = _alone(gray, ia, ib, mode)
            assert _bits(got) == _bits(alone), f"{c.label}, R={mode}: {float(got).hex()} in the batch, {float(alone).hex()} alone"


# ---- pair plumbing ------------------------------------------------------------------------------------------------------------
PLUMBING_SHAPE = (43, 263)                                          # 2 x 2 tiles: a pair's partials are four doubles of the workspace
PLUMBING_KEYS = ("a", "b", "narrow", "low_254_255_a", "low_200_202_a", "chk", "const")


def _pair_list(n_pairs, n_frames):
    head = [(0, 1), (1, 0), (2, 2), (n_frames - 1, 0), (0, 1), (3, n_frames - 1), (4, 3), (3, 4), (0, 1)]
    rng = np.random.default_rng(n_pairs)
    return (head + [tuple(int(v) for v in rng.integers(0, n_frames, 2)) for _ in range(n_pairs)])[:n_pairs]


@pytest.fixture(scope="module")
def plumbing():
    """The frames on the device, their (min, max), and every pair's score alone in both R modes."""
    seg = _seg()
    H, W = PLUMBING_SHAPE
    frames = np.stack([C.frame(H, W, k) for k in PLUMBING_KEYS])
    assert len({int(f.max()) - int(f.min()) for f in frames}) >= 5              # frames of different ranges in one buffer
    gray = torch.from_numpy(frames).cuda()
    n = len(frames)
    alone = {mode: {(i, j): _alone(gray, i, j, mode) for i in range(n) for j in range(n)} for mode in C.MODES}
    for (i, j), got in alone[255.0].items():
        C.check(got, frames[i], frames[j], 255.0, f"plumbing ({i}, {j})")
    for (i, j), got in alone[None].items():
        C.check(got, frames[i], frames[j], float(int(frames[i].max()) - int(frames[i].min())), f"plumbing ({i}, {j}), R from a")
    return frames, gray, alone


@pytest.mark.parametrize("n_pairs", [1, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1, 2 * C.CHUNK + 1])
def test_pairs_across_the_launch_chunks_in_a_workspace_of_exactly_the_stated_size(plumbing, n_pairs):
    """The library entry itself: the workspace is hmm_ssim_pairs_workspace_bytes and not a byte more, and the bytes behind it and
    behind the scores keep their poison.  Repeated pairs, (i, i), a pair on the last frame, (i, j) next to (j, i)."""
    L, lib = _lib()
    frames, gray, alone = plumbing
    n, (H, W) = len(frames), PLUMBING_SHAPE
    pairs = _pair_list(n_pairs, n)
    if n_pairs >= 9:
        assert pairs.count((0, 1)) >= 3 and (2, 2) in pairs and (n - 1, 0) in pairs and pairs.index((3, 4)) == pairs.index((4, 3)) + 1
    host = np.ascontiguousarray(pairs, dtype=np.int32)
    need = lib.hmm_ssim_pairs_workspace_bytes(H, W, n_pairs)
    assert need >= n_pairs * C.n_tiles(H, W) * 8 and need % 256 == 0
    minmax = torch.full((n + 1, 2), -77, dtype=torch.int32, device="cuda")
    L.check(lib.hmm_gray_u8(gray.data_ptr(), n, H, W, 2, None, minmax.data_ptr(), L.stream_ptr()), "hmm_gray_u8")
    for mode in C.MODES:
        ws = torch.full((need + 4096,), POISON, dtype=torch.uint8, device="cuda")
        out = torch.full((n_pairs + 8,), -7.0e33, dtype=torch.float64, device="cuda")
        L.check(lib.hmm_ssim_pairs(gray.data_ptr(), n, H, W, host.ctypes.data, n_pairs, -1.0 if mode is None else mode,
                                   minmax.data_ptr() if mode is None else None, out.data_ptr(), ws.data_ptr(), need, L.stream_ptr()),
                "hmm_ssim_pairs")
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert bool((ws[need:] == POISON).all()), f"n_pairs={n_pairs}, R={mode}: bytes behind the workspace were written"
        assert bool((got[n_pairs:] == -7.0e33).all()), f"n_pairs={n_pairs}, R={mode}: scores behind the last pair were written"
        want = np.array([alone[mode][p] for p in pairs])
        wrong = np.flatnonzero(_bits(got[:n_pairs]) != _bits(want))
        assert wrong.size == 0, f"n_pairs={n_pairs}, R={mode}: pairs {[(int(k), pairs[k]) for k in wrong[:8]]} differ from their scores alone"
        # a workspace one byte short is refused before any launch
        assert lib.hmm_ssim_pairs(gray.data_ptr(), n, H, W, host.ctypes.data, n_pairs, 255.0, None, out.data_ptr(), ws.data_ptr(),
                                  need - 1, L.stream_ptr()) != 0
    assert minmax[n:].cpu().tolist() == [[-77, -77]]
    assert minmax[:n].cpu().tolist() == [[int(f.min()), int(f.max())] for f in frames]


# ---- the walk -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.WALK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_walk_diffs_are_the_bits_of_ssim_pairs(shape):
    """extract_tile_kernel and extract_decide_kernel share the tile body and the finish sum with hmm_ssim_pairs: on one full tile,
    on 257 tiles in a column and on 2 x 129 tiles every compared diff is 1 - ssim_pairs(frame, anchor), bits."""
    seg = _seg()
    H, W = shape
    gray = C.walk_frames(H, W)
    n = len(gray)
    records, state = seg.extraction_records(gray, range(n), 1.0, check_interval=1, max_diff_threshold=0.3)
    gray_dev = torch.from_numpy(gray).cuda()
    anchor, decisions = None, []
    for i, r in enumerate(records):
        if r["compared"]:
            score = seg.ssim_pairs(gray_dev, [(i, anchor)], 255.0).cpu().numpy()[0]
            assert float(r["diff"]).hex() == float(1.0 - score).hex(), i
            C.check(score, gray[i], gray[anchor], 255.0, f"{H}x{W}: frame {i} against anchor {anchor}")
        else:
            assert r["diff"] == 0.0
        if r["saved"]:
            anchor = i
        decisions.append((int(r["compared"]), int(r["saved"]), anchor))
        assert r["anchor_slot_after"] == anchor + 1 and r["has_anchor_after"] == 1
    # frame 0 without a comparison, frame 4 for the cumulative difference, frames 6 and 9 for their own (ssim_cases.walk_decisions)
    assert decisions == [(0, 1, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 1, 4), (1, 0, 4), (1, 1, 6), (1, 0, 6), (1, 0, 6), (1, 1, 9)]
    assert torch.equal(state.anchor.cpu(), torch.from_numpy(gray[9]))


@pytest.mark.parametrize("shape", C.WALK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_walk_over_identical_frames_saves_the_first_alone(shape):
    seg = _seg()
    H, W = shape
    gray = np.stack([C.frame(H, W, "a")] * 5)
    records, state = seg.extraction_records(gray, range(5), 1.0, check_interval=1, max_diff_threshold=0.3)
    assert records["compared"].tolist() == [0, 1, 1, 1, 1] and records["saved"].tolist() == [1, 0, 0, 0, 0]
    assert [float(d).hex() for d in records["diff"]] == [(0.0).hex()] * 5
    assert [float(d).hex() for d in records["cumulative_after"]] == [(0.0).hex()] * 5
    assert torch.equal(state.anchor.cpu(), torch.from_numpy(gray[0]))


# ---- hmm_gray_u8 ------------------------------------------------------------------------------------------------------------------
TRIP = C.GRAY_THREADS * C.GRAY_BLOCKS                               # pixels of one trip of the grid-stride loop: 131072
GRAY_SIZES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 256), (1, 257), (1, TRIP - 1), (1, TRIP), (3, 43691), (1, 2 * TRIP + 1)]
GRAY_RANGES = [(10, 250), (60, 61), (0, 131)]                       # (min, max) of the three frames


def _min_at(hw):
    return hw - 2 if hw == TRIP + 1 else hw - 1


def _gray_targets(hw):
    """(3, hw) gray values: the minimum at each frame's last pixel, the maximum at pixel TRIP -- the first of the second trip of the
    grid-stride loop -- where the frame has one, else at its first pixel; a frame of one pixel holds its minimum alone.  At
    hw = TRIP + 1 the last pixel IS pixel TRIP, the only one of the second trip: it takes the maximum, the pixel before it --
    the last of the first trip -- the minimum."""
    out = np.empty((3, hw), np.uint8)
    for f, (lo, hi) in enumerate(GRAY_RANGES):
        g = np.random.default_rng([hw, f]).integers(lo + 1, hi, hw, dtype=np.uint8) if hi - lo > 1 else np.full(hw, lo, np.uint8)
        g[TRIP if hw > TRIP else 0] = hi
        g[_min_at(hw)] = lo
        out[f] = g
    return out


def _colours(gray, seed):
    """(..., 3) B,G,R whose BGR2GRAY is near ``gray`` and inside the frame's range: the pixels that carry the minimum and the
    maximum are neutral (the gray of (v, v, v) is v), the others differ per channel by +-1 where that stays inside 1 .. 254."""
    rng = np.random.default_rng(seed)
    bgr = np.repeat(gray[..., None].astype(np.int16), 3, -1)
    lo, hi = gray.min(-1, keepdims=True)[..., None], gray.max(-1, keepdims=True)[..., None]
    free = (bgr > lo + 1) & (bgr < hi - 1)
    bgr = bgr + np.where(free, rng.integers(-1, 2, bgr.shape), 0)
    return bgr.astype(np.uint8)


@pytest.mark.parametrize("size", GRAY_SIZES, ids=lambda s: f"{s[0] * s[1]}px")
def test_gray_and_minmax_at_the_edges_of_the_grid_stride_loop(size):
    L, lib = _lib()
    H, W = size
    hw, n = H * W, 3
    assert hw in (1, 63, 64, 65, 255, 256, 257, TRIP - 1, TRIP, TRIP + 1, 2 * TRIP + 1)
    target = _gray_targets(hw)
    bgr = _colours(target, hw)
    want = O.gray_from_bgr(bgr)
    want_minmax = [[int(g.min()), int(g.max())] for g in want]
    assert want_minmax == [[lo, hi] if hw > 1 else [lo, lo] for lo, hi in GRAY_RANGES]
    assert all(int(g[_min_at(hw)]) == lo and int(np.argmax(g)) == (TRIP if hw > TRIP else 0) for g, (lo, hi) in zip(want, GRAY_RANGES))
    for order, frames in ((1, bgr), (0, bgr[..., ::-1]), (2, want)):
        src = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        out = torch.full((n * hw + 256,), POISON, dtype=torch.uint8, device="cuda")
        minmax = torch.full((n + 1, 2), -77, dtype=torch.int32, device="cuda")
        L.check(lib.hmm_gray_u8(src.data_ptr(), n, H, W, order, None if order == 2 else out.data_ptr(), minmax.data_ptr(),
                                L.stream_ptr()), "hmm_gray_u8")
        torch.cuda.synchronize()
        assert minmax[:n].cpu().tolist() == want_minmax, (order, hw)
        assert minmax[n:].cpu().tolist() == [[-77, -77]], (order, hw)
        got = out.cpu().numpy()
        if order == 2:
            assert bool((got == POISON).all())
        else:
            assert np.array_equal(got[:n * hw].reshape(n, hw), want), (order, hw)
            assert bool((got[n * hw:] == POISON).all()), (order, hw)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_minmax_of_many_frames_and_the_range_read_behind_frame_255(n):
    """gray_minmax_init_kernel runs 256 frames per workgroup; R of frame a is read from minmax[a]."""
    seg = _seg()
    L, lib = _lib()
    frames = np.empty((n, 7, 7), np.uint8)
    for f in range(n):
        lo, hi = f % 100, f % 100 + 1 + f % 150
        frames[f] = np.random.default_rng([n, f]).integers(lo, hi + 1, (7, 7), dtype=np.uint8)
        frames[f, 0, 0], frames[f, 6, 6] = hi, lo
    gray = torch.from_numpy(frames).cuda()
    minmax = torch.full((n + 1, 2), -77, dtype=torch.int32, device="cuda")
    L.check(lib.hmm_gray_u8(gray.data_ptr(), n, 7, 7, 2, None, minmax.data_ptr(), L.stream_ptr()), "hmm_gray_u8")
    assert minmax[:n].cpu().tolist() == [[f % 100, f % 100 + 1 + f % 150] for f in range(n)]
    assert minmax[n:].cpu().tolist() == [[-77, -77]]
    firsts = [a for a in (254, 255, 256) if a < n]
    pairs = [(a, b) for a in firsts for b in (0, 100, n - 1)] + [(0, n - 1)]
    got = seg.ssim_pairs(gray, pairs, None).cpu().numpy()
    assert any(a == n - 1 for a, _ in pairs) and len({int(frames[a].max()) - int(frames[a].min()) for a, _ in pairs}) == len(firsts) + 1
    for (a, b), s in zip(pairs, got):
        C.check(s, frames[a], frames[b], float(int(frames[a].max()) - int(frames[a].min())), f"n={n}, pair ({a}, {b})")
