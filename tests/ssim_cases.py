"""The shapes, the frames, the reference and the comparison of tests/test_gpu_ssim_edges.py, kept apart from it so that
tests/test_cpu_ssim_cases.py can run WRONG kernels through exactly the same inputs and the same comparison without a GPU.  Nothing
of hippomm_amd/ is imported here.

Shapes.  SHAPES puts (H - 6, W - 6) on every side of the seams of the 256 x 36 output tile of hippomm_amd/csrc/ssim_core.h -- one
short of it, exactly full, one past, two tiles full, one past two -- gives a single output row and a single output column spread
over several tiles, and takes the tile count to 256, 257 and 513: the finish sum (ssim_partials_sum, shared by ssim_finish_kernel
and extract_decide_kernel) strides 256 threads over a pair's tile partials, so 257 is the first count at which a thread adds a
second partial and 513 the first at which one adds a third.  LOW_SHAPES are small frames (N <= 1024 positions) for the ``low``
content alone: only there is the bound below tight enough to see the ORDER of the fp64 operations.

Contents, each a seeded function of the shape (cases(H, W, content)):
  self     (a, a): every S is exactly 1.0 in numpy and a sum of N ones is exact in any order, so the score is 1.0, bits: one
           dropped or doubled position, column, row or tile partial changes it.  [counts positions exactly, at any size]
  probe    b is a with one pixel flipped by 0x80, one case per pixel of probe_pixels(): the four corners, the last pixel, and the
           pixels around the first tile seam.  Only the <= 49 windows that hold the pixel leave 1.0.  [which positions]
  full     independent uniform 0..255 frames.  [ordinary values]
  low      frames of {254, 255}, {200, 201, 202} and {0, 1}; a holds both ends of its range.  With R from a the constants C1, C2
           are tiny, the variances are differences of nearly equal numbers and a reordered expression shows.  [arithmetic order]
  extreme  all-255 against all-0 and back (the largest box sums, 49 x 255^2), a 1-pixel checkerboard against its complement
           (S near -1), a constant frame against itself (R from a is 0: NaN, as numpy gives), a constant against a textured frame.
  order    (a, b) and (b, a) for frames of different ranges.  [R comes from the FIRST index]

Reference: the numpy-order fp64 map of tests/ssim_oracle.py, summed by math.fsum and divided by N -- the oracle's S values with an
exactly rounded mean, so it holds no summation order of its own.

Comparison, check(): NaN iff the reference is NaN; otherwise |got - ref| <= N 2^-53 mean|S| + 2^-53 |ref|, the bound on the error
of a sum of N fp64 terms in ANY order (each of the N - 1 additions is off by at most 2^-53 of a partial sum, and no partial sum
exceeds sum|S|), plus the rounding of the final division.  Derived, not measured; it assumes nothing about tiles, waves or the
finish loop.  About 6e-15 at N = 448 and 1.3e-10 at N = 1.2M.  ``self`` is compared with == against 1.0 instead.
"""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np

import ssim_oracle as O

# kSsimTW, kSsimTH, kFinishThreads (ssim_core.h); kSsimChunk, kGrayThreads, kGrayBlocksPerFrame (ssim.hip).  Literals on purpose:
# tests/test_cpu_ssim_cases.py reads the sources, so a changed tile fails the table loudly instead of silently moving the seams.
TW, TH, FINISH, CHUNK, GRAY_THREADS, GRAY_BLOCKS = 256, 36, 256, 128, 256, 512
EPS = 2.0 ** -53

SHAPES = [  # (H, W)                tiles
    (7, 7),                       # 1: one position
    (41, 261),                    # 1, one short both ways
    (42, 262),                    # 1, exactly full
    (43, 263),                    # 2 x 2 with 1-wide remainders
    (78, 518),                    # 2 x 2, all full
    (79, 519),                    # 3 x 3
    (7, 519),                     # 3 x 1, one output row
    (79, 7),                      # 1 x 3, one output column
    (9222, 7),                    # 256 = FINISH
    (9223, 7),                    # 257: a second trip of the finish sum
    (18439, 7),                   # 513: a third
    (7, 65543),                   # 257 in one tile row
    (4615, 263),                  # 2 x 129 = 258
]
LOW_SHAPES = [(13, 70), (11, 134), (22, 45)]      # N = 448, 640, 624
CONTENTS = ("self", "probe", "full", "low", "extreme", "order")
LOW_SETS = {"254_255": (254, 255), "200_202": (200, 201, 202), "0_1": (0, 1)}
MODES = (None, 255.0)                             # data_range: R of frame a, or the full scale


def tiles(H, W):
    """(tiles_x, tiles_y) of ssim_tiles."""
    return -(-(W - 6) // TW), -(-(H - 6) // TH)


def n_tiles(H, W):
    tx, ty = tiles(H, W)
    return tx * ty


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _rng(H, W, tag):
    return np.random.default_rng([H, W, tag])


def _from_set(rng, H, W, values):
    """A frame drawn from ``values`` that holds the smallest and the largest of them."""
    f = np.asarray(values, np.uint8)[rng.integers(0, len(values), (H, W))]
    f[0, 0], f[H - 1, W - 1] = min(values), max(values)
    return f


def probe_pixels(H, W):
    """(x, y): the four corners, the last pixel, and every pixel with x in TW-1 .. TW+6 and y in TH-1 .. TH+6 that the frame has;
    a frame with only one of the two seams takes its middle row or column for the other coordinate."""
    xs = [x for x in range(TW - 1, TW + 7) if x < W]
    ys = [y for y in range(TH - 1, TH + 7) if y < H]
    seam = [(x, y) for y in (ys or [H // 2]) for x in (xs or [W // 2])] if xs or ys else []
    out = []
    for p in [(0, 0), (W - 1, 0), (0, H - 1)] + seam + [(W - 1, H - 1)]:
        if p not in out:
            out.append(p)
    return out


@functools.lru_cache(maxsize=4)
def base_frames(H, W):
    """The frames every content of a shape is made of; read-only."""
    a = _rng(H, W, 1).integers(0, 256, (H, W), dtype=np.uint8)
    b = _rng(H, W, 2).integers(0, 256, (H, W), dtype=np.uint8)
    a[0, 0], a[0, W - 1] = 0, 255                                   # R of a is 255 at every size
    b[0, 0], b[0, W - 1] = 0, 255
    narrow = _rng(H, W, 3).integers(100, 141, (H, W), dtype=np.uint8)
    narrow[0, 0], narrow[H - 1, W - 1] = 100, 140                   # R of narrow is 40
    yy, xx = np.mgrid[:H, :W]
    chk = (((xx + yy) & 1) * 255).astype(np.uint8)
    f = {"a": a, "b": b, "narrow": narrow, "chk": chk, "chk_c": (255 - chk).astype(np.uint8),
         "white": np.full((H, W), 255, np.uint8), "black": np.zeros((H, W), np.uint8), "const": np.full((H, W), 77, np.uint8)}
    for i, (name, values) in enumerate(LOW_SETS.items()):
        f[f"low_{name}_a"] = _from_set(_rng(H, W, 10 + 2 * i), H, W, values)
        f[f"low_{name}_b"] = _from_set(_rng(H, W, 11 + 2 * i), H, W, values[:2])   # {200, 201}: another range than its a
    for v in f.values():
        v.setflags(write=False)
    return f


def frame(H, W, key):
    """key: a name of base_frames, or ("probe", x, y): frame a with pixel (x, y) flipped by 0x80."""
    if isinstance(key, tuple):
        _, x, y = key
        f = base_frames(H, W)["a"].copy()
        f[y, x] ^= 0x80
        return f
    return base_frames(H, W)[key]


def frame_range(H, W, key):
    f = frame(H, W, key)
    return int(f.max()) - int(f.min())


def cases(H, W, content):
    """[NS(label, content, H, W, a, b)], a and b keys of frame()."""
    def c(a, b, what):
        return NS(label=f"{H}x{W}:{content}:{what}", content=content, H=H, W=W, a=a, b=b)
    if content == "self":
        return [c("a", "a", "a,a")]
    if content == "probe":
        return [c("a", ("probe", x, y), f"x{x},y{y}") for x, y in probe_pixels(H, W)]
    if content == "full":
        return [c("a", "b", "a,b")]
    if content == "low":
        out = [c(f"low_{n}_a", f"low_{n}_b", n) for n in LOW_SETS]
        return out + [c("low_200_202_b", "low_200_202_a", "200_201,200_202")]
    if content == "extreme":
        return [c("white", "black", "255,0"), c("black", "white", "0,255"), c("chk", "chk_c", "checkerboard"),
                c("const", "const", "const,const"), c("const", "b", "const,textured")]
    if content == "order":
        return [c("a", "narrow", "wide,narrow"), c("narrow", "a", "narrow,wide")]
    raise KeyError(content)


def data_range(case, mode):
    """The R a call with data_range = mode uses for the case."""
    return float(frame_range(case.H, case.W, case.a)) if mode is None else float(mode)


# ---- the reference --------------------------------------------------------------------------------------------------------
def probe_patch(H, W, x, y, R):
    """(oy0, ox0, patch): the oracle's S at the windows that hold pixel (x, y) of the probe pair, computed on the 13 x 13 crop
    around the pixel -- the box sums are exact integers, so the crop gives the values of the whole frame."""
    oy0, oy1, ox0, ox1 = max(y - 6, 0), min(y, H - 7), max(x - 6, 0), min(x, W - 7)
    a = base_frames(H, W)["a"][oy0:oy1 + 7, ox0:ox1 + 7]
    b = a.copy()
    b[y - oy0, x - ox0] ^= 0x80
    return oy0, ox0, O.ssim_map(a, b, R)


def smap(case, R):
    """The oracle's S map of a case.  Every S of (a, a) is exactly 1.0 (tests/test_cpu_ssim_cases.py checks it on every shape), so
    the map of a probe pair is ones with the patch of the probed pixel."""
    H, W = case.H, case.W
    if case.content == "self":
        return np.ones((H - 6, W - 6))
    if case.content == "probe":
        S = np.ones((H - 6, W - 6))
        oy0, ox0, patch = probe_patch(H, W, case.b[1], case.b[2], R)
        S[oy0:oy0 + patch.shape[0], ox0:ox0 + patch.shape[1]] = patch
        return S
    return _pair_map(H, W, case.a, case.b, float(R))


@functools.lru_cache(maxsize=16)
def _pair_map(H, W, a, b, R):
    S = O.ssim_map(frame(H, W, a), frame(H, W, b), R)
    S.setflags(write=False)
    return S


def reference(S):
    """(ref, tolerance) of an S map: the exactly rounded mean, and N 2^-53 mean|S| + 2^-53 |ref|."""
    flat = np.asarray(S, np.float64).ravel()
    if not np.isfinite(flat).all():
        return math.nan, math.nan
    n = flat.size
    ref = math.fsum(flat) / n
    return ref, n * EPS * (math.fsum(np.abs(flat)) / n) + EPS * abs(ref)


def case_reference(case, R):
    """reference(smap(case, R)), without the map where the map is ones: the sum of N - k ones is the integer."""
    n = (case.H - 6) * (case.W - 6)
    if case.content == "self":
        return 1.0, n * EPS + EPS
    if case.content == "probe":
        patch = probe_patch(case.H, case.W, case.b[1], case.b[2], R)[2].ravel()
        assert np.isfinite(patch).all()
        ref = math.fsum(list(patch) + [float(n - patch.size)]) / n
        return ref, n * EPS * (math.fsum(list(np.abs(patch)) + [float(n - patch.size)]) / n) + EPS * abs(ref)
    return reference(smap(case, R))


def _ratio(got, ref, tol):
    """|got - ref| / tolerance; 0 where both are NaN, inf where one is."""
    got = float(got)
    if math.isnan(ref) or math.isnan(got):
        return 0.0 if math.isnan(ref) and math.isnan(got) else math.inf
    err = abs(got - ref)
    return err / tol if tol > 0 else (0.0 if err == 0 else math.inf)


def deviation(got, S):
    return _ratio(got, *reference(S))


def _check(got, ref, tol, label):
    got = float(got)
    if math.isnan(ref) or math.isnan(got):
        assert math.isnan(ref) and math.isnan(got), f"{label}: got {got!r}, reference {ref!r}"
        return
    assert abs(got - ref) <= tol, (f"{label}: got {got!r}, reference {ref!r}: off by {abs(got - ref):.3e} = "
                                   f"{_ratio(got, ref, tol):.3g} x the tolerance {tol:.3e}")


def check_map(got, S, label=""):
    _check(got, *reference(S), label)


def check(got, a, b, R, label=""):
    """The score ``got`` of the pair of uint8 frames (a, b) at data range R against the oracle."""
    check_map(got, O.ssim_map(a, b, R), label)


def check_case(got, case, mode):
    """check() for a case of the tables; ``self`` must be 1.0 exactly."""
    label = f"{case.label}:R={'a' if mode is None else mode}"
    if case.content == "self":
        assert float(got) == 1.0, (f"{label}: {float(got)!r} ({float(got).hex()}), 1.0 wanted: "
                                   f"{(float(got) - 1.0) * (case.H - 6) * (case.W - 6):+.6g} positions")
        return
    _check(got, *case_reference(case, data_range(case, mode)), label)


# ---- frames for the extraction walk -----------------------------------------------------------------------------------------
WALK_SHAPES = [(42, 262), (9223, 7), (4615, 263)]                   # one full tile; 257 tiles in a column; 258 tiles, two columns
WALK_NOISE = (0.0, 0.05, 0.10, 0.12, 0.14, 0.16, 0.60, 0.62, 0.58, 0.90)


def walk_frames(H, W):
    """Ten gray frames: frame a with the share WALK_NOISE[i] of its pixels -- always the same pixels first -- replaced by noise, so
    1 - SSIM of two frames grows with the difference of their shares.  At threshold 0.3 a walk that checks every frame saves
    frame 0, then one frame for the cumulative difference, then others for a single difference (walk_decisions())."""
    a = base_frames(H, W)["a"]
    rng = _rng(H, W, 100)
    u, noise = rng.random((H, W)), rng.integers(0, 256, (H, W), dtype=np.uint8)
    return np.stack([np.where(u < p, noise, a) for p in WALK_NOISE])


def walk_decisions(frames, threshold=0.3):
    """[(compared, saved, anchor after)] of the reference's loop with every frame a check frame, scored by the oracle."""
    out, anchor, cum = [(0, 1, 0)], 0, 0.0
    for i in range(1, len(frames)):
        d = 1.0 - O.ssim(frames[i], frames[anchor], 255.0)
        cum += d
        saved = d > threshold or cum > threshold
        if saved:
            anchor, cum = i, 0.0
        out.append((1, int(saved), anchor))
    return out
