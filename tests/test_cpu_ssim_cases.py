"""CPU: the tables of tests/ssim_cases.py can fail, and reach what they say they reach.  No kernel runs.

1. Census: the literal constants are the sources'; the shapes sit on every side of the tile seams and of the finish sum's trips.
2. The reference accepts itself: numpy's own mean of the oracle's map passes the comparison on every case, and (a, a) is exactly
   1.0 in numpy on every shape, which is what lets ``self`` be compared with == and a probe's map be ones plus a patch.
3. Geometry mutants: wrong kernels applied to the oracle's S map and pushed through the same comparison; each must be rejected
   on every shape where it applies.
4. Arithmetic mutants: the map restated in another operation order.  Invisible on ``full`` (asserted, so nobody mistakes ``full``
   for an arithmetic test), rejected by the ``low`` cases with room to spare.
5. Conditions on the inputs.
"""
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import ssim_cases as C
import ssim_oracle as O

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hippomm_amd" / "csrc"
ALL_SHAPES = C.SHAPES + C.LOW_SHAPES


def _all_cases(shapes=ALL_SHAPES, contents=C.CONTENTS):
    for H, W in shapes:
        for content in contents:
            yield from C.cases(H, W, content)


# ---- 1. census ------------------------------------------------------------------------------------------------------------
def _constant(text, name):
    m = re.search(rf"constexpr int {name} = (\d+);", text)
    assert m, name
    return int(m.group(1))


def test_the_literal_constants_are_the_sources():
    core, ssim = (CSRC / "ssim_core.h").read_text(), (CSRC / "ssim.hip").read_text()
    got = (_constant(core, "kSsimTW"), _constant(core, "kSsimTH"), _constant(core, "kFinishThreads"), _constant(ssim, "kSsimChunk"),
           _constant(ssim, "kGrayThreads"), _constant(ssim, "kGrayBlocksPerFrame"))
    assert got == (C.TW, C.TH, C.FINISH, C.CHUNK, C.GRAY_THREADS, C.GRAY_BLOCKS)
    # what the tables take from the kernels besides the numbers: one thread per output column, the finish sum strided by its
    # thread count, the tile count rounded up in both directions
    assert "for (int t = threadIdx.x; t < n_tiles; t += kFinishThreads)" in core
    assert "(W - 6 + kSsimTW - 1) / kSsimTW" in core and "(H - 6 + kSsimTH - 1) / kSsimTH" in core
    assert "__launch_bounds__(kSsimTW) void ssim_tile_kernel" in ssim


def test_shapes_sit_on_every_side_of_every_seam():
    TW, TH, F = C.TW, C.TH, C.FINISH
    assert {W - 6 for _, W in C.SHAPES} >= {1, TW - 1, TW, TW + 1, 2 * TW, 2 * TW + 1}
    assert {H - 6 for H, _ in C.SHAPES} >= {1, TH - 1, TH, TH + 1, 2 * TH, 2 * TH + 1}
    counts = {s: C.n_tiles(*s) for s in C.SHAPES}
    assert set(counts.values()) >= {1, 4, 9, F, F + 1, 2 * F + 1}
    assert counts[(41, 261)] == counts[(42, 262)] == 1 and C.tiles(43, 263) == (2, 2) == C.tiles(78, 518) and C.tiles(79, 519) == (3, 3)
    assert C.tiles(7, 519) == (3, 1) and C.tiles(79, 7) == (1, 3)                # one output row / column over three tiles
    assert any(C.tiles(*s)[1] == 1 and C.tiles(*s)[0] > F for s in C.SHAPES)      # past FINISH through tiles_x alone
    assert any(C.tiles(*s)[0] > 1 and C.tiles(*s)[1] > 1 and n > F for s, n in counts.items())      # ... and with tiles_x > 1
    assert any(C.tiles(*s)[0] == 1 and n > F for s, n in counts.items())          # ... and through tiles_y alone
    assert all((H - 6) * (W - 6) <= 1024 and C.n_tiles(H, W) == 1 for H, W in C.LOW_SHAPES) and len(C.LOW_SHAPES) >= 2
    assert max(H * W for H, W in C.SHAPES) < 1.3e6                                # the largest frame: 1.2 MB


def test_probe_pixels_surround_the_first_seam():
    for H, W in C.SHAPES:
        px = C.probe_pixels(H, W)
        assert len(set(px)) == len(px) and all(0 <= x < W and 0 <= y < H for x, y in px), (H, W)
        assert {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)} <= set(px) and px[-1] == (W - 1, H - 1)
        xs = {x for x in range(C.TW - 1, C.TW + 7) if x < W}
        ys = {y for y in range(C.TH - 1, C.TH + 7) if y < H}
        if xs and ys:
            assert {(x, y) for x in xs for y in ys} <= set(px), (H, W)
        elif xs:
            assert xs <= {x for x, _ in px}, (H, W)
        elif ys:
            assert ys <= {y for _, y in px}, (H, W)
    assert len(C.probe_pixels(79, 519)) == 64 + 4 and len(C.probe_pixels(7, 7)) == 4
    # a seam pixel's windows lie in both tiles: (TW + 2, TH + 2) is held by output columns TW-4 .. TW+2 and rows TH-4 .. TH+2
    oy0, ox0, patch = C.probe_patch(79, 519, C.TW + 2, C.TH + 2, 255.0)
    assert (oy0, ox0, patch.shape) == (C.TH - 4, C.TW - 4, (7, 7)) and bool((patch != 1.0).all())


# ---- 2. the reference accepts itself ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_self_is_exactly_one_in_numpy_and_a_probe_map_is_ones_with_its_patch(shape):
    H, W = shape
    a = C.frame(H, W, "a")
    for R in (255.0, float(C.frame_range(H, W, "a"))):
        assert bool((O.ssim_map(a, a, R) == 1.0).all()), (shape, R)
    assert O.ssim(a, a) == 1.0 and O.ssim(a, a, 255.0) == 1.0
    probes = C.cases(H, W, "probe")
    for case in (probes[0], probes[len(probes) // 2], probes[-1]):
        whole = O.ssim_map(a, C.frame(H, W, case.b), 255.0)
        assert np.array_equal(whole, C.smap(case, 255.0)), case.label
        assert C.case_reference(case, 255.0) == C.reference(whole), case.label
        assert 1 <= int((whole != 1.0).sum()) <= 49, case.label


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_comparison_accepts_numpys_own_mean_on_every_case(shape):
    n = 0
    for case in _all_cases([shape]):
        for mode in C.MODES:
            S = C.smap(case, C.data_range(case, mode))
            C.check_case(float(S.mean()), case, mode)
            if case.content != "probe" and S.size <= 1 << 17:        # ssim_oracle.ssim itself, where a second map is cheap
                got = O.ssim(C.frame(*shape, case.a), C.frame(*shape, case.b), mode)
                C.check_case(got, case, mode)
                C.check(got, C.frame(*shape, case.a), C.frame(*shape, case.b), C.data_range(case, mode), case.label)
            n += 1
    assert n >= 2 * (1 + 4 + 1 + 4 + 5 + 2)


def test_the_comparison_is_the_derived_bound():
    S = np.tile([[1.0, -0.5], [0.25, 2.0 ** -30]], (16, 16))
    ref, tol = C.reference(S)
    assert ref == (0.75 + 2.0 ** -30) / 4 and tol == 1024 * 2.0 ** -53 * ((1.75 + 2.0 ** -30) / 4) + 2.0 ** -53 * ref
    C.check_map(ref + 0.99 * tol, S)
    C.check_map(ref - 0.99 * tol, S)
    with pytest.raises(AssertionError, match="x the tolerance"):
        C.check_map(ref + 1.01 * tol, S)
    with pytest.raises(AssertionError):
        C.check_map(math.nan, S)
    nan = np.array([1.0, math.nan])
    C.check_map(math.nan, nan)
    with pytest.raises(AssertionError):
        C.check_map(1.0, nan)
    ones = np.ones((64, 7))
    ref, tol = C.reference(ones)
    assert ref == 1.0 and tol == 449 * 2.0 ** -53                      # N = 448, every S = 1: 5e-14


# ---- 3. geometry mutants ----------------------------------------------------------------------------------------------------
def _mean(S, extra=0.0):
    return (math.fsum(S.ravel()) + extra) / S.size


def _zeroed(S, rows, cols):
    S = S.copy()
    S[rows, cols] = 0.0
    return _mean(S)


def _tile_block(H, W, t):
    tx, _ = C.tiles(H, W)
    return slice((t // tx) * C.TH, (t // tx + 1) * C.TH), slice((t % tx) * C.TW, (t % tx + 1) * C.TW)


def _past_the_width(c, R):
    """Sum of S at the output columns W-6 .. tiles_x TW - 1 of a kernel that reads zeros there instead of masking them."""
    H, W = c.H, c.W
    pad = C.tiles(H, W)[0] * C.TW - (W - 6)
    a, b = (np.pad(C.frame(H, W, k)[:, W - 6:], ((0, 0), (0, pad))) for k in (c.a, c.b))
    return math.fsum(O.ssim_map(a, b, R).ravel())


def _shifted(c, S, R):
    """Every window anchored one pixel to the right (the column past the frame reads as zeros)."""
    a, b = (np.pad(C.frame(c.H, c.W, k), ((0, 0), (0, 1)))[:, 1:] for k in (c.a, c.b))
    return _mean(O.ssim_map(a, b, R))


GEOMETRY_MUTANTS = {  # name -> (applies to the shape, the score the wrong kernel gives for (case, S, R))
    "output column TW-1 dropped": (lambda H, W: W - 6 >= C.TW, lambda c, S, R: _zeroed(S, slice(None), C.TW - 1)),
    "output row TH counted twice": (lambda H, W: H - 6 > C.TH, lambda c, S, R: _mean(S, math.fsum(S[C.TH]))),
    "tile partial FINISH dropped": (lambda H, W: C.n_tiles(H, W) > C.FINISH, lambda c, S, R: _zeroed(S, *_tile_block(c.H, c.W, C.FINISH))),
    "the last tile's partial dropped": (lambda H, W: True, lambda c, S, R: _zeroed(S, *_tile_block(c.H, c.W, C.n_tiles(c.H, c.W) - 1))),
    "positions past W-6 read as zeros": (lambda H, W: (W - 6) % C.TW != 0, lambda c, S, R: _mean(S, _past_the_width(c, R))),
    "the window anchored one pixel right": (lambda H, W: True, _shifted),
}
SELF_SEES = list(GEOMETRY_MUTANTS)[:4]


def _rejected(got, case, mode):
    try:
        C.check_case(got, case, mode)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_geometry_mutant_is_rejected_where_it_applies(shape):
    H, W = shape
    own, full = C.cases(H, W, "self")[0], C.cases(H, W, "full")[0]
    corner = C.cases(H, W, "probe")[0]
    assert corner.b == ("probe", 0, 0)
    applied = 0
    for name, (applies, wrong) in GEOMETRY_MUTANTS.items():
        if not applies(H, W):
            continue
        applied += 1
        for mode in C.MODES:
            R = C.data_range(full, mode)
            assert _rejected(wrong(full, C.smap(full, R), R), full, mode), f"{full.label} accepts: {name}"
            if name in SELF_SEES or name == "positions past W-6 read as zeros":
                assert _rejected(wrong(own, C.smap(own, R), R), own, mode), f"{own.label} accepts: {name}"
        if name == "the window anchored one pixel right":              # (a, a) cannot see it; the probe in the corner does
            assert not _rejected(_mean(np.ones((H - 6, W - 6))), own, 255.0)
            assert _rejected(wrong(corner, None, 255.0), corner, 255.0), f"{corner.label} accepts: {name}"
    assert applied >= 2
    if C.n_tiles(H, W) > C.FINISH:
        assert applied >= 4


def test_every_geometry_mutant_applies_somewhere():
    for name, (applies, _) in GEOMETRY_MUTANTS.items():
        assert sum(applies(H, W) for H, W in C.SHAPES) >= 3, name


# ---- 4. arithmetic mutants ----------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a b + c rounded once, elementwise."""
    if hasattr(math, "fma"):
        return np.array([math.fma(x, y, z) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())]).reshape(a.shape)
    return np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())]).reshape(a.shape)


def _restated(a, b, R, how):
    """ssim_oracle.ssim_map with one thing done another way."""
    x, y = a.astype(np.int64), b.astype(np.int64)
    sx, sy, sxx, syy, sxy = O.box7(x), O.box7(y), O.box7(x * x), O.box7(y * y), O.box7(x * y)
    if how == "reciprocal":
        r = 1 / 49.0
        ux, uy, uxx, uyy, uxy = sx * r, sy * r, sxx * r, syy * r, sxy * r
    else:
        ux, uy, uxx, uyy, uxy = sx / 49.0, sy / 49.0, sxx / 49.0, syy / 49.0, sxy / 49.0
    cov_norm = 49.0 / 48.0
    if how == "fused":
        vx, vy, vxy = cov_norm * _fma(-ux, ux, uxx), cov_norm * _fma(-uy, uy, uyy), cov_norm * _fma(-ux, uy, uxy)
    elif how == "integer variances":
        vx, vy, vxy = (49 * sxx - sx * sx) / (49.0 * 48.0), (49 * syy - sy * sy) / (49.0 * 48.0), (49 * sxy - sx * sy) / (49.0 * 48.0)
    else:
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    if how == "R from b":
        R = float(int(b.max()) - int(b.min()))
    C1, C2 = (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


ARITHMETIC_MUTANTS = ("reciprocal", "fused", "integer variances", "R from b")


def _mutant_ratio(case, how):
    H, W = case.H, case.W
    R = C.data_range(case, None)
    wrong = _restated(C.frame(H, W, case.a), C.frame(H, W, case.b), R, how)
    return C.deviation(math.fsum(wrong.ravel()) / wrong.size, C.smap(case, R))


def test_the_restatement_is_the_oracle():
    for case in _all_cases(C.LOW_SHAPES + [(43, 263)], ("full", "low", "extreme", "order")):
        R = C.data_range(case, None)
        got = _restated(C.frame(case.H, case.W, case.a), C.frame(case.H, case.W, case.b), R, None)
        assert np.array_equal(got, C.smap(case, R), equal_nan=True), case.label
    a, b, c = np.array([1.0 + 2.0 ** -30]), np.array([1.0 - 2.0 ** -30]), np.array([-1.0])
    assert _fma(a, b, c)[0] == -2.0 ** -60 and (a * b + c)[0] == 0.0


def test_full_cannot_see_the_arithmetic_mutants():
    """Uniform 0..255 frames have variances in the thousands: a reordered expression moves an S by an ulp or two, and from some
    tens of positions on that drowns in the bound of the sum.  (At (7, 7), one position, the bound is two ulps of that one S and
    even ``full`` sees them; no other shape of the table does.)"""
    worst = {}
    for how in ARITHMETIC_MUTANTS[:3]:
        shapes = [s for s in ALL_SHAPES if 64 <= (s[0] - 6) * (s[1] - 6) <= (1024 if how == "fused" else 1 << 17)]
        assert len(shapes) >= 5
        worst[how] = max(_mutant_ratio(C.cases(H, W, "full")[0], how) for H, W in shapes)
    assert all(v <= 1.0 for v in worst.values()), f"|mutant - reference| / tolerance on `full`: {worst}"


def test_low_rejects_every_arithmetic_mutant_with_room_to_spare():
    low = [c for H, W in C.LOW_SHAPES for c in C.cases(H, W, "low")]
    ratios = {how: {c.label: _mutant_ratio(c, how) for c in low} for how in ARITHMETIC_MUTANTS}
    seen = {how: {k: round(v, 1) for k, v in r.items() if v >= 8.0} for how, r in ratios.items()}
    report = "|mutant - reference| / tolerance on `low`, where >= 8: " + repr(seen)
    print(report)
    for how in ARITHMETIC_MUTANTS:
        assert len(seen[how]) >= 2, f"{how}: " + report
    # the pairs of {254, 255} alone see the first three, as overexposed shots and white slides would
    for how in ARITHMETIC_MUTANTS[:3]:
        assert sum("254_255" in k for k in seen[how]) >= 2, f"{how}: " + report


# ---- 5. conditions on the inputs ----------------------------------------------------------------------------------------------
def test_conditions_on_the_inputs():
    for case in _all_cases():
        if (case.H - 6) * (case.W - 6) > 1 << 17 and case.content in ("low", "extreme"):
            continue                                                # the frames are made the same way at every size
        for mode in C.MODES:
            if case.content != "extreme":
                assert not math.isnan(C.case_reference(case, C.data_range(case, mode))[0]), case.label
            else:
                S = C.smap(case, C.data_range(case, mode))
                assert np.isfinite(S).all() or np.isnan(S).all(), case.label       # NaN everywhere or nowhere, never inf
        if case.content == "low":
            assert C.frame_range(case.H, case.W, case.a) >= 1 and C.frame_range(case.H, case.W, case.b) >= 1, case.label
            f = C.frame(case.H, case.W, case.a)
            assert {int(f.min()), int(f.max())} <= set(sum(C.LOW_SETS.values(), ())), case.label
    for H, W in ALL_SHAPES:
        f = C.base_frames(H, W)
        assert C.frame_range(H, W, "a") == 255 and C.frame_range(H, W, "narrow") == 40
        for name, values in C.LOW_SETS.items():
            assert set(np.unique(f[f"low_{name}_a"])) == set(values) and set(np.unique(f[f"low_{name}_b"])) == set(values[:2]), (H, W, name)
        ex = {c.label.split(":")[2]: c for c in C.cases(H, W, "extreme")}
        assert math.isnan(C.reference(C.smap(ex["const,const"], 0.0))[0])                # R from a is 0: 0 / 0
        assert C.reference(C.smap(ex["const,const"], 255.0))[0] == 1.0
        if (H - 6) * (W - 6) <= 1 << 17:
            assert C.reference(C.smap(ex["checkerboard"], 255.0))[0] < -0.9              # negative S
        assert int(O.box7(f["white"][:7, :7].astype(np.int64) ** 2)[0, 0]) == 49 * 255 ** 2       # the largest box sum
        fwd, back = C.cases(H, W, "order")
        (r1, t1), (r2, t2) = (C.reference(C.smap(c, C.data_range(c, None))) for c in (fwd, back))
        assert abs(r1 - r2) > 100 * max(t1, t2), (H, W, r1, r2)


def test_walk_frames_make_several_compares_and_saves_of_both_kinds():
    """Frame 4 is saved for the cumulative difference (no single diff reaches the threshold), frames 6 and 9 for their own."""
    for H, W in C.WALK_SHAPES[:2]:
        frames = C.walk_frames(H, W)
        assert frames.shape == (10, H, W) and frames.dtype == np.uint8 and np.array_equal(frames[0], C.frame(H, W, "a"))
        assert C.walk_decisions(frames) == [(0, 1, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 1, 4), (1, 0, 4), (1, 1, 6), (1, 0, 6),
                                            (1, 0, 6), (1, 1, 9)]
        assert all(1.0 - O.ssim(frames[i], frames[0], 255.0) < 0.3 for i in range(1, 5))
    assert {C.n_tiles(*s) for s in C.WALK_SHAPES} == {1, C.FINISH + 1, C.FINISH + 2} and C.tiles(*C.WALK_SHAPES[2])[0] == 2
