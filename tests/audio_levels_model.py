"""A numpy model of window_sums_kernel (hippomm_amd/csrc/audio_track.hip), step by step in the kernel's own order, for the tests only.

sum_squares(x)      the sum of squares of a contiguous 1-D window in its dtype T (float32 or float64) as the kernel forms it:
                    chunks of 8192 squares added left to right; per chunk the split tree expanded level by level into a heap
                    (node i, children 2 i and 2 i + 1; a node of more than 128 elements splits at (m / 2) - (m / 2) % 8); a leaf on
                    eight lanes -- lane j accumulates the squares of elements 8 i + j in order, the lanes are combined by a
                    butterfly over XOR 1, 2, 4 and lane 0 is read, then the m % 8 tail elements are added one by one (a leaf under
                    8 elements is all tail, from 0); inner nodes bottom-up, left + right.
mean_square(x)      T(sum / n) with n as numpy counts it: np.mean(np.square(x)) bit for bit (tests/test_cpu_audio_levels_model.py).

The keyword arguments switch in the WRONG variants the tests must be able to tell from numpy:
    chunk=None            no 8192-element chunking (one tree over the whole window)
    fused=True            the square folded into the add as one fused multiply-add (what contraction would make of r + x * x)
    leaf="running"        a leaf summed left to right instead of over eight accumulators
    split_multiple=1      the split point not rounded down to a multiple of 8
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

CHUNK = 8192
LEAF = 128
DEPTH = 7
_XOR = [np.arange(8) ^ k for k in (1, 2, 4)]


def _fma(a, b, c):
    """round(a * b + c) in the dtype of a: exact rational arithmetic, rounded once to float64 (int / int division is correctly
    rounded) and, for float32, once more -- which cannot be told from a single rounding except in rare double-rounding cases; good
    enough for a variant that only has to be told apart from the unfused sum."""
    T = type(a)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return T(exact.numerator / exact.denominator)


def expand(m: int, depth: int = DEPTH, split_multiple: int = 8):
    """The heap of one chunk of m elements: (offsets, lengths), 2 ** (depth + 1) entries, entry 0 unused, length 0 = no node."""
    size = 2 << depth
    off, length = [0] * size, [0] * size
    length[1] = m
    for d in range(depth):
        for i in range(1 << d, 2 << d):
            if length[i] > LEAF:
                half = length[i] >> 1
                left = half - half % split_multiple
                off[2 * i], length[2 * i] = off[i], left
                off[2 * i + 1], length[2 * i + 1] = off[i] + left, length[i] - left
    return off, length


def leaf_sum(s: np.ndarray, fused: bool = False, leaf: str = "eight"):
    """s: the leaf's samples (<= 128, or any length for the variants) -> the sum of their squares, a scalar of s.dtype."""
    T = s.dtype.type
    n = s.shape[0]
    if fused or leaf == "running":
        rows = 0 if leaf == "running" else n >> 3

        def add_square(r, x):
            return _fma(x, x, r) if fused else r + x * x
        lanes = []
        for j in range(8 if rows else 0):
            r = _fma(s[j], s[j], T(0)) if fused else s[j] * s[j]
            for i in range(1, rows):
                r = add_square(r, s[8 * i + j])
            lanes.append(r)
        r = ((lanes[0] + lanes[1]) + (lanes[2] + lanes[3])) + ((lanes[4] + lanes[5]) + (lanes[6] + lanes[7])) if rows else T(0)
        for i in range(rows * 8, n):
            r = add_square(r, s[i])
        return r
    rows = n >> 3
    sq = s * s                                                     # each square rounded to T on its own
    lanes = np.zeros(8, dtype=s.dtype)                             # a lane without a row holds 0 * 0
    if rows:
        body = sq[:8 * rows].reshape(rows, 8)
        lanes = body[0].copy()
        for i in range(1, rows):
            lanes = lanes + body[i]
    for perm in _XOR:                                              # the butterfly: every lane ends with the same bits
        lanes = lanes + lanes[perm]
    r = lanes[0]
    for i in range(rows * 8, n):
        r = r + sq[i]
    return r


def chunk_sum(s: np.ndarray, fused: bool = False, leaf: str = "eight", split_multiple: int = 8):
    m = s.shape[0]
    depth = DEPTH
    while (LEAF << depth) < 2 * m:                                 # only the unchunked variant needs a deeper heap than the kernel's
        depth += 1
    off, length = expand(m, depth, split_multiple)
    val = [None] * len(off)
    for i in range(1, len(off)):
        if 0 < length[i] <= LEAF:
            val[i] = leaf_sum(s[off[i]:off[i] + length[i]], fused, leaf)
    for d in range(depth - 1, -1, -1):
        for i in range(1 << d, 2 << d):
            if length[i] > LEAF:
                val[i] = val[2 * i] + val[2 * i + 1]
    return val[1]


def sum_squares(x: np.ndarray, chunk=CHUNK, fused: bool = False, leaf: str = "eight", split_multiple: int = 8):
    x = np.ascontiguousarray(x)
    assert x.ndim == 1 and x.dtype in (np.float32, np.float64)
    n = x.shape[0]
    total = x.dtype.type(0)
    step = chunk if chunk else max(n, 1)
    with np.errstate(all="ignore"):
        for c0 in range(0, n, step):
            total = total + chunk_sum(x[c0:c0 + step], fused, leaf, split_multiple)
    return total


def mean_square(x: np.ndarray, **variant):
    s = sum_squares(x, **variant)
    with np.errstate(all="ignore"):
        return s.dtype.type(s / np.intp(x.shape[0]))
