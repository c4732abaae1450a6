"""The inputs, the exact reference, the tables and the comparison of tests/test_gpu_gemm_edges.py, kept apart from it so that
tests/test_cpu_gemm_cases.py can run WRONG references through exactly the same inputs and the same comparison without a GPU.
From hippomm_amd/ this module uses one thing: the host-only plan entry hmm_op_gemm_plan, which answers what a call would launch.

Exact operands.  A and W are seeded integers in [-3, 3], the bias integers in [-64, 64], the residual integers in [-1000, 1000]:
|sum| <= 9 K <= 46 080 at K = 5120, everything stays far below 2^24, so every fp32 partial sum of every kernel is exact, the result
does not depend on the order of summation and equals the float64 (= integer) product.  HMM_EPI_F32 and HMM_EPI_BIAS_RESID_F32
must give that number bit for bit, HMM_EPI_BIAS_BF16 that number rounded to the nearest bf16, ties to even.  No tolerance, no
reference kernel.  What exact integers can NOT see is the order of (accumulator + bias) + residual: every order gives the same
bits here.  That order stays pinned by the bitwise tests of tests/test_gpu_ops.py on random normal data.

HMM_EPI_BIAS_GELU_BF16 is compared with float64 0.5 x (1 + erf(x / sqrt 2)) under gelu_tolerance().

Tables.  ``geometry``: every named geometry at the ends of its K pipeline and at ragged M.  ``splitk``: every ring geometry at
every split count over slabs of 1 .. 5 K-tiles.  ``route``: one shape on each side of every change of plan that the dispatcher
makes along M, found by scanning the plan entry (search_routes(); ``python tests/gemm_cases.py`` prints the table).  ``gelu``:
the activation alone, A = 0 and the bias carrying the sweep.
"""
import ctypes
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

F64 = torch.float64
EPI_BIAS_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_RESID_F32, EPI_F32 = 0, 1, 2, 3
EPIS = (EPI_BIAS_BF16, EPI_BIAS_GELU_BF16, EPI_BIAS_RESID_F32, EPI_F32)
AUTO, AUTO_TILED = -1, -2
PP, PP_PEELED, SLIVER = 3, 4, 5
FLAG_PP_TAIL, FLAG_SLIVER_PEEL = 1, 2
CANARY_F32 = -7.0e33                    # what the rows behind an fp32 output hold; bf16 outputs hold NaN there
GUARD_ROWS = 2

# launch_tile's table (gemm_bf16.hip), mirrored: id -> (BM, BN, STAGES, KSUB).  STAGES 2 is the double buffer.  The ping-pong
# kernel (3) walks K in steps of 128, the sliver kernel (5) has its own table below, and 4 (ping-pong with peeled tails) is a route
# through these kernels, not one of them: it is in the route table by name.
GEOMETRY = {0: (128, 128, 2, 1), 1: (256, 128, 2, 1), 2: (256, 256, 2, 1), 3: (256, 256, 0, 2),
            6: (128, 128, 4, 1), 7: (64, 64, 4, 1), 8: (32, 32, 4, 1), 9: (32, 32, 4, 2), 10: (32, 32, 4, 4), 11: (64, 64, 3, 2),
            12: (128, 64, 4, 1), 13: (64, 128, 4, 1), 14: (128, 128, 4, 1), 15: (128, 64, 4, 1), 16: (64, 128, 4, 1)}
SLIVER_DEPTH = {1: 8, 2: 6, 4: 4}       # rows-per-wave class (16-row blocks) -> K steps in flight (launch_gemm_sliver)
RING_IDS = tuple(range(6, 17))
ALL_IDS = tuple(range(17))


# ---- the plan entry -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan_fn():
    from hippomm_amd import _lib as L
    return L.load()


_PLAN_BUF = (ctypes.c_int32 * 48)()


def plan_raw(M, N, K, epi=EPI_F32, tile=AUTO, small_tiles=128, splits=0):
    """(status, records): records as tuples (geometry, row0, rows, splits, sliver class, flags), or the error text."""
    lib = _plan_fn()
    n = lib.hmm_op_gemm_plan(M, N, K, epi, tile, small_tiles, splits, ctypes.addressof(_PLAN_BUF), 8)
    if n < 0:
        return n, lib.hmm_last_error().decode()
    return n, tuple(tuple(_PLAN_BUF[6 * i:6 * i + 6]) for i in range(n))


def plan(M, N, K, epi=EPI_F32, tile=AUTO, small_tiles=128, splits=0):
    n, recs = plan_raw(M, N, K, epi, tile, small_tiles, splits)
    assert n >= 1, (M, N, K, epi, tile, small_tiles, splits, recs)
    return recs


def signature(recs):
    """What a plan is, apart from the shape: per launch (geometry, sliver class, flags); a ping-pong tail also tells the number
    of 256-row tiles that were peeled."""
    return tuple((g, mt, fl) + ((-(-rows // 256),) if fl & FLAG_PP_TAIL else ()) for g, _, rows, _, mt, fl in recs)


# ---- exact operands -------------------------------------------------------------------------------------------------------
_POOL_M, _POOL_N, _POOL_K = 4200, 5120, 5120


@functools.lru_cache(maxsize=None)
def _pools():
    g = torch.Generator().manual_seed(20261019)
    a = torch.randint(-3, 4, (_POOL_M, _POOL_K), generator=g, dtype=torch.int8)
    w = torch.randint(-3, 4, (_POOL_N, _POOL_K), generator=g, dtype=torch.int8)
    bias = torch.randint(-64, 65, (_POOL_N,), generator=g, dtype=torch.int32)
    return a, w, bias


def operands(M, N, K):
    """A [M][K], W [N][K] (bf16, exact small integers) and the bias (fp32).  Slices of one seeded pool: every case of one (N, K)
    shares W, and a case of fewer rows is a prefix of a case of more."""
    a, w, bias = _pools()
    assert M <= _POOL_M and N <= _POOL_N and K <= _POOL_K, (M, N, K)
    return a[:M, :K].to(torch.bfloat16), w[:N, :K].to(torch.bfloat16), bias[:N].to(torch.float32)


def residual(M, N):
    g = torch.Generator().manual_seed(977 * M + N)
    return torch.randint(-1000, 1001, (M, N), generator=g, dtype=torch.int32).to(torch.float32)


_PRODUCTS = {}


def product(M, N, K):
    """A W^T in float64, exact: at least M rows.  One product is kept per (N, K), at the most rows asked for so far (a case of
    fewer rows is a prefix), and only the last few (N, K)."""
    have = _PRODUCTS.get((N, K))
    if have is None or have.shape[0] < M:
        a, w, _ = operands(M, N, K)
        have = a.to(F64) @ w.to(F64).T
        _PRODUCTS.pop((N, K), None)
        while len(_PRODUCTS) >= 6:
            _PRODUCTS.pop(next(iter(_PRODUCTS)))
        _PRODUCTS[(N, K)] = have
    return have


def out_dtype(epi):
    return torch.bfloat16 if epi in (EPI_BIAS_BF16, EPI_BIAS_GELU_BF16) else torch.float32


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def round_bf16(x64, truncate=False):
    """float64 -> bf16, to nearest with ties to even as the hardware converts (through fp32, which holds these values exactly);
    ``truncate`` is the mistake of dropping the low 16 bits."""
    f = x64.to(torch.float32)
    if truncate:
        return (f.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    return f.to(torch.bfloat16)


def buffer(c):
    """What the call is given as C: the residual (HMM_EPI_BIAS_RESID_F32) or the canary in the M rows, the canary behind."""
    dt = out_dtype(c.epi)
    buf = torch.full((c.M + GUARD_ROWS, c.N), float("nan") if dt == torch.bfloat16 else CANARY_F32, dtype=dt)
    if c.epi == EPI_BIAS_RESID_F32:
        buf[:c.M] = c.resid
    return buf


def finish(c, acc64, *, bias_times=1, truncate=False):
    """The output buffer that a kernel with accumulators ``acc64`` leaves: epilogue, rounding, canary rows.  HMM_EPI_BIAS_GELU_BF16
    gives the rounded float64 GELU.  The keywords are mistakes for tests/test_cpu_gemm_cases.py."""
    x = acc64 + bias_times * c.bias.to(F64)
    out = buffer(c)
    if c.epi == EPI_BIAS_RESID_F32:
        out[:c.M] = (x + c.resid.to(F64)).to(torch.float32)
    elif c.epi == EPI_F32:
        out[:c.M] = x.to(torch.float32)
    elif c.epi == EPI_BIAS_BF16:
        out[:c.M] = round_bf16(x, truncate)
    else:
        out[:c.M] = round_bf16(gelu64(x), truncate)
    return out


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- GELU -----------------------------------------------------------------------------------------------------------------
def gelu_model_f32(x):
    """gelu_erf of gemm_bf16.hip, operation by operation in numpy float32 (an fma as the float64 product and sum rounded once to
    float32; the reciprocal and the exponential correctly rounded, which v_rcp / v_exp are not)."""
    f32 = np.float32
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(f32) if not isinstance(b, np.ndarray) else \
        (a.astype(np.float64) * b.astype(np.float64) + np.float64(c)).astype(f32)
    x = np.asarray(x, dtype=f32)
    u = np.abs(x)
    with np.errstate(under="ignore"):
        t = (f32(1.0) / fma(u, f32(0.3275911) * f32(0.70710678118654752440), f32(1.0))).astype(f32)
        poly = fma(t, f32(0.5) * f32(1.061405429), f32(0.5) * f32(-1.453152027))
        poly = fma(poly, t, f32(0.5) * f32(1.421413741))
        poly = fma(poly, t, f32(0.5) * f32(-0.284496736))
        poly = fma(poly, t, f32(0.5) * f32(0.254829592))
        poly = (poly * t).astype(f32)
        e = np.exp2(((u * u).astype(f32) * (f32(-0.5) * f32(1.4426950408889634))).astype(f32)).astype(f32)
        return (np.maximum(x, f32(0.0)) - ((u * poly).astype(f32) * e).astype(f32)).astype(f32)


@functools.lru_cache(maxsize=None)
def gelu_sweep():
    """The pre-activations, fp32 (a torch tensor whose length is a multiple of 256): a dense grid on [-9, 9] (8192 points, each
    fp32), every bf16 value in [-6, 6] (both zeros and the subnormals among them), +-2^-126, +-20, +-30; padded with 0.5.
    No infinity and no NaN: the header promises nothing for them."""
    grid = torch.linspace(-9.0, 9.0, 8192, dtype=F64).to(torch.float32)
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).to(torch.float32)
    allb = allb[torch.isfinite(allb) & (allb.abs() <= 6.0)]
    special = torch.tensor([0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 20.0, -20.0, 30.0, -30.0], dtype=torch.float32)
    x = torch.cat([grid, allb, special])
    pad = (-len(x)) % 256
    return torch.cat([x, torch.full((pad,), 0.5)])


@functools.lru_cache(maxsize=None)
def gelu_slack():
    """(model error, a): the worst |gelu_model_f32(x) - float64 GELU(x)| / max(|x|, 1) over the sweep, and twice that -- the
    margin is for v_rcp and v_exp, approximations of about one ulp that the model does not have."""
    x = gelu_sweep()
    got = torch.from_numpy(gelu_model_f32(x.numpy())).to(F64)
    err = (got - gelu64(x.to(F64))).abs() / x.to(F64).abs().clamp(min=1.0)
    worst = float(err.max())
    return worst, 2.0 * worst


BF16_SUBNORMAL_STEP = 2.0 ** -133         # bf16 subnormals are multiples of 2^-133


def gelu_tolerance(x64):
    """Per element: 2^-8 |want| for the one bf16 rounding of the result (at most 2^-9 of the power of two above it) and a |x| for
    the fp32 evaluation of the formula.  The sweep holds every bf16 value down to the subnormals, whose results (x / 2) fall on
    the bf16 subnormal grid, where rounding is no longer relative but up to half a step: one step of that grid, 2^-133 = 9.2e-41,
    is added, so that the correctly rounded float64 reference uses half of the tolerance there as it does everywhere else."""
    return 2.0 ** -8 * gelu64(x64).abs() + gelu_slack()[1] * x64.abs() + BF16_SUBNORMAL_STEP


def gelu_ratio(x64, got):
    """Worst |got - want| / tolerance over the elements; inf for a NaN or an infinity."""
    r = (got.to(F64) - gelu64(x64)).abs() / gelu_tolerance(x64)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


# ---- comparison -----------------------------------------------------------------------------------------------------------
def check(c, got):
    """Raises AssertionError when ``got`` -- the whole buffer after the call, on the CPU, or a mutant's finish() -- is not the
    case's result."""
    want = c.want
    assert got.dtype == want.dtype and got.shape == want.shape, (c.label, got.dtype, got.shape)
    assert torch.equal(bits(got[c.M:]), bits(want[c.M:])), f"{c.label}: rows past M were written"
    if c.epi == EPI_BIAS_GELU_BF16:
        r = gelu_ratio(c.x64, got[:c.M])
        assert r <= 1.0, f"{c.label}: GELU is off by {r:.3f} of the tolerance"
        return
    same = (bits(got[:c.M]) == bits(want[:c.M]))
    if not bool(same.all()):
        m, n = (int(v) for v in torch.nonzero(~same)[0])
        raise AssertionError(f"{c.label}: {int((~same).sum())} of {same.numel()} elements differ from the exact result; first at "
                             f"[{m}][{n}]: got {float(got[m, n])}, want {float(want[m, n])}")


def make_case(label, M, N, K, epi, tile, group, **extra):
    a, w, bias = operands(M, N, K)
    c = NS(label=label, M=M, N=N, K=K, epi=epi, tile=tile, group=group, a=a, w=w, bias=bias,
           resid=residual(M, N) if epi == EPI_BIAS_RESID_F32 else None, **extra)
    c.acc = product(M, N, K)[:M]
    c.x64 = c.acc + bias.to(F64)
    c.want = finish(c, c.acc)
    return c


# ---- the geometry table ---------------------------------------------------------------------------------------------------
def _up(x, unit):
    return -(-x // unit) * unit


def geometry_shapes(g):
    """The (M, N, K) of one named tiled geometry: M in {1, BM-1, BM+1, 2 BM + 17}; N one column tile rounded up to the ABI's 128 (256
    for the 256-column tiles, which another geometry replaces otherwise) and three column tiles, likewise; K groups of 64 KSUB in
    {1, 2, STAGES-1, STAGES, STAGES+1, 2 STAGES+1} -- the ring's prologue guard, a ring that is never full, full once, and
    wrapped -- and {1, 2, 3, 5} for the double buffer and for the ping-pong loop's steps of 128."""
    BM, BN, stages, ksub = GEOMETRY[g]
    unit = 256 if BN == 256 else 128
    ns = sorted({_up(BN, unit), _up(3 * BN, unit)})
    groups = (1, 2, 3, 5) if stages in (0, 2) else sorted({1, 2, stages - 1, stages, stages + 1, 2 * stages + 1})
    return [(M, N, kg * 64 * ksub) for M in (1, BM - 1, BM + 1, 2 * BM + 17) for N in ns for kg in groups]


@functools.lru_cache(maxsize=None)
def sliver_shapes():
    """(class, M, N, K) of the sliver kernel forced by name: for each instantiation (16, 32, 64 rows per wave; 8, 6, 4 K steps in
    flight) K tiles of 64 in {1, DEPTH-1, DEPTH, DEPTH+1, 2 DEPTH-1, 2 DEPTH, 2 DEPTH+1} -- the re-load of the last step for
    KT < DEPTH and both bounds of the branch-free loop -- at the smallest and the largest M below 400 that the plan entry gives
    that class (the class is sliver_mt's choice by M, N and K), at the narrowest N of 128, 384, 1024 that has one."""
    rows = []
    for mt, depth in SLIVER_DEPTH.items():
        for kt in sorted({1, depth - 1, depth, depth + 1, 2 * depth - 1, 2 * depth, 2 * depth + 1}):
            K = 64 * kt
            for N in (128, 384, 1024):
                ms = [M for M in range(1, 400) if plan(M, N, K, EPI_F32, SLIVER)[0][4] == mt]
                if ms:
                    rows += [(mt, M, N, K) for M in sorted({ms[0], ms[-1]})]
                    break
    return tuple(rows)


def geometry_specs(g):
    """Specs (cheap) of geometry g over the four epilogues."""
    if g == SLIVER:
        shapes = [(M, N, K, f",class={mt}") for mt, M, N, K in sliver_shapes()]
    else:
        shapes = [(M, N, K, "") for M, N, K in geometry_shapes(g)]
    return tuple(NS(group="geometry", tile=g, M=M, N=N, K=K, epi=epi, label=f"tile={g}{tag},M={M},N={N},K={K},epi={epi}")
                 for M, N, K, tag in shapes for epi in EPIS)


# ---- the split-K table ----------------------------------------------------------------------------------------------------
SPLITK_N = 768                          # a width hmm_op_layernorm_reduce_bf16 takes; 6 / 12 / 24 column tiles


def splitk_specs(g):
    """Ring geometry g with 1, 2, 4, 8 splits over slabs of 1 .. 5 K-tiles (where KSUB divides the slab) at M = BM + 17: two row
    tiles, the second ragged, so that slab s + 1 starts right behind the rows of slab s."""
    BM, _, _, ksub = GEOMETRY[g]
    return tuple(NS(group="splitk", tile=g, M=BM + 17, N=SPLITK_N, K=64 * kt * splits, splits=splits,
                    label=f"tile={g},splits={splits},slab={kt}x64,M={BM + 17}")
                 for splits in (1, 2, 4, 8) for kt in (1, 2, 3, 4, 5) if kt % ksub == 0)


def splitk_case(s):
    a, w, bias = operands(s.M, s.N, s.K)
    kl = s.K // s.splits
    slabs = torch.stack([a[:, i * kl:(i + 1) * kl].to(F64) @ w[:, i * kl:(i + 1) * kl].to(F64).T for i in range(s.splits)])
    return NS(**vars(s), a=a, w=w, bias=bias, resid=residual(s.M, s.N), slabs=slabs)


def splitk_want(c, slabs64=None):
    """The partial buffer after the call: [splits][M][N] fp32 and GUARD_ROWS canary rows behind the last slab."""
    slabs64 = c.slabs if slabs64 is None else slabs64
    out = torch.full((c.splits * c.M + GUARD_ROWS, c.N), CANARY_F32, dtype=torch.float32)
    out[:c.splits * c.M] = slabs64.to(torch.float32).reshape(c.splits * c.M, c.N)
    return out


def splitk_check(c, got):
    want = splitk_want(c)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(bits(got[c.splits * c.M:]), bits(want[c.splits * c.M:])), f"{c.label}: rows past the last slab were written"
    for i in range(c.splits):
        same = bits(got[i * c.M:(i + 1) * c.M]) == bits(want[i * c.M:(i + 1) * c.M])
        assert bool(same.all()), (f"{c.label}: slab {i}: {int((~same).sum())} elements differ from the product of its own K range; "
                                  f"first at {tuple(int(v) for v in torch.nonzero(~same)[0])}")


def splitk_reduced(c):
    """x after hmm_op_layernorm_reduce_bf16: slabs + bias + residual, exact."""
    return (c.slabs.sum(0) + c.bias.to(F64) + c.resid.to(F64)).to(torch.float32)


# ---- the route table ------------------------------------------------------------------------------------------------------
# The towers' GEMMs as (N, K): qkv, out-proj, fc1, fc2 of the vision, text and audio towers, and the heads.
TOWER_NK = ((3840, 1280), (1280, 1280), (5120, 1280), (1280, 5120), (3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096),
            (2304, 768), (768, 768), (3072, 768), (768, 3072), (1024, 1280), (1024, 768))
# The families search_routes() scans along M: the widths at which a tile-count rule changes sides within 4200 rows, and for K
# the smallest (128), the ping-pong kernel's refusal (64), and both sides of every K limit and divisibility of small_tile.
SEARCH_N = (256, 512, 768, 1024, 1280, 2304, 3072, 3840, 4096, 5120)
SEARCH_K = (64, 128, 896, 1024, 1088, 1792, 2048, 2176, 4992, 5120)


def search_routes(max_m=4200):
    """Both sides of every change of plan along M, for AUTO and AUTO_TILED over SEARCH_N x SEARCH_K: for every distinct (signature
    before, signature after) the change with the fewest multiply-adds is kept.  Returns rows (M, N, K, tile), two per change."""
    best = {}
    for tile in (AUTO, AUTO_TILED):
        for N in SEARCH_N:
            for K in SEARCH_K:
                prev = None
                for M in range(1, max_m + 1):
                    sig = signature(plan(M, N, K, EPI_F32, tile))
                    if prev is not None and sig != prev:
                        key = (prev, sig)
                        if key not in best or M * N * K < best[key][0] * best[key][1] * best[key][2]:
                            best[key] = (M, N, K, tile)
                    prev = sig
    rows = set()
    for M, N, K, tile in best.values():
        rows.add((M - 1, N, K, tile))
        rows.add((M, N, K, tile))
    return sorted(rows, key=lambda r: (r[3], r[1], r[2], r[0]))


def _g(*ids):
    return tuple((i, 0, 0) for i in ids)


_S1 = ((SLIVER, 1, 0),)                                        # the one-wave kernel, 16 rows per wave, as the whole launch
_RING_PEEL = ((14, 0, 0), (SLIVER, 1, FLAG_SLIVER_PEEL))       # full 128-row tiles on the ring, the last rows through the sliver kernel
_PP_PEEL1 = ((PP, 0, 0), (14, 0, FLAG_PP_TAIL, 1))             # ping-pong on whole rounds, one 256-row tile peeled
_PP_PEEL2 = ((PP, 0, 0), (14, 0, FLAG_PP_TAIL, 2))             # ... two row tiles peeled


def _r(M, N, K, auto, tiled=None, auto64=None, tiled64=None):
    tiled = auto if tiled is None else tiled
    return (M, N, K, {(AUTO, 128): auto, (AUTO_TILED, 128): tiled, (AUTO, 64): auto if auto64 is None else auto64,
                      (AUTO_TILED, 64): (tiled if auto64 is None else auto64) if tiled64 is None else tiled64})


# What search_routes() found at the commit that added this file, with the plan's signature the dispatcher gave then: for AUTO,
# for AUTO_TILED where it differs, and for small_tiles = 64 (what a forward on two chains passes) where that differs.  LITERAL on
# purpose: test_cpu_gemm_cases.py asks the plan entry for every row, so a threshold that moves, or a row of kDispatchRules that
# goes, fails there on the row that sat next to it -- and the row says which route lost its case.  Neighbouring rows are the two
# sides of one limit.
ROUTES = [
    # K % 128 != 0 refuses the ping-pong path (256 x 256, or 256 x 128 where N % 256 != 0); the sliver kernel's fitted lines;
    # the deep-K rings' limits in K (>= 1024 and even, >= 2048 and a multiple of four K-tiles)
    _r(17, 256, 64, _g(2)), _r(17, 256, 128, _g(8)), _r(17, 256, 896, _S1, _g(8)), _r(17, 256, 1024, _S1, _g(9)),
    _r(17, 256, 1088, _g(2)), _r(17, 256, 1792, _S1, _g(9)), _r(17, 256, 2048, _g(10)), _r(17, 256, 2112, _g(2)),
    _r(17, 256, 4096, _S1, _g(10)), _r(17, 256, 4992, _S1, _g(9)), _r(1, 640, 64, _g(1)),
    # g_gemm_rect64_min_t64 / one 64 x 128 tile per CU; the 64 x 64 deep-K ring's 256 tiles; g_gemm_rect_rows_longk in K and in M
    _r(1600, 1280, 128, _g(13)), _r(1601, 1280, 128, _g(14)), _r(768, 1280, 1024, _g(11)), _r(769, 1280, 1024, _g(7)),
    _r(1000, 1280, 4992, _g(7)), _r(1000, 1280, 5120, _g(15)), _r(1536, 1280, 5120, _g(15)), _r(1537, 1280, 5120, _g(13)),
    # g_gemm_rect_rows (700 / 701), g_gemm_rect64_min_t64 (432 / 468 tiles), g_gemm_small_64 (>512 tiles: the 128 x 128 ring)
    _r(1000, 2304, 64, _g(2)), _r(700, 2304, 128, _g(15)), _r(701, 2304, 128, _g(7)), _r(768, 2304, 128, _g(7)),
    _r(769, 2304, 128, _g(13)), _r(1000, 2304, 128, _g(14)),
    # 16 / 17 rows: where the sliver kernel stops winning; g_gemm_small_32 / g_gemm_deepk: the 32 x 32 rings and their tile limits
    _r(16, 2304, 896, _S1, _g(8)), _r(17, 2304, 896, _g(8)), _r(16, 2304, 1024, _S1, _g(9)), _r(17, 2304, 1024, _g(9)),
    _r(17, 2304, 1088, _g(2)), _r(17, 2304, 1792, _g(9)), _r(65, 2304, 1792, _g(8)), _r(17, 2304, 2048, _g(10)),
    _r(65, 2304, 2048, _g(10)), _r(16, 2304, 4096, _S1, _g(10)), _r(17, 2304, 4096, _g(10)), _r(65, 2304, 4096, _g(10)),
    _r(17, 2304, 4992, _g(9)), _r(65, 2304, 4992, _g(8)),
    # g_gemm_rect: 64 x 64 tiles outnumber the CUs (320 / 321 rows) while 128 x 64 tiles do not (640 / 641); one 128 x 128 ring tile
    # per CU (1280 rows) and g_gemm_ring_peel_rows behind it (1 .. 16 / 17 rows); with small_tiles 64 these are ping-pong launches
    _r(320, 3072, 128, _g(7)), _r(321, 3072, 128, _g(15)), _r(640, 3072, 128, _g(15)), _r(641, 3072, 128, _g(14)),
    _r(1280, 3072, 128, _g(14)), _r(1281, 3072, 128, _RING_PEEL, auto64=_g(PP)), _r(1296, 3072, 128, _RING_PEEL, auto64=_g(PP)),
    _r(1297, 3072, 128, _g(0), auto64=_g(PP)), _r(320, 3072, 1024, _g(11)), _r(321, 3072, 1024, _g(15)),
    _r(300, 3840, 64, _g(2)), _r(300, 3840, 128, _g(15)), _r(32, 3840, 1024, _g(9)), _r(33, 3840, 1024, _g(8)),
    # small_tiles: 112 / 128 ping-pong tiles, and 48 / 64 of them
    _r(1792, 4096, 128, _g(0), auto64=_g(PP)), _r(1793, 4096, 128, _g(PP)),
    _r(768, 4096, 128, _g(14)), _r(769, 4096, 128, _g(14), auto64=_g(PP)),
    _r(65, 5120, 64, _g(2)), _r(1000, 5120, 64, _g(2)), _r(64, 5120, 128, _g(8)), _r(65, 5120, 128, _g(7)),
    _r(1000, 5120, 128, _g(0), auto64=_g(PP)),
    # the ping-pong peel: 240 tiles; 260 = one round + one row tile peeled (and 280: the same); 300: two peeled; 15 row tiles: none
    _r(3072, 5120, 128, _g(PP)), _r(3073, 5120, 128, _PP_PEEL1), _r(3328, 5120, 128, _PP_PEEL1), _r(3329, 5120, 128, _PP_PEEL2),
    _r(3584, 5120, 128, _PP_PEEL2), _r(3585, 5120, 128, _g(PP)),
    _r(65, 5120, 896, _g(7)), _r(64, 5120, 1024, _g(8)), _r(65, 5120, 1024, _g(11)), _r(65, 5120, 1088, _g(2)),
    _r(32, 5120, 2048, _g(10)), _r(33, 5120, 2048, _g(8)),
]
# What no AUTO choice reaches today, by name: (M, N, K, tile, signature).  The four-wave rings 6 / 12 / 16 (g_gemm_ring8 chose their
# eight-wave forms), the sliver kernel's 32- and 64-row classes, the ping-pong kernel with a guarded last row tile, the peeled
# launch by name, and 256 x 256 falling to 256 x 128 where N % 256 != 0.
NAMED_ROUTES = [
    (130, 384, 256, 6, _g(6)), (130, 384, 256, 12, _g(12)), (130, 384, 256, 16, _g(16)), (65, 1024, 512, SLIVER, ((SLIVER, 2, 0),)),
    (161, 1024, 512, SLIVER, ((SLIVER, 4, 0),)), (300, 256, 128, PP, _g(PP)), (3329, 5120, 128, PP_PEELED, _PP_PEEL2),
    (130, 384, 64, 2, _g(1)),
]
# Plan only (the operands would not fit the pools, or the GPU test's few seconds): the ping-pong kernel's 32-bit staging offsets.
PLAN_ONLY_ROUTES = [(420000, 5120, 5120, AUTO, _g(2)), (419430, 5120, 5120, AUTO, _PP_PEEL1)]


@functools.lru_cache(maxsize=None)
def route_specs():
    out = []
    for i, (M, N, K, sigs) in enumerate(ROUTES):
        for tile in (AUTO, AUTO_TILED):
            if tile == AUTO_TILED and all(sigs[(AUTO_TILED, st)] == sigs[(AUTO, st)] for st in (128, 64)):
                continue                                     # the same launches: one GPU run
            out.append(NS(group="route", M=M, N=N, K=K, epi=EPIS[i % 4], tile=tile, sig128=sigs[(tile, 128)], sig64=sigs[(tile, 64)],
                          label=f"M={M},N={N},K={K},epi={EPIS[i % 4]},tile={tile}"))
    for i, (M, N, K, tile, sig) in enumerate(NAMED_ROUTES):
        out.append(NS(group="route", M=M, N=N, K=K, epi=EPIS[(i + 1) % 4], tile=tile, sig128=sig, sig64=sig,
                      label=f"M={M},N={N},K={K},epi={EPIS[(i + 1) % 4]},tile={tile}"))
    return tuple(out)


def case(spec):
    """The inputs and the exact result of a geometry or route spec (built on demand, never modified)."""
    return make_case(spec.label, spec.M, spec.N, spec.K, spec.epi, spec.tile, spec.group)


def from_row_zero(c, recs):
    """The mistake of a peel that reads A from row 0 instead of its own first row: the accumulators of every launch but the first
    are those of rows 0 .. of A."""
    acc = c.acc.clone()
    for _, row0, rows, _, _, _ in recs[1:]:
        acc[row0:row0 + rows] = c.acc[:rows]
    return acc


if __name__ == "__main__":
    for M, N, K, tile in search_routes():
        print((M, N, K, tile), signature(plan(M, N, K, EPI_F32, tile)), signature(plan(M, N, K, EPI_F32, tile, 64)))
