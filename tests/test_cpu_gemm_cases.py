"""CPU: the GEMM tables of tests/gemm_cases.py can fail, and reach what they say they reach.  No kernel runs: the dispatcher is
asked through hmm_op_gemm_plan, which launches nothing.

1. Plan properties over a sweep of the towers' shapes.
2. Census: the literal route table still gets the plans written next to its rows, holds every record the sweep can reach, every
   geometry, sliver class, flag and both sides of every row of kDispatchRules -- and what the older fuzz test reaches is on record.
3. Mutants: wrong references through the same inputs and the same comparison; each must be rejected.  What exact integers can NOT
   see -- the order of (accumulator + bias) + residual -- stays pinned by the bitwise tests of tests/test_gpu_ops.py.
4. Conditions on the GELU sweep and its tolerance.
5. The refusals, which happen before any launch.
"""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import gemm_cases as G

ROOT = Path(__file__).resolve().parent.parent


# ---- 1. plan properties ---------------------------------------------------------------------------------------------------
def _sweep_m():
    """1 .. 5000 and 13 000 .. 16 000, sampled: every M to 800, every seventh beyond, every 128-row tile edge with -1, +1 and the ring
    peel's 16 / 17 rows, and in the large range every 37th M and every 256-row tile edge."""
    ms = set(range(1, 801)) | set(range(801, 5001, 7)) | {m + d for m in range(768, 5001, 128) for d in (-1, 0, 1, 16, 17)}
    ms |= set(range(13000, 16001, 37)) | {m + d for m in range(13056, 16001, 256) for d in (-1, 0, 1)}
    return sorted(m for m in ms if 1 <= m <= 16000)


def _legal(rec, N, K):
    g, row0, rows, splits, mt, flags = rec
    if g not in G.ALL_IDS or g == G.PP_PEELED or rows < 1 or splits != 1:
        return False
    if g == G.SLIVER:
        return mt in G.SLIVER_DEPTH
    if mt != 0:
        return False
    BM, BN, stages, ksub = G.GEOMETRY[g]
    return N % (256 if BN == 256 else 128) == 0 and (K // 64) % ksub == 0


@pytest.mark.parametrize("tile", [G.AUTO, G.AUTO_TILED])
def test_plans_tile_the_rows_with_legal_launches(tile):
    """Records tile rows [0, M) in order without gap or overlap; each is legal for its (N, K) -- ping-pong only with N % 256 == 0
    and K % 128 == 0, the deep-K rings only where their K-tiles per stage divide K / 64.  The sliver kernel as the launch is
    AUTO's alone; under AUTO_TILED it appears only as the flagged peel of the last <= 16 rows off a ring launch (plan_small,
    g_gemm_ring_peel_rows: the peel belongs to the tiled route, as include/hippomm_hip.h says of AUTO_TILED)."""
    reached = set()
    for N, K in G.TOWER_NK:
        for small_tiles in (128, 64):
            for M in _sweep_m():
                epi = G.EPIS[M % 4]
                recs = G.plan(M, N, K, epi, tile, small_tiles)
                where = (M, N, K, epi, tile, small_tiles, recs)
                row = 0
                for rec in recs:
                    assert rec[1] == row and _legal(rec, N, K), where
                    row += rec[2]
                    if rec[0] == G.SLIVER and not rec[5] & G.FLAG_SLIVER_PEEL:
                        assert tile == G.AUTO and len(recs) == 1, where
                    if rec[5] & G.FLAG_SLIVER_PEEL:
                        assert rec[0] == G.SLIVER and rec[2] <= 16 and rec is recs[-1] and len(recs) == 2, where
                    if rec[5] & G.FLAG_PP_TAIL:
                        assert recs[0][0] == G.PP and rec is recs[-1] and rec[2] <= 512 and recs[0][2] % 256 == 0, where
                assert row == M, where
                reached |= {(small_tiles, r) for r in G.signature(recs)}
    # ---- census, first half: a record the sweep reaches has a row in the table
    table = _table_records(tile)
    lost = sorted(reached - table)
    assert not lost, f"tile {tile}: (small_tiles, (geometry, sliver class, flags[, peeled row tiles])) without a row in gemm_cases.ROUTES: {lost}"


# ---- 2. census ------------------------------------------------------------------------------------------------------------
def _table_records(tile):
    return {(st, r) for _, _, _, sigs in G.ROUTES for st in (128, 64) for r in sigs[(tile, st)]}


def test_route_table_rows_still_get_their_plans():
    wrong = []
    for M, N, K, sigs in G.ROUTES:
        for (tile, st), want in sigs.items():
            got = G.signature(G.plan(M, N, K, G.EPI_F32, tile, st))
            if got != want:
                wrong.append(f"M={M},N={N},K={K},tile={tile},small_tiles={st}: the table's case for {want} now runs {got}")
    for M, N, K, tile, want in G.NAMED_ROUTES + G.PLAN_ONLY_ROUTES:
        got = G.signature(G.plan(M, N, K, G.EPI_F32, tile))
        if got != want:
            wrong.append(f"M={M},N={N},K={K},tile={tile}: the table's case for {want} now runs {got}")
    assert not wrong, "routes that lost their case:\n" + "\n".join(wrong)


def test_route_specs_carry_the_table():
    specs = G.route_specs()
    assert len({s.label for s in specs}) == len(specs)
    assert {(s.M, s.N, s.K) for s in specs} == {r[:3] for r in G.ROUTES} | {r[:3] for r in G.NAMED_ROUTES}
    assert {s.epi for s in specs} == set(G.EPIS)
    for s in specs:                                                  # the epilogue does not change the plan
        assert len({G.signature(G.plan(s.M, s.N, s.K, e, s.tile)) for e in G.EPIS}) == 1, s.label


def test_route_table_holds_every_geometry_class_flag_and_peel():
    recs = {r for tile in (G.AUTO, G.AUTO_TILED) for _, r in _table_records(tile)} | {r for *_, sig in G.NAMED_ROUTES for r in sig}
    ids = {r[0] for r in recs} | {row[3] for row in G.NAMED_ROUTES}
    assert ids >= set(G.ALL_IDS), sorted(set(G.ALL_IDS) - ids)
    assert {r[1] for r in recs if r[0] == G.SLIVER} == {1, 2, 4}
    assert {r[2] for r in recs} == {0, G.FLAG_PP_TAIL, G.FLAG_SLIVER_PEEL}
    assert {r[3] for r in recs if len(r) == 4} == {1, 2}              # the ping-pong peel of one and of two row tiles ...
    assert any(sigs[(G.AUTO, 128)] == G._g(G.PP) and M > 3000 for M, _, _, sigs in G.ROUTES)   # ... and of none, past 256 tiles
    # the sliver peel at its 16 rows, and 17 rows not peeled
    by_shape = {r[:3]: r[3] for r in G.ROUTES}
    assert by_shape[(1296, 3072, 128)][(G.AUTO, 128)] == G._RING_PEEL and by_shape[(1297, 3072, 128)][(G.AUTO, 128)] == G._g(0)
    assert G.plan(1296, 3072, 128)[1][1:3] == (1280, 16)
    # small_tiles 64, which no hmm_op_* entry passes, changes some rows' plans
    assert any(sigs[(G.AUTO, 64)] != sigs[(G.AUTO, 128)] for *_, sigs in G.ROUTES)


# Both sides of every row of kDispatchRules: two rows of the table that differ by that limit alone.  A side given with four
# numbers is a row of NAMED_ROUTES -- g_gemm_ring8 is on or off for a whole build, so its other side is the four-wave tile by name.
RULE_SIDES = {
    "g_gemm_small_64": [((1600, 1280, 128), (1601, 1280, 128))],                       # 500 / 520 tiles of 64 x 64
    "g_gemm_small_32": [((64, 5120, 128), (65, 5120, 128))],                           # 320 / 480 tiles of 32 x 32
    "g_gemm_deepk": [((17, 2304, 1024), (17, 2304, 896)), ((17, 2304, 2048), (17, 2304, 1792)),      # K >= 1024, K >= 2048
                     ((17, 2304, 2048), (17, 256, 2112)),                                           # K / 64 even / odd
                     ((32, 3840, 1024), (33, 3840, 1024)), ((32, 5120, 2048), (33, 5120, 2048)),    # 192 and 256 tiles of 32 x 32
                     ((768, 1280, 1024), (769, 1280, 1024)), ((65, 5120, 1024), (65, 5120, 896))],  # 64 x 64: 256 tiles, K >= 1024
    "g_gemm_ring8": [((641, 3072, 128), (130, 384, 256, 6)), ((321, 3072, 128), (130, 384, 256, 12))],
    "g_gemm_rect": [((320, 3072, 128), (321, 3072, 128)), ((640, 3072, 128), (641, 3072, 128))],
    "g_gemm_rect_rows": [((700, 2304, 128), (701, 2304, 128))],
    "g_gemm_rect_rows_longk": [((1536, 1280, 5120), (1537, 1280, 5120)), ((1000, 1280, 5120), (1000, 1280, 4992))],
    "g_gemm_rect64_min_t64": [((768, 2304, 128), (769, 2304, 128))],                   # 432 / 468 tiles of 64 x 64
    "g_gemm_ring_peel_rows": [((1296, 3072, 128), (1297, 3072, 128)), ((1280, 3072, 128), (1281, 3072, 128))],
}


def test_both_sides_of_every_dispatch_rule_are_in_the_table():
    text = (ROOT / "hippomm_amd" / "csrc" / "gemm_bf16.hip").read_text()
    table = text[text.index("constexpr DispatchRule kDispatchRules[]"):]
    knobs = re.findall(r'\{"(g_gemm_\w+)",', table[:table.index("};")])
    assert len(knobs) >= 9 and sorted(knobs) == sorted(RULE_SIDES), sorted(set(knobs) ^ set(RULE_SIDES))
    by_shape = {r[:3]: r[3][(G.AUTO_TILED, 128)] for r in G.ROUTES}
    named = {r[:4]: r[4] for r in G.NAMED_ROUTES}
    for knob, pairs in RULE_SIDES.items():
        for a, b in pairs:
            sa, sb = ((named[s] if len(s) == 4 else by_shape[s]) for s in (a, b))
            assert sa != sb, f"{knob}: {a} and {b} are the same route {sa}"


def test_what_the_dispatcher_fuzz_of_test_gpu_ops_reaches_today():
    """On record: the seeded fuzz reaches the one-row-tile ping-pong peel through one random draw, (4104, 4096, .), and the
    two-row-tile peel never; it never draws the sliver kernel's 32- or 64-row classes or the four-wave rings, and small_tiles = 64 is out of its
    reach by construction.
    This pins what test_gpu_ops._dispatch_fuzz_shapes() draws, not the GEMM.  When its seed or its lists change, this test fails
    for that reason alone: print ``recs`` below and write the new facts here -- whatever it then reaches or misses, the routes
    themselves stay covered by gemm_cases.ROUTES."""
    import test_gpu_ops
    shapes = test_gpu_ops._dispatch_fuzz_shapes()
    recs = {}
    for M, N, K, epi in shapes:
        for tile in (G.AUTO, G.AUTO_TILED):
            for r in G.signature(G.plan(M, N, K, epi, tile)):
                recs.setdefault(r, set()).add((M, N))
    assert recs[(14, 0, G.FLAG_PP_TAIL, 1)] == {(4104, 4096)}           # a random draw; its M = 3341 did not draw N = 5120
    assert 5120 not in {N for M, N, _, _ in shapes if M == 3341}
    assert (14, 0, G.FLAG_PP_TAIL, 2) not in recs
    assert {r[1] for r in recs if r[0] == G.SLIVER} == {1}
    assert not {6, 12, 16} & {r[0] for r in recs}
    assert (G.SLIVER, 1, G.FLAG_SLIVER_PEEL) in recs


def test_the_memory_contract_cases_run_one_launcher_kind_each():
    """The GEMM rows of tests/test_gpu_memory_contract.py's ``ops`` group (its _hot_ops), by what they launch."""
    want = {(77, 256, 256, 5): G._S1, (77, 256, 256, 7): G._g(7), (1283, 3072, 128, G.AUTO_TILED): G._RING_PEEL,
            (300, 256, 128, G.PP): G._g(G.PP), (3077, 5120, 128, G.AUTO): G._PP_PEEL1}
    text = (ROOT / "tests" / "test_gpu_memory_contract.py").read_text()
    for (M, N, K, tile), sig in want.items():
        assert f", {M}, {N}, {K}, {tile})" in text, (M, N, K, tile)
        for epi in G.EPIS:
            assert G.signature(G.plan(M, N, K, epi, tile)) == sig, (M, N, K, tile, epi)
    assert G.plan(300, 256, 128, 0, G.PP)[0][2] % 256 != 0                     # a last row tile that needs the guard
    assert G.signature(G.plan(77, 1024, 1024, G.EPI_F32, -1, splits=4)) == G._g(9)


def test_geometry_table_reaches_the_ends_of_every_k_pipeline():
    for g, (BM, BN, stages, ksub) in G.GEOMETRY.items():
        shapes = G.geometry_shapes(g)
        groups = {K // (64 * ksub) for _, _, K in shapes}
        assert groups == ({1, 2, 3, 5} if stages in (0, 2) else {1, 2, stages - 1, stages, stages + 1, 2 * stages + 1}), (g, groups)
        assert {M for M, _, _ in shapes} == {1, BM - 1, BM + 1, 2 * BM + 17}
        for M, N, K in shapes:                                       # the named geometry is the one that runs
            assert [r[0] for r in G.plan(M, N, K, G.EPI_F32, g)] == [g], (g, M, N, K)
        # three column tiles on an odd count of row tiles: a workgroup count that is no multiple of 8 (the XCD remap's remainder)
        assert any((-(-M // BM) * (N // BN)) % 8 for M, N, _ in shapes), g
    by_class = {}
    for mt, M, N, K in G.sliver_shapes():
        by_class.setdefault(mt, set()).add(K // 64)
        assert G.plan(M, N, K, G.EPI_F32, G.SLIVER) == ((G.SLIVER, 0, M, 1, mt, 0),)
    for mt, depth in G.SLIVER_DEPTH.items():
        assert by_class[mt] == {1, depth - 1, depth, depth + 1, 2 * depth - 1, 2 * depth, 2 * depth + 1}, (mt, by_class.get(mt))
    for g in G.RING_IDS:
        ksub = G.GEOMETRY[g][3]
        got = {(s.splits, s.K // s.splits // 64) for s in G.splitk_specs(g)}
        assert got == {(sp, kt) for sp in (1, 2, 4, 8) for kt in (1, 2, 3, 4, 5) if kt % ksub == 0}
        for s in G.splitk_specs(g):
            assert G.plan(s.M, s.N, s.K, G.EPI_F32, g, splits=s.splits) == ((g, 0, s.M, s.splits, 0, 0),)


# ---- 3. mutants -----------------------------------------------------------------------------------------------------------
def _ktile(c, t):
    return c.a[:, 64 * t:64 * t + 64].to(G.F64) @ c.w[:, 64 * t:64 * t + 64].to(G.F64).T


def _row_answered_by_the_row_before(c):
    acc = c.acc.clone()
    acc[c.M - 1] = acc[c.M - 2]
    return acc


def _column_block_shifted(c):
    acc = c.acc.clone()
    acc[:, 16:32] = c.acc[:, 32:48]
    return acc


def _block_transposed(c):
    acc = c.acc.clone()
    acc[:16, :16] = c.acc[:16, :16].T
    return acc


MUTANTS = {  # name -> (applies to the case, the buffer the wrong kernel leaves)
    "one K-tile dropped": (lambda c: True, lambda c: G.finish(c, c.acc - _ktile(c, (c.K // 64) // 2))),
    "the last K-tile used twice": (lambda c: True, lambda c: G.finish(c, c.acc + _ktile(c, c.K // 64 - 1))),
    "row M-1 answered with row M-2": (lambda c: c.M >= 2, lambda c: G.finish(c, _row_answered_by_the_row_before(c))),
    "a 16-column block shifted by 16": (lambda c: True, lambda c: G.finish(c, _column_block_shifted(c))),
    "a 16x16 block transposed": (lambda c: c.M >= 16, lambda c: G.finish(c, _block_transposed(c))),
    "the bias added twice": (lambda c: True, lambda c: G.finish(c, c.acc, bias_times=2)),
    "bf16 by truncation": (lambda c: c.epi == G.EPI_BIAS_BF16 and c.K >= 256, lambda c: G.finish(c, c.acc, truncate=True)),
    "a peel's rows computed from row 0": (lambda c: len(c.recs) == 2, lambda c: G.finish(c, G.from_row_zero(c, c.recs))),
}


def _mutant_cases():
    specs = [s for g in (0, 7, G.PP) for s in G.geometry_specs(g) if s.M > 1 and s.K // 64 in (2, 5)]
    specs += [s for s in G.geometry_specs(G.SLIVER) if s.K // 64 in (5, 8) and s.M > 16]
    specs += [s for s in G.route_specs() if (s.M, s.N) in ((1281, 3072), (1296, 3072), (3073, 5120))]
    for s in specs:
        c = G.case(s)
        c.recs = G.plan(c.M, c.N, c.K, c.epi, c.tile)
        yield c


def test_the_comparison_accepts_the_reference_and_rejects_every_mutant():
    rejected = {name: 0 for name in MUTANTS}
    n = 0
    for c in _mutant_cases():
        n += 1
        G.check(c, G.finish(c, c.acc))
        for name, (applies, wrong) in MUTANTS.items():
            if not applies(c):
                continue
            try:
                G.check(c, wrong(c))
            except AssertionError:
                rejected[name] += 1
            else:
                # exact epilogues see every mutant; GELU saturates (0 below about -9, x above), so it may be blind to some
                assert c.epi == G.EPI_BIAS_GELU_BF16 or name == "bf16 by truncation", f"{c.label} accepts: {name}"
        guard = G.finish(c, c.acc)
        guard[c.M, 5] = 1.0
        with pytest.raises(AssertionError, match="past M"):
            G.check(c, guard)
    assert n >= 40 and all(v >= 2 for v in rejected.values()), rejected


def test_split_k_comparison_rejects_swapped_slabs_and_a_slab_of_the_whole_k():
    rejected = 0
    for g in (7, 9, 14):
        for s in G.splitk_specs(g):
            c = G.splitk_case(s)
            G.splitk_check(c, G.splitk_want(c))
            assert torch.equal(G.splitk_reduced(c), (G.product(c.M, c.N, c.K)[:c.M] + c.bias.double() + c.resid.double()).float())
            if c.splits >= 2:
                swapped = c.slabs.clone()
                swapped[[0, 1]] = c.slabs[[1, 0]]
                with pytest.raises(AssertionError, match="slab 0"):
                    G.splitk_check(c, G.splitk_want(c, swapped))
                rejected += 1
            late = G.splitk_want(c)
            late[c.splits * c.M] = 0.0
            with pytest.raises(AssertionError, match="past the last slab"):
                G.splitk_check(c, late)
    assert rejected >= 2


# ---- 4. GELU --------------------------------------------------------------------------------------------------------------
def test_gelu_sweep_and_tolerance():
    x = G.gelu_sweep()
    assert len(x) % 256 == 0 and bool(torch.isfinite(x).all())
    x64 = x.double()
    assert float(x.min()) == -30.0 and float(x.max()) == 30.0 and int((x < -5).sum()) > 1000 and int((x > 0).sum()) > 10000
    as_bits = set(x.view(torch.int32).tolist())
    for v in (0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 20.0, -20.0, 6.0, -6.0, 2.0 ** -133):
        assert torch.tensor(v, dtype=torch.float32).view(torch.int32).item() in as_bits, v
    every_bf16 = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    every_bf16 = every_bf16[torch.isfinite(every_bf16) & (every_bf16.abs() <= 6)]
    assert set(every_bf16.view(torch.int32).tolist()) <= as_bits and len(every_bf16) > 33000
    model, a = G.gelu_slack()
    assert 5e-8 < model < 5e-7 and a == 2 * model                    # the formula's |error| <= 1.5e-7 on erf, times |x| / 2, and fp32
    # The correctly rounded float64 reference alone.  A bf16 rounding moves a value by up to 2^-8 of the power of two BELOW it, so
    # next to the 2^-8 |want| term it uses half of the tolerance just under a power of two and 256 / 257 of it at the first
    # midpoint above one (2.0078 -> 2.0): "half the tolerance" cannot hold for this tolerance, 256 / 257 is the bound that does.
    # The sweep reaches 0.990 (x = 2.0492, GELU 2.00776).  What is left for the kernel there is a |x| = 6e-7 and the 3e-5 by
    # which 2^-8 |want| exceeds half a step -- two orders above its fp32 error.
    rounded = G.gelu_ratio(x64, G.round_bf16(G.gelu64(x64)))
    assert 0.5 < rounded <= 256.0 / 257.0, rounded
    # the fp32 model of the kernel's formula, rounded, passes; truncated instead of rounded, or with tanh-GELU, it does not
    model_out = torch.from_numpy(G.gelu_model_f32(x.numpy()))
    assert G.gelu_ratio(x64, model_out.to(torch.bfloat16)) <= 1.0
    assert G.gelu_ratio(x64, G.round_bf16(model_out.double(), truncate=True)) > 1.0
    tanh = torch.nn.functional.gelu(x64, approximate="tanh")
    assert G.gelu_ratio(x64, G.round_bf16(tanh)) > 1.0
    assert G.gelu_ratio(x64, G.round_bf16(torch.relu(x64))) > 1.0


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
P = 4096                                 # a non-null pointer that no refused call may touch
REFUSED = [  # label, (a, w, bias, c), M, N, K, epilogue, tile, text; plan: whether hmm_op_gemm_plan can be asked the same
    ("K % 64 != 0", (P, P, P, P), 5, 128, 96, 0, 0, "unsupported shape", True),
    ("N % 128 != 0", (P, P, P, P), 5, 192, 64, 0, 0, "unsupported shape", True),
    ("M = 0", (P, P, P, P), 0, 128, 64, 0, 0, "unsupported shape", True),
    ("null A", (None, P, P, P), 5, 128, 64, 0, 0, "null pointer", False),
    ("null W", (P, None, P, P), 5, 128, 64, 0, 0, "null pointer", False),
    ("null C", (P, P, P, None), 5, 128, 64, 0, 0, "null pointer", False),
    ("epilogue 0, null bias", (P, P, None, P), 5, 128, 64, 0, 0, "needs a bias", False),
    ("epilogue 1, null bias", (P, P, None, P), 5, 128, 64, 1, 0, "needs a bias", False),
    ("epilogue 2, null bias", (P, P, None, P), 5, 128, 64, 2, 0, "needs a bias", False),
    ("epilogue 4", (P, P, P, P), 5, 128, 64, 4, 0, "unknown epilogue 4", True),
    ("tile 17", (P, P, P, P), 5, 128, 64, 0, 17, "unknown tile geometry 17", True),
    ("32x32 K2, K = 192", (P, P, P, P), 5, 128, 192, 0, 9, "not a multiple of 128", True),
    ("32x32 K4, K = 384", (P, P, P, P), 5, 128, 384, 0, 10, "not a multiple of 256", True),
    ("64x64 K2, K = 64", (P, P, P, P), 5, 128, 64, 3, 11, "not a multiple of 128", True),
]


@pytest.mark.parametrize("label,ptrs,M,N,K,epi,tile,text,planned", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_need_no_gpu_and_the_plan_gives_the_same_text(label, ptrs, M, N, K, epi, tile, text, planned):
    from hippomm_amd import _lib as L
    lib = L.load()
    a, w, bias, c = ptrs
    texts = []
    assert lib.hmm_op_gemm_bf16_tile(a, w, bias, c, M, N, K, epi, tile, None) == -1
    texts.append(lib.hmm_last_error().decode())
    if tile == 0:
        assert lib.hmm_op_gemm_bf16(a, w, bias, c, M, N, K, epi, None) == -1
        texts.append(lib.hmm_last_error().decode())
    if planned:
        n, said = G.plan_raw(M, N, K, epi, tile)
        assert n == -1
        texts.append(said)
    assert text in texts[0] and len(set(texts)) == 1, texts


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 17])
def test_split_k_refuses_a_geometry_outside_the_rings(tile):
    from hippomm_amd import _lib as L
    lib = L.load()
    assert lib.hmm_op_gemm_bf16_splitk(P, P, P, 5, 128, 128, 2, tile, None) == -1
    said = lib.hmm_last_error().decode()
    assert f"tile geometry {tile} has no split-K launch" in said
    assert G.plan_raw(5, 128, 128, G.EPI_F32, tile, splits=2) == (-1, said)


def test_plan_entry_bounds_its_output():
    buf = (ctypes.c_int32 * 12)(*([-77] * 12))
    from hippomm_amd import _lib as L
    lib = L.load()
    assert lib.hmm_op_gemm_plan(3329, 5120, 128, 0, G.AUTO, 128, 0, ctypes.addressof(buf), 1) == 2      # two launches, one written
    assert list(buf[:6]) == [G.PP, 0, 3072, 1, 0, 0] and list(buf[6:]) == [-77] * 6
    assert lib.hmm_op_gemm_plan(3329, 5120, 128, 0, G.AUTO, 128, 0, None, 0) == 2
    assert lib.hmm_op_gemm_plan(3329, 5120, 128, 0, G.AUTO, 128, 0, None, 1) == -1
    assert lib.hmm_op_gemm_plan(3329, 5120, 128, 0, G.AUTO, 128, -1, ctypes.addressof(buf), 2) == -1
