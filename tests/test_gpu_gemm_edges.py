"""GPU: the bf16 GEMM (hmm_op_gemm_bf16_tile, hmm_op_gemm_bf16_splitk, hmm_op_layernorm_reduce_bf16's sum) at every geometry, at the
ends of every K pipeline, on every route of the dispatcher and across the GELU's whole domain, against the exact integer reference
of tests/gemm_cases.py, where the inputs, the tables and the comparison live; tests/test_cpu_gemm_cases.py proves without a GPU
that the same comparison on the same inputs rejects a subtly wrong kernel, and that the route table holds every route.

The bitwise tests of tests/test_gpu_ops.py run the product's shapes on random data and pin the order of the epilogue's sums;
this module runs the shapes at which the code takes another path, on operands whose result needs no tolerance.  Every output
buffer carries canary rows behind its end.  The worst GELU error per kernel and the launches per geometry go to
profiles/gemm_edges_parity.json when every test of the module has run and passed in one session (a partial run, -k or a
failure, leaves the file alone).
"""
import json
from collections import Counter
from pathlib import Path

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

PROFILE = Path(__file__).resolve().parent.parent / "profiles" / "gemm_edges_parity.json"
LAUNCHES = Counter()                     # geometry id -> launches the exact tables made on it
GELU_RATIO = {}                          # kernel -> worst |error| / tolerance over the sweep
TABLES_RUN = set()


def _lib():
    from hippomm_amd import _lib as L
    return L, L.load()


def _row(t, m):
    return t.data_ptr() + m * t.shape[1] * t.element_size()


def gemm(ad, wd, bd, cd, M, N, K, epi, tile, row0=0):
    """hmm_op_gemm_bf16_tile on rows [row0, row0 + M) of device tensors, counted per planned launch."""
    L, lib = _lib()
    for rec in G.plan(M, N, K, epi, tile):
        LAUNCHES[rec[0]] += 1
    L.check(lib.hmm_op_gemm_bf16_tile(_row(ad, row0), wd.data_ptr(), bd.data_ptr(), _row(cd, row0), M, N, K, epi, tile, L.stream_ptr()),
            "gemm")


def run(c, tile=None):
    """The whole buffer after the call of a case, back on the CPU."""
    ad, wd, bd, cd = c.a.cuda(), c.w.cuda(), c.bias.cuda(), G.buffer(c).cuda()
    gemm(ad, wd, bd, cd, c.M, c.N, c.K, c.epi, c.tile if tile is None else tile)
    torch.cuda.synchronize()
    return cd.cpu()


def _run_table(specs):
    assert specs
    worst = 0.0
    for s in specs:
        c = G.case(s)
        got = run(c)
        G.check(c, got)
        if c.epi == G.EPI_BIAS_GELU_BF16:
            worst = max(worst, G.gelu_ratio(c.x64, got[:c.M]))
    print(f"{len(specs)} cases; GELU epilogue: worst error {worst:.3f} of the tolerance")


@pytest.mark.parametrize("g", sorted(G.GEOMETRY))
def test_named_geometry_at_the_ends_of_its_k_pipeline(g):
    """M in {1, BM-1, BM+1, 2 BM + 17} x one and three column tiles x K groups {1, 2, STAGES-1, STAGES, STAGES+1, 2 STAGES+1} (ping-pong
    and the double buffer: {1, 2, 3, 5}) x the four epilogues."""
    _run_table(G.geometry_specs(g))
    TABLES_RUN.add(("geometry", g))


def test_sliver_kernel_at_the_ends_of_its_k_loop_in_each_instantiation():
    """KT in {1, DEPTH-1, DEPTH, DEPTH+1, 2 DEPTH-1, 2 DEPTH, 2 DEPTH+1} for 16, 32 and 64 rows per wave."""
    assert {s.label.split("class=")[1][0] for s in G.geometry_specs(G.SLIVER)} == {"1", "2", "4"}
    _run_table(G.geometry_specs(G.SLIVER))
    TABLES_RUN.add(("geometry", G.SLIVER))


@pytest.mark.parametrize("g", G.RING_IDS)
def test_split_k_slabs_and_the_layernorm_that_reduces_them(g):
    """Each slab is the product of its own K range, exactly; the canary behind the last slab stays; and x after
    hmm_op_layernorm_reduce_bf16 is exactly slabs + bias + residual."""
    L, lib = _lib()
    for s in G.splitk_specs(g):
        c = G.splitk_case(s)
        ad, wd = c.a.cuda(), c.w.cuda()
        part = torch.full((c.splits * c.M + G.GUARD_ROWS, c.N), G.CANARY_F32, dtype=torch.float32, device="cuda")
        LAUNCHES[G.plan(c.M, c.N, c.K, G.EPI_F32, g, splits=c.splits)[0][0]] += 1
        L.check(lib.hmm_op_gemm_bf16_splitk(ad.data_ptr(), wd.data_ptr(), part.data_ptr(), c.M, c.N, c.K, c.splits, g, L.stream_ptr()),
                "gemm_splitk")
        torch.cuda.synchronize()
        G.splitk_check(c, part.cpu())
        x = torch.cat([c.resid, torch.full((G.GUARD_ROWS, c.N), G.CANARY_F32)]).cuda()
        y = torch.full((c.M + G.GUARD_ROWS, c.N), float("nan"), dtype=torch.bfloat16, device="cuda")
        bd, gamma, beta = c.bias.cuda(), torch.ones(c.N, device="cuda"), torch.zeros(c.N, device="cuda")
        L.check(lib.hmm_op_layernorm_reduce_bf16(x.data_ptr(), part.data_ptr(), c.splits, bd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                                 y.data_ptr(), c.M, c.N, 1e-5, L.stream_ptr()), "layernorm_reduce")
        torch.cuda.synchronize()
        x, y = x.cpu(), y.cpu()
        assert torch.equal(G.bits(x[:c.M]), G.bits(G.splitk_reduced(c))), f"{c.label}: x is not slabs + bias + residual"
        assert bool((x[c.M:] == G.CANARY_F32).all()) and bool(torch.isnan(y[c.M:].float()).all()), f"{c.label}: rows past M were written"
        assert bool(torch.isfinite(y[:c.M].float()).all()), c.label
    TABLES_RUN.add(("splitk", g))


@pytest.mark.parametrize("spec", G.route_specs(), ids=[s.label for s in G.route_specs()])
def test_route(spec):
    """The call as the table's row names it (what hmm_op_gemm_bf16_tile launches is the row's plan: the CPU census checks that):
    the exact result, and the bits of geometry 0 on the same operands.  Where small_tiles = 64 -- what a forward on two chains
    passes and no hmm_op_* entry does -- plans something else, those launches are forced by id on their row ranges."""
    c = G.case(spec)
    assert G.signature(G.plan(c.M, c.N, c.K, c.epi, c.tile)) == spec.sig128
    ad, wd, bd = c.a.cuda(), c.w.cuda(), c.bias.cuda()
    outs = {}
    for tile in (c.tile, 0):
        cd = G.buffer(c).cuda()
        gemm(ad, wd, bd, cd, c.M, c.N, c.K, c.epi, tile)
        outs[tile] = cd.cpu()
    G.check(c, outs[c.tile])
    assert torch.equal(G.bits(outs[c.tile][:c.M]), G.bits(outs[0][:c.M])), f"{c.label}: differs from the 128 x 128 kernel"
    if spec.tile in (G.AUTO, G.AUTO_TILED) and spec.sig64 != spec.sig128:
        recs = G.plan(c.M, c.N, c.K, c.epi, c.tile, 64)
        assert G.signature(recs) == spec.sig64
        cd = G.buffer(c).cuda()
        for g, row0, rows, _, mt, _ in recs:
            assert G.plan(rows, c.N, c.K, c.epi, g) == ((g, 0, rows, 1, mt, 0),)        # by name, these rows run as planned
            gemm(ad, wd, bd, cd, rows, c.N, c.K, c.epi, g, row0)
        forced = cd.cpu()
        G.check(c, forced)
        assert torch.equal(G.bits(forced[:c.M]), G.bits(outs[0][:c.M])), f"{c.label}: the small_tiles = 64 plan differs from the 128 x 128 kernel"
    TABLES_RUN.add(("route", spec.label))


GELU_KERNELS = {"128x128": (0, 3), "ping-pong": (G.PP, 3), "sliver": (G.SLIVER, 1)}      # name -> (tile, M)


@pytest.mark.parametrize("kernel", sorted(GELU_KERNELS))
def test_gelu_over_its_whole_domain(kernel):
    """A = 0 and the bias carrying the sweep, so the pre-activation is the bias exactly: a dense grid on [-9, 9], every bf16 value
    in [-6, 6], +-0, +-2^-126, +-20, +-30, against float64 0.5 x (1 + erf(x / sqrt 2)) under gemm_cases.gelu_tolerance."""
    tile, M = GELU_KERNELS[kernel]
    x = G.gelu_sweep()
    N, K = len(x), 128
    assert G.plan(M, N, K, G.EPI_BIAS_GELU_BF16, tile) == ((tile, 0, M, 1, 1 if tile == G.SLIVER else 0, 0),)
    ad = torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")
    wd = torch.zeros(N, K, dtype=torch.bfloat16, device="cuda")
    cd = torch.full((M + G.GUARD_ROWS, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    L, lib = _lib()
    L.check(lib.hmm_op_gemm_bf16_tile(ad.data_ptr(), wd.data_ptr(), x.cuda().data_ptr(), cd.data_ptr(), M, N, K, G.EPI_BIAS_GELU_BF16, tile,
                                      L.stream_ptr()), "gemm")
    torch.cuda.synchronize()
    got = cd.cpu()
    assert bool(torch.isnan(got[M:].float()).all()), "rows past M were written"
    assert bool((G.bits(got[:M]) == G.bits(got[:1])).all()), "rows of the same pre-activations differ"
    r = G.gelu_ratio(x.double(), got[0])
    GELU_RATIO[kernel] = r
    print(f"gelu {kernel}: worst error {r:.3f} of the tolerance (a = {G.gelu_slack()[1]:.3e})")
    assert r <= 1.0, f"{kernel}: GELU is off by {r:.3f} of the tolerance"


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    whole = ({("geometry", g) for g in list(G.GEOMETRY) + [G.SLIVER]} | {("splitk", g) for g in G.RING_IDS} |
             {("route", s.label) for s in G.route_specs()}) <= TABLES_RUN
    if not (whole and set(GELU_RATIO) == set(GELU_KERNELS)):
        return                                                       # a partial run leaves the file alone
    model, a = G.gelu_slack()
    PROFILE.write_text(json.dumps({
        "what": "tests/test_gpu_gemm_edges.py: GELU epilogue against float64 over gemm_cases.gelu_sweep(), tolerance 2^-8 |want| + a |x| "
                "(+ one bf16 subnormal step); launches per geometry id made by the exact tables (geometry, split-K, route)",
        "gelu_sweep_points": len(G.gelu_sweep()),
        "gelu_model_error": model, "gelu_a": a,
        "gelu_worst_ratio": {k: round(v, 4) for k, v in sorted(GELU_RATIO.items())},
        "launches_per_geometry": {str(g): LAUNCHES[g] for g in sorted(LAUNCHES)},
    }, indent=1) + "\n")
