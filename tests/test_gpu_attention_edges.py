"""GPU: the attention core (hmm_op_attention_bf16, hmm_op_attention_causal_bf16) at every key-tile, chunk, capacity and route
edge, against the float64 reference of tests/attention_cases.py, where the inputs and the comparison live;
tests/test_cpu_attention_cases.py proves without a GPU that the same comparison on the same inputs rejects a subtly wrong kernel.

test_attention and test_attention_causal (tests/test_gpu_ops.py) run the product's shapes; this module runs the shapes at which
the code takes another path.  Every output buffer is filled with NaN and carries one guard row behind its end.
"""
import pytest
import torch

import attention_cases as A

pytestmark = pytest.mark.gpu


def _lib():
    from hippomm_amd import _lib as L
    return L, L.load()


def _p(t):
    return None if t is None else t.data_ptr()


def call(qkv, B, T, H, dh, bk, bv, causal):
    """One call on CPU inputs -> (status, the B*T output rows on the CPU, still bf16).  The output starts as NaN; the guard row
    behind it must keep its bits."""
    L, lib = _lib()
    rows, D = max(B, 1) * max(T, 1), max(H, 1) * dh
    out = torch.full((rows + 1, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    before = out[rows:].clone()
    qd, bkd, bvd = qkv.cuda(), (None if bk is None else bk.cuda()), (None if bv is None else bv.cuda())
    if causal:
        assert bk is None and bv is None
        rc = lib.hmm_op_attention_causal_bf16(_p(qd), _p(out), B, T, H, dh, L.stream_ptr())
    else:
        rc = lib.hmm_op_attention_bf16(_p(qd), _p(out), B, T, H, dh, _p(bkd), _p(bvd), L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out[rows:].view(torch.int16), before.view(torch.int16)), "the row behind the output was written"
    return rc, out[:rows].cpu()


def run(c):
    """The kernel's output for a case of the table."""
    L, _ = _lib()
    rc, got = call(c.qkv, c.B, c.T, c.H, c.dh, c.bk, c.bv, c.causal)
    L.check(rc, "attention")
    return got


def _group(name):
    return pytest.mark.parametrize("spec", A.specs(name), ids=A.spec_ids(name))


def _value(spec):
    c = A.case(spec)
    got = run(c)
    assert torch.isfinite(got.float()).all(), f"{c.label}: NaN left in the output, or an infinity written"
    print(f"attention {c.label}: worst error {A.ratio(c, got):.3f} of the tolerance")
    A.check(c, got)


@_group("value")
def test_values_at_tile_chunk_and_capacity_edges(spec):
    _value(spec)


@_group("route")
def test_values_on_every_block_map_and_threshold_side(spec):
    _value(spec)


@_group("onehot")
def test_one_hot_rows_pick_exactly_the_right_value_row(spec):
    c = A.case(spec)
    got = run(c)
    assert torch.equal(got, c.picked), f"{c.label}: {int((got != c.picked).any(dim=1).sum())} rows are not the picked V row"
    A.check(c, got)


@pytest.mark.parametrize("T,H,dh,bias,causal,batches", A.INVARIANCE, ids=[f"T={i[0]},H={i[1]},dh={i[2]}" for i in A.INVARIANCE])
def test_sample_bits_do_not_depend_on_batch_size_or_position(T, H, dh, bias, causal, batches):
    """attention_core.h: "the same bits for every q_parts" -- and for every block map.  Sample 0 rides alone, then at the first,
    the middle and the last position of larger batches that take the split (B 8), the even map or the legacy map's second and
    third round (B 9, 17); its rows must keep their bits."""
    pool, bk, bv = A.invariance_pool(T, H, dh, bias, causal)
    L, _ = _lib()
    rc, alone = call(pool[:1].reshape(T, -1), 1, T, H, dh, bk, bv, causal)
    L.check(rc, "attention")
    assert torch.isfinite(alone.float()).all()
    routes = {A.route(1, T, H, dh, bias, causal)[1:4]}
    for B in batches[1:]:
        routes.add(A.route(B, T, H, dh, bias, causal)[1:4])
        for position in (0, B // 2, B - 1):
            rc, got = call(A.invariance_batch(pool, B, position), B, T, H, dh, bk, bv, causal)
            L.check(rc, "attention")
            mine = got.reshape(B, T, -1)[position]
            same = (mine.view(torch.int16) == alone.view(torch.int16)).all(dim=1)
            assert bool(same.all()), (f"B={B}, position {position}: {int((~same).sum())} of sample 0's {T} rows differ from the B=1 call; "
                                      f"first at query {int(torch.nonzero(~same)[0])}")
            assert torch.isfinite(got.float()).all()
    assert len(routes) >= (2 if T > 128 else 1)


@pytest.mark.parametrize("label,B,T,H,dh,bk,bv,causal", A.REJECTED, ids=[r[0] for r in A.REJECTED])
def test_unsupported_calls_return_minus_one_and_leave_the_output_alone(label, B, T, H, dh, bk, bv, causal):
    """Buffers have the size the refused call would have needed, so that a refusal that failed would still stay in bounds."""
    rows, D = max(B, 1) * max(T, 1), max(H, 1) * dh
    qkv = torch.ones(rows, 3 * D, dtype=torch.bfloat16)
    bias = lambda given: torch.ones(D) if given else None
    rc, out = call(qkv, B, T, H, dh, bias(bk), bias(bv), causal)
    assert rc == -1, f"{label}: status {rc}"
    assert bool(torch.isnan(out.float()).all()), f"{label}: a refused call wrote to the output"
