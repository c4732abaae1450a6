"""GPU: the fused in_proj + attention kernels (hmm_op_qkv_attention_bf16, hmm_op_qkv_attention_audio_bf16) against the exact
float64 reference of tests/fused_attention_cases.py, where the inputs, the lift and the mutants live;
tests/test_cpu_fused_attention_cases.py proves without a GPU that the same comparison on the same inputs rejects a kernel that
drops a bias, mixes up heads, images, the cls row or the stored rows, or loses a key.

test_fused_qkv_attention_equals_gemm_plus_attention (tests/test_gpu_ops.py) compares the fused kernel with the project's own two
kernels on Gaussian operands; here the images the kernel must hold are known exactly, so the reference owes nothing to either,
and the two-kernel route is checked against the same images on the way (an exact check of the GEMM's bias epilogue).  Every
output buffer is filled with NaN and carries one guard row behind its end.
"""
import functools

import pytest
import torch

import attention_cases as A
import fused_attention_cases as F

pytestmark = pytest.mark.gpu
EPI_BIAS_BF16 = 0


def _lib():
    from hippomm_amd import _lib as L
    return L, L.load()


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same(x, y):
    return x.shape == y.shape and torch.equal(x.view(torch.int16), y.view(torch.int16))


def fused(c, n=None, a=None):
    """One fused call on CPU inputs -> (status, the n*T output rows on the CPU, still bf16).  The output starts as NaN; the guard
    row behind it must keep its bits.  ``c`` has name, T, D, a, w, in_bias, bk, bv and (vision) qkv_cls."""
    L, lib = _lib()
    n = c.B if n is None else n
    rows = max(n, 1) * c.T
    out = torch.full((rows + 1, c.D), float("nan"), dtype=torch.bfloat16, device="cuda")
    before = out[rows:].clone()
    ad, wd, bd = (c.a if a is None else a).cuda(), c.w.cuda(), c.in_bias.cuda()
    if c.name == "vision":
        cls = c.qkv_cls.cuda()
        rc = lib.hmm_op_qkv_attention_bf16(ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), cls.data_ptr(), out.data_ptr(), n, L.stream_ptr())
    else:
        bkd, bvd = c.bk.cuda(), c.bv.cuda()
        rc = lib.hmm_op_qkv_attention_audio_bf16(ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), bkd.data_ptr(), bvd.data_ptr(), out.data_ptr(),
                                                 n, L.stream_ptr())
    torch.cuda.synchronize()
    assert _same(out[rows:], before), "the row behind the output was written"
    return rc, out[:rows].cpu()


def run(c):
    """The fused kernel's output for a case of the table."""
    L, _ = _lib()
    rc, got = fused(c)
    L.check(rc, "qkv_attention")
    return got


def two_kernels(c):
    """The route the fused kernel replaces, on the same operands: (qkv, qkv_cls or None, attention output), on the CPU."""
    L, lib = _lib()
    n, T, D = c.B, c.T, c.D
    ad, wd, bd = c.a.cuda(), c.w.cuda(), c.in_bias.cuda()
    qkv = torch.full((n * T, 3 * D), float("nan"), dtype=torch.bfloat16, device="cuda")
    L.check(lib.hmm_op_gemm_bf16(ad.data_ptr(), wd.data_ptr(), bd.data_ptr(), qkv.data_ptr(), n * T, 3 * D, D, EPI_BIAS_BF16, L.stream_ptr()), "gemm")
    qkv_cls = None
    if c.name == "vision":                                                           # the small cls GEMM of the fused route
        cls_rows = ad.view(n, T, D)[:, 0].contiguous()
        qkv_cls = torch.full((n, 3 * D), float("nan"), dtype=torch.bfloat16, device="cuda")
        L.check(lib.hmm_op_gemm_bf16(cls_rows.data_ptr(), wd.data_ptr(), bd.data_ptr(), qkv_cls.data_ptr(), n, 3 * D, D, EPI_BIAS_BF16,
                                     L.stream_ptr()), "gemm cls")
    bkd, bvd = (None, None) if c.bk is None else (c.bk.cuda(), c.bv.cuda())
    out = torch.full((n * T, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    L.check(lib.hmm_op_attention_bf16(qkv.data_ptr(), out.data_ptr(), n, T, c.H, c.dh, None if bkd is None else bkd.data_ptr(),
                                      None if bvd is None else bvd.data_ptr(), L.stream_ptr()), "attention")
    torch.cuda.synchronize()
    return qkv.cpu(), (None if qkv_cls is None else qkv_cls.cpu()), out.cpu()


def _rows_off(x, y):
    bad = (x.view(torch.int16) != y.view(torch.int16)).any(dim=1)
    return f"{int(bad.sum())} / {bad.numel()} rows differ, first {int(torch.nonzero(bad)[0]) if bad.any() else None}"


def _both_routes(c):
    """The fused output of a case, after the two-kernel route has been held against the same exact images and the fused output
    against the two-kernel one."""
    got = run(c)
    assert torch.isfinite(got.float()).all(), f"{c.label}: NaN left in the output, or an infinity written"
    qkv, qkv_cls, two = two_kernels(c)
    assert _same(qkv, c.qkv), f"{c.label}: the GEMM's qkv is not (P + bias) rounded once: {_rows_off(qkv, c.qkv)}"
    if c.name == "vision":
        assert _same(qkv_cls, c.qkv_cls), f"{c.label}: the cls GEMM's rows are not (P + bias) rounded once: {_rows_off(qkv_cls, c.qkv_cls)}"
    assert _same(got, two), f"{c.label}: fused and two-kernel outputs differ: {_rows_off(got, two)}"
    return got


def _value(c):
    got = _both_routes(c)
    print(f"fused attention {c.label}: worst error {A.ratio(c, got):.3f} of the tolerance")
    A.check(c, got)


@pytest.mark.parametrize("spec", F.specs("value"), ids=F.spec_ids("value"))
def test_values_on_exactly_known_images(spec):
    _value(F.case(spec))


@pytest.mark.parametrize("spec", F.specs("onehot"), ids=F.spec_ids("onehot"))
def test_one_hot_rows_pick_exactly_the_right_value_row(spec):
    c = F.case(spec)
    got = _both_routes(c)
    assert torch.equal(got, c.picked), f"{c.label}: {int((got != c.picked).any(dim=1).sum())} rows are not the picked V row"
    A.check(c, got)


DEAL_SLOTS = [(name, i) for name in F.GEOS for i in range(len(F.DEAL_NAMES[name]))]


@pytest.mark.parametrize("name,slot", DEAL_SLOTS, ids=[f"{name},n={F.DEAL_NAMES[name][i]}" for name, i in DEAL_SLOTS])
def test_values_at_every_deal_of_workgroups(name, slot):
    """Batch sizes around one round of workgroups (one is resident per CU) and, for audio, with both remainders of the
    eight-run deal.  Every image is distinct and has its own reference, so an exchange of two images or heads shows."""
    spec = [s for s in F.specs("deal", _cus()) if s.name == name][slot]
    c = F.case(spec)
    assert c.B == F.deal_sizes(name, _cus())[slot]
    _value(c)


@pytest.mark.parametrize("name", list(F.GEOS))
def test_dense_operands_equal_the_two_kernel_route_beyond_one_round(name):
    """Gaussian a, w and bias, more workgroups than CUs: the K loop with dense operands at the new batch sizes.  Bitwise against
    the two-kernel route only; the exact reference is the business of the other tests."""
    c = F.dense_inputs(name, F.dense_sizes(_cus())[name])
    assert c.B * c.H > _cus()
    qkv, c.qkv_cls, two = two_kernels(c)
    assert torch.isfinite(two.float()).all()
    if name == "vision":
        assert _same(c.qkv_cls, qkv.reshape(c.B, c.T, 3 * c.D)[:, 0]), "small-M GEMM differs from the large one on the cls rows"
    L, _ = _lib()
    rc, got = fused(c)
    L.check(rc, "qkv_attention")
    assert _same(got, two), f"{name}, n={c.B}: {_rows_off(got, two)}"


@pytest.mark.parametrize("name", list(F.GEOS))
def test_image_bits_do_not_depend_on_batch_size_or_position(name):
    """Image 0 of the pool rides alone, then at the first, the middle and the last position of every deal batch size; the
    (sample, head) deal changes with each, the image's rows must keep their bits."""
    L, _ = _lib()
    alone = run(F.batch(name, [0]))
    assert torch.isfinite(alone.float()).all()
    for n in F.deal_sizes(name, _cus())[1:]:
        for position in sorted({0, n // 2, n - 1}):
            c = F.batch(name, F.invariance_order(n, position))
            got = run(c)
            assert torch.isfinite(got.float()).all()
            mine = got.reshape(n, c.T, c.D)[position]
            assert _same(mine, alone), f"{name}, n={n}, position {position}: {_rows_off(mine, alone)} from the n=1 call"


def test_the_cls_row_reaches_the_kernel_through_qkv_cls_alone():
    """qkv_attention.hip: "the cls row (token 0), which does not fit the 256-row tile, comes from a small GEMM over the cls rows
    of all images (qkv_cls, computed by the caller)".  So with row 0 of every image of ``a`` set to NaN and qkv_cls unchanged the
    output keeps its bits.  This documents the present contract and moves with it if the cls projection ever moves into the
    kernel."""
    c = F.case(F.by_label("value", "vision,scale=1"))
    L, _ = _lib()
    want = run(c)
    a = c.a.clone()
    a.reshape(c.B, c.T, c.D)[:, 0] = float("nan")
    rc, got = fused(c, a=a)
    L.check(rc, "qkv_attention")
    assert _same(got, want), _rows_off(got, want)
    A.check(c, got)


@pytest.mark.parametrize("name", list(F.GEOS))
def test_an_empty_batch_is_refused_and_the_output_left_alone(name):
    """Buffers have the size of the n = 1 call, so that a refusal that failed would still stay in bounds."""
    c = F.batch(name, [0])
    rc, out = fused(c, n=0)
    assert rc == -1, f"{name}: status {rc}"
    assert bool(torch.isnan(out.float()).all()), f"{name}: a refused call wrote to the output"
    _, lib = _lib()
    assert b"out of range" in lib.hmm_last_error()
