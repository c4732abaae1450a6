"""GPU parity of every tower stage that is neither a GEMM nor the attention core, each kernel called on its own
(hmm_op_* entry points of encoder_ops.hip and attention.hip) against the plain float64 references of tests/stage_refs.py.

Inputs and comparisons live in tests/stage_cases.py; tests/test_cpu_stage_refs.py proves without a GPU that these same
comparisons on these same inputs reject a subtly wrong stage.  Exact stages (the two im2col kernels, the Conv3d fold, the text
embedding, the row gather) are compared bit for bit; LayerNorm-EOS and the one-query attention with the bf16 tolerance of
tests/test_gpu_ops.py; the fp32 outputs (token assembly, L2 normalise) against 4x the error of float32 torch on the same case.
Every output buffer carries NaN canary rows behind its end.

Not covered: select_eos_kernel and gather_selected_rows_kernel.  They run only in the probe build (g_enc_text_head_fused = 0),
are not exported, and nothing under tests/ loads the probe library; layernorm_eos_bf16_kernel replaces both in the product.
"""
import pytest
import torch

import stage_cases as S

pytestmark = pytest.mark.gpu

CANARY = 3       # NaN rows behind every output


def _lib():
    from hippomm_amd import _lib as L
    return L, L.load()


def _out(rows, width, dtype):
    """rows x width of `dtype` followed by CANARY rows, all NaN (0xFF bytes for a byte buffer)."""
    if dtype == torch.uint8:
        return torch.full((rows + CANARY, width), 0xFF, dtype=dtype, device="cuda")
    return torch.full((rows + CANARY, width), float("nan"), dtype=dtype, device="cuda")


def _take(out, rows):
    """The kernel's rows on the CPU, after checking that the canaries survived."""
    tail = out[rows:]
    intact = (tail == 0xFF).all() if out.dtype == torch.uint8 else torch.isnan(tail.float()).all()
    assert bool(intact), "rows past the end of the output were written"
    return out[:rows].cpu()


def _p(t):
    return None if t is None else t.data_ptr()


def run(stage, c):
    """One call of the stage's entry point on the case's inputs -> the output on the CPU (canaries checked)."""
    L, lib = _lib()
    st = L.stream_ptr()
    dev = lambda t: None if t is None else t.cuda()
    if stage == "im2col_vision":
        x, out = dev(c.frames), _out(c.n * 256, 640, torch.bfloat16)
        L.check(lib.hmm_op_im2col_vision_bf16(_p(x), _p(out), c.n, st), stage)
        return _take(out, c.n * 256)
    if stage == "im2col_audio":
        x, out = dev(c.mels), _out(c.n * 228, 256, torch.bfloat16)
        L.check(lib.hmm_op_im2col_audio_bf16(_p(x), _p(out), c.n, st), stage)
        return _take(out, c.n * 228)
    if stage == "fold_conv3d":
        w, out = dev(c.w), _out(c.D, 640, torch.bfloat16)
        L.check(lib.hmm_op_fold_conv3d_bf16(_p(w), _p(out), c.D, st), stage)
        return _take(out, c.D)
    if stage == "embed_tokens":
        ids, table, pos, out = dev(c.ids), dev(c.table), dev(c.pos), _out(c.n_rows, 1024, torch.float32)
        L.check(lib.hmm_op_embed_tokens(_p(ids), _p(table), _p(pos), _p(out), c.n_rows, c.T, c.vocab, st), stage)
        return _take(out, c.n_rows)
    if stage == "gather_rows":
        src, out = dev(c.src), _out(c.n_rows, c.row_bytes, torch.uint8)
        L.check(lib.hmm_op_gather_rows(_p(src), c.stride, _p(out), c.n_rows, c.row_bytes, st), stage)
        return _take(out, c.n_rows)
    if stage == "assemble_tokens":
        patches, cls, pos, out = dev(c.patches), dev(c.cls), dev(c.pos), _out(c.n_img * c.T, c.D, torch.float32)
        sg, sb, se = (dev(c.stem[0]), dev(c.stem[1]), c.stem[2]) if c.stem else (None, None, 0.0)
        pg, pb, pe = (dev(c.pre[0]), dev(c.pre[1]), c.pre[2]) if c.pre else (None, None, 0.0)
        L.check(lib.hmm_op_assemble_tokens(_p(patches), _p(cls), _p(pos), _p(sg), _p(sb), se, _p(pg), _p(pb), pe, _p(out),
                                           c.n_img, c.T, c.D, st), stage)
        return _take(out, c.n_img * c.T)
    if stage == "layernorm_eos":
        x, ids, g, b, out = dev(c.x), dev(c.ids), dev(c.gamma), dev(c.beta), _out(c.B, c.D, torch.bfloat16)
        L.check(lib.hmm_op_layernorm_eos_bf16(_p(x), _p(ids), c.T, _p(g), _p(b), _p(out), c.B, c.D, S.LN_EPS, st), stage)
        return _take(out, c.B)
    if stage == "attention_cls":
        q, kv, bk, bv, out = dev(c.q), dev(c.kv), dev(c.bk), dev(c.bv), _out(c.B, c.H * c.dh, torch.bfloat16)
        L.check(lib.hmm_op_attention_cls_bf16(_p(q), _p(kv), _p(out), c.B, c.T, c.H, c.dh, _p(bk), _p(bv), st), stage)
        return _take(out, c.B)
    if stage == "l2norm_rows":
        v, ls, out = dev(c.v), dev(c.log_scale), _out(c.n_out, 1024, torch.float32)
        L.check(lib.hmm_op_l2norm_rows(_p(v), _p(out), c.n_out, c.clips, _p(ls), st), stage)
        return _take(out, c.n_out)
    raise KeyError(stage)


def _all(stage):
    return pytest.mark.parametrize("case", S.cases(stage), ids=S.case_ids(stage))


@_all("im2col_vision")
def test_im2col_vision(case):
    got = run("im2col_vision", case)
    assert (got[:, 588:].float() == 0).all(), "pad columns 588..639 are not zero"
    S.check("im2col_vision", case, got)


@_all("im2col_audio")
def test_im2col_audio(case):
    got = run("im2col_audio", case)
    assert torch.isfinite(got.float()).all(), "a mel row >= 126 or column >= 196 (NaN here) reached the output"
    S.check("im2col_audio", case, got)


@_all("fold_conv3d")
def test_fold_conv3d(case):
    S.check("fold_conv3d", case, run("fold_conv3d", case))


@_all("embed_tokens")
def test_embed_tokens(case):
    S.check("embed_tokens", case, run("embed_tokens", case))


@_all("gather_rows")
def test_gather_rows(case):
    S.check("gather_rows", case, run("gather_rows", case))


@_all("assemble_tokens")
def test_assemble_tokens(case):
    import stage_refs as R
    got = run("assemble_tokens", case)
    err, _ = S.f32_error(got, case.want)
    print(f"assemble {case.label}: error {float(err.max()):.3e}  float32-torch yardstick {case.yardstick:.3e}")
    S.check("assemble_tokens", case, got)
    # the cls rows on their own: no stem LayerNorm, pos[0], and the pre-LayerNorm
    cls = (case.cls + case.pos[0]).to(torch.float64)
    if case.pre:
        cls = R.layernorm(cls, *case.pre)
    rows = torch.arange(case.n_img) * case.T
    S.check_f32(got[rows], cls.expand(case.n_img, -1), case.yardstick)


@_all("layernorm_eos")
def test_layernorm_eos(case):
    """The value against the reference, and the kernel comment's promise: the bits of hmm_op_layernorm_bf16 on the selected row."""
    import stage_refs as R
    L, lib = _lib()
    got = run("layernorm_eos", case)
    S.check("layernorm_eos", case, got)
    rows = torch.stack([case.x[b * case.T + R.eos_position(case.ids[b])] for b in range(case.B)]).cuda()
    g, b = case.gamma.cuda(), case.beta.cuda()
    y = torch.empty(case.B, case.D, dtype=torch.bfloat16, device="cuda")
    L.check(lib.hmm_op_layernorm_bf16(rows.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), case.B, case.D, S.LN_EPS, L.stream_ptr()), "layernorm")
    S.check_exact(got, y.cpu())


@_all("attention_cls")
def test_attention_cls(case):
    S.check("attention_cls", case, run("attention_cls", case))


@pytest.mark.parametrize("case", [c for c in S.cases("attention_cls") if not c.exact and c.T + (c.bk is not None) <= (288 if c.dh == 80 else 256)],
                         ids=lambda c: c.label)
def test_attention_cls_against_row_0_of_the_full_kernel(case):
    """Cross-check with hmm_op_attention_bf16 on the packed [q | k | v] form of the same q, k, v (query rows other than token 0
    are zero), where the full kernel takes the shape (80 x <= 288 keys, 64 x <= 256 keys).  The full kernel rounds P to bf16 and
    this one does not, so bit-equality is not expected.  test_attention's tolerance formula bounds a bf16-ROUNDED output against
    an unrounded reference; two rounded outputs that each meet it can lie a whole bf16 ulp apart.  So both kernels are held to
    the same float64 reference: the full kernel's row 0 with that formula, this kernel with the tighter bf16 tolerance of
    test_attention_cls -- which bounds their distance by the sum, and shows that the reference and the [k | v] layout here are
    the ones the independently tested kernel computes.  The distance itself is printed."""
    L, lib = _lib()
    c = case
    D = c.H * c.dh
    qkv = torch.zeros(c.B, c.T, 3 * D, dtype=torch.bfloat16)
    qkv[:, 0, :D] = c.q
    qkv[:, :, D:] = c.kv.reshape(c.B, c.T, 2 * D)
    qd, bk, bv = qkv.cuda(), (c.bk.cuda() if c.bk is not None else None), (c.bv.cuda() if c.bv is not None else None)
    full = torch.empty(c.B * c.T, D, dtype=torch.bfloat16, device="cuda")
    L.check(lib.hmm_op_attention_bf16(qd.data_ptr(), full.data_ptr(), c.B, c.T, c.H, c.dh, _p(bk), _p(bv), L.stream_ptr()), "attention")
    one = run("attention_cls", c)
    row0 = full.reshape(c.B, c.T, D)[:, 0].float().cpu()
    want = c.want.float()
    tol = 2.0 ** -8 * want.abs() + 2.0 ** -8 * c.scale + 1e-4
    print(f"attention_cls {c.label}: full kernel row 0 off the reference by {float(((row0 - want).abs() / tol).max()):.2f} of its tolerance, "
          f"the two kernels apart by {float(((one.float() - row0).abs() / tol).max()):.2f} of it")
    S.check("attention_cls", c, one)
    bad = (row0 - want).abs() > tol
    assert not bad.any(), f"{int(bad.sum())}/{bad.numel()} off; worst {float((row0 - want).abs().max()):.4g}"


@_all("l2norm_rows")
def test_l2norm_rows(case):
    got = run("l2norm_rows", case)
    err, _ = S.f32_error(got, case.want)
    print(f"l2norm {case.label}: error {float(err.max()):.3e}  float32-torch yardstick {case.yardstick:.3e}")
    S.check("l2norm_rows", case, got)
    if case.n_out == 5:
        assert (got[1] == 0).all(), "an all-zero row must give 0, not NaN"
        assert torch.isfinite(got[:4]).all() and torch.isnan(got[4]).all(), "the NaN left its own output row, or did not fill it"


@pytest.mark.parametrize("D", [768, 1024, 1280])
def test_layernorm_strided_has_the_bits_of_the_dense_kernel_on_the_gathered_rows(D):
    """The form the fused path uses for token 0 of every image: rows T*D floats apart.  The source ends with the last row read."""
    L, lib = _lib()
    rows, T = 5, 7
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(rows * T, D, generator=g) * 3 + 0.7).reshape(-1)[: ((rows - 1) * T + 1) * D].cuda()
    gamma, beta = (1 + 0.2 * torch.randn(D, generator=g)).cuda(), (0.3 * torch.randn(D, generator=g)).cuda()
    y = _out(rows, D, torch.bfloat16)
    L.check(lib.hmm_op_layernorm_strided_bf16(x.data_ptr(), T * D, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), rows, D, 1e-6,
                                              L.stream_ptr()), "layernorm_strided")
    dense_in = torch.stack([x[r * T * D: r * T * D + D] for r in range(rows)]).contiguous()
    dense = torch.empty(rows, D, dtype=torch.bfloat16, device="cuda")
    L.check(lib.hmm_op_layernorm_bf16(dense_in.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dense.data_ptr(), rows, D, 1e-6,
                                      L.stream_ptr()), "layernorm")
    S.check_exact(_take(y, rows), dense.cpu())


def test_layernorm_non_temporal_path_has_the_bits_of_the_plain_one():
    """launch_layernorm_bf16 reads with non-temporal loads from 4096 rows on: rows 0..4094 of a 4096-row call equal a 4095-row call."""
    L, lib = _lib()
    D = 1280
    g = torch.Generator(device="cuda").manual_seed(4096)
    x = torch.randn(4096, D, device="cuda", generator=g) * 3 + 0.7
    gamma, beta = 1 + 0.2 * torch.randn(D, device="cuda", generator=g), 0.3 * torch.randn(D, device="cuda", generator=g)
    outs = []
    for rows in (4096, 4095):
        y = _out(rows, D, torch.bfloat16)
        L.check(lib.hmm_op_layernorm_bf16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), rows, D, 1e-6, L.stream_ptr()), "layernorm")
        outs.append(_take(y, rows))
    S.check_exact(outs[0][:4095], outs[1])
