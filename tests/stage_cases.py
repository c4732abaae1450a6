"""The inputs and the comparison functions of tests/test_gpu_stage_ops.py, kept apart from it so that
tests/test_cpu_stage_refs.py can run WRONG references (mutants of tests/stage_refs.py) through exactly the same inputs and
comparisons without a GPU: a comparison that accepts a mutant would accept a kernel with that mistake.

A case is a plain namespace: the CPU inputs, the arguments, and ``want`` -- the reference result, computed once per process
(``cases(stage)`` is cached) and never modified.  ``check(stage, case, got)`` raises AssertionError when ``got`` (the kernel's
output without its canary rows, or a mutant's result cast to the output type) is not the stage's result.
"""
import functools
import math
from types import SimpleNamespace as NS

import torch

import stage_refs as R
from test_gpu_ops import _close_bf16           # the bf16 tolerance of the op tests, unchanged

F32_FACTOR = 4.0                 # the kernel's fp32 error may be this many times float32 torch's on the same case ...
F32_FLOOR = 8 * 2.0 ** -24       # ... floored at 8 fp32 half-ulps of the row's largest magnitude (torch's fp32 can be exact)
STEM_EPS, PRE_EPS = 1e-5, 1e-6   # as at the call site in encoder.hip; different on purpose
LN_EPS = 1e-6


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- comparisons --------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def check_exact(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    same = _bits(got) == _bits(want)
    assert bool(same.all()), f"{int((~same).sum())} / {same.numel()} elements differ in their bits; first at {torch.nonzero(~same)[0].tolist()}"


def check_bf16(got, want):
    assert got.dtype == torch.bfloat16 and got.shape == want.shape
    assert torch.isfinite(got.float()).all()
    _close_bf16(got, want, extra_atol=1e-5)


def f32_yardstick(want64, want32):
    """Max error of the float32-torch evaluation of the reference against the float64 one (NaN positions aside)."""
    d = (want32.to(torch.float64) - want64).abs()
    return float(torch.nan_to_num(d, nan=0.0).max())


def f32_error(got, want64):
    """(worst |got - want| over the finite positions, per-row tolerance floor); NaN must sit exactly where the reference has it."""
    assert got.dtype == torch.float32 and got.shape == want64.shape
    nan_w, nan_g = torch.isnan(want64), torch.isnan(got)
    assert torch.equal(nan_w, nan_g), f"NaN at {int(nan_g.sum())} positions, the reference has {int(nan_w.sum())}"
    assert torch.isfinite(got[~nan_g]).all()
    err = torch.nan_to_num((got.to(torch.float64) - want64).abs(), nan=0.0)
    floor = F32_FLOOR * torch.nan_to_num(want64.abs(), nan=0.0).max(dim=-1, keepdim=True).values
    return err, floor


def check_f32(got, want64, yardstick):
    err, floor = f32_error(got, want64)
    tol = torch.maximum(torch.full_like(floor, F32_FACTOR * yardstick), floor)
    bad = err > tol
    assert not bad.any(), (f"{int(bad.sum())} / {bad.numel()} off; worst error {float(err.max()):.3e} against a float32-torch "
                           f"yardstick of {yardstick:.3e}")


# ---- cases --------------------------------------------------------------------------------------------------------------
def _im2col_vision():
    out = []
    for n_img in (1, 3):
        c, y, x = torch.meshgrid(torch.arange(3), torch.arange(224), torch.arange(224), indexing="ij")
        img = ((c * 224 * 224 + y * 224 + x) % 251 - 125).float()                  # exact in bf16, distinct along every axis
        frames = torch.stack([img + b for b in range(n_img)])
        out.append(NS(label=f"n_img={n_img}", n=n_img, frames=frames, want=R.im2col_vision(frames)))
    return out


def _im2col_audio():
    out = []
    for n in (1, 3):
        r, c = torch.meshgrid(torch.arange(128), torch.arange(204), indexing="ij")
        mels = torch.stack([((i * 7 + r * 204 + c) % 251 - 125).float() for i in range(n)])
        mels[:, 126:, :] = float("nan")                                              # never read: must not reach the output
        mels[:, :, 196:] = float("nan")
        out.append(NS(label=f"n_clip={n}", n=n, mels=mels, want=R.im2col_audio(mels)))
    return out


def _fold_conv3d():
    g = _gen(11)
    w = torch.randn(5, 3, 2, 14, 14, generator=g)
    w[:, :, 1] *= -3.0                                                               # the taps differ in sign and size
    return [NS(label="D=5", D=5, w=w, want=R.fold_conv3d(w))]


def _embed_tokens():
    out = []
    for batch in (1, 3):
        g = _gen(20 + batch)
        T, vocab = 77, 50
        ids = torch.randint(0, vocab, (batch * T,), generator=g)
        ids[3], ids[10], ids[40], ids[T - 1], ids[0] = -1, vocab, 2 ** 40, 49, 0     # clamp to 0, 49, 49
        ids[batch * T - 2] = -(2 ** 40)
        table, pos = torch.randn(vocab, 1024, generator=g), torch.randn(T, 1024, generator=g)
        out.append(NS(label=f"batch={batch}", ids=ids, table=table, pos=pos, T=T, vocab=vocab, n_rows=batch * T,
                      want=R.embed_tokens(ids, table, pos, T)))
    return out


def _gather_rows():
    out = []
    for row_bytes in (1536, 2560, 5120):
        for T in (229, 257):
            for n_rows in (1, 3, 5):
                stride = T * row_bytes
                g = _gen(row_bytes + T + n_rows)
                # the source ends with the last byte of the last gathered row, not at a whole stride
                src = torch.randint(0, 256, ((n_rows - 1) * stride + row_bytes,), generator=g, dtype=torch.uint8)
                out.append(NS(label=f"row={row_bytes},T={T},n={n_rows}", src=src, stride=stride, n_rows=n_rows, row_bytes=row_bytes,
                              want=R.gather_rows(src, stride, n_rows, row_bytes)))
    return out


def _assemble_tokens():
    out = []
    shapes = [("pre", 257, 1280, False, True, 1.0), ("stem", 229, 768, True, False, 1.0), ("both", 229, 1280, True, True, 1.0),
              ("neither", 257, 768, False, False, 1.0)]
    lows = [("stem,low-variance", 229, 768, True, False, 3e-3), ("pre,low-variance", 257, 1280, False, True, 3e-3),
            ("both,low-variance", 229, 1280, True, True, 3e-3)]
    # n_img 1, 2, 3: 257 / 514 / 771 (229 / 458 / 687) rows, every residue of the four-rows-per-block tail
    for (kind, T, D, has_stem, has_pre, size), n_img in [(s, n) for s in shapes for n in (1, 2, 3)] + [(s, 2) for s in lows]:
        g = _gen(T + D + n_img + len(kind))
        # size 3e-3: rows of variance about 1e-5, the size of the eps values, with a small mean (no cancellation in x - mean)
        patches = (torch.randn(n_img * (T - 1), D, generator=g) + 0.3) * size
        cls, pos = (torch.randn(D, generator=g) - 0.2) * size, torch.randn(T, D, generator=g) * (size if has_pre and size != 1.0 else 0.5)
        vec = lambda base: base + 0.3 * torch.randn(D, generator=g)                  # rich gamma / beta
        stem = (vec(1.0), vec(0.0), STEM_EPS) if has_stem else None
        pre = (vec(1.0), vec(0.0), PRE_EPS) if has_pre else None
        c = NS(label=f"{kind},T={T},D={D},n_img={n_img}", kind=kind, patches=patches, cls=cls, pos=pos, stem=stem, pre=pre,
               n_img=n_img, T=T, D=D)
        c.want = R.assemble_tokens(patches, cls, pos, stem, pre, n_img, T)
        c.yardstick = f32_yardstick(c.want, R.assemble_tokens(patches, cls, pos, stem, pre, n_img, T, dtype=torch.float32))
        out.append(c)
    return out


EOS = 49407


def _eos_ids(T, rows, seed):
    g = _gen(seed)
    ids = torch.randint(1, 1000, (len(rows), T), generator=g)
    for b, at in enumerate(rows):
        if at == "equal":
            ids[b] = 7
        elif at == "negative":
            ids[b] = -torch.randint(5, 1000, (T,), generator=g)
            ids[b, 40], ids[b, 41] = -2, -2                                          # the largest, twice
        else:
            for t in at:
                ids[b, t] = EOS
    return ids


def _layernorm_eos():
    out = []
    main = [(0,), (76,), (70,), (6, 70), (5, 70), "equal"]       # 6 and 70 fall to the same lane (70 = 6 + 64), 5 and 70 do not
    for label, T, D, rows in [("T=77,D=1024", 77, 1024, main), ("T=77,D=1024,odd rows", 77, 1024, ["negative", (33, 34), (76,)]),
                              ("T=1", 1, 1024, [(0,)] * 5), ("T=77,D=768", 77, 768, main), ("T=77,D=1280", 77, 1280, main)]:
        g = _gen(T + D + len(rows))
        B = len(rows)
        ids = _eos_ids(T, rows, T + D)
        x = torch.randn(B * T, D, generator=g) * 3 + 0.7
        gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)
        out.append(NS(label=label, x=x, ids=ids, T=T, D=D, B=B, gamma=gamma, beta=beta,
                      want=R.layernorm_eos(x, ids, gamma, beta, LN_EPS)))
    return out


ATTN_CLS_SHAPES = [(2, 257, 16, 80, False), (3, 229, 12, 64, True), (1, 33, 3, 64, True), (1, 1, 1, 64, False),
                   (1, 320, 2, 64, False), (1, 319, 2, 80, True)]                     # the last two: 320 keys, the limit


def _attention_cls():
    out = []
    for (B, T, H, dh, bias) in ATTN_CLS_SHAPES:
        for scale in (1.0, 6.0):                                                     # 6: a peaky softmax, as test_attention
            D = H * dh
            g = _gen(B * 1000 + T + int(scale))
            q = (torch.randn(B, D, generator=g) * scale).to(torch.bfloat16)
            kv = (torch.randn(B * T, 2 * D, generator=g) * scale).to(torch.bfloat16)
            bk = torch.randn(D, generator=g) * scale if bias else None
            bv = torch.randn(D, generator=g) * scale if bias else None
            # The last key of every (sample, head), and sample 0's bias_k position, point along the query with the score of the
            # best random key of that head, so that they carry weight under the peaky softmax too (a dropped last key or bias_v
            # would otherwise be invisible at scale 6).
            if T > 1:
                qh = q.float().reshape(B, 1, H, dh)
                kh = kv.float().reshape(B, T, 2, H, dh)[:, :T - 1, 0]
                alpha = (qh * kh).sum(-1).max(dim=1).values / (qh * qh).sum(-1).reshape(B, H)      # (B, H): best score / |q|^2
                along = (alpha.reshape(B, H, 1) * qh.reshape(B, H, dh)).reshape(B, D)
                kv.reshape(B, T, 2 * D)[:, T - 1, :D] = along.to(torch.bfloat16)
                if bias:
                    bk = along[0].clone()
            out.append(NS(label=f"B={B},T={T},H={H},dh={dh},bias={bias},scale={scale}", B=B, T=T, H=H, dh=dh, q=q, kv=kv, bk=bk, bv=bv,
                          scale=scale, exact=False, want=R.attention_cls(q, kv, B, T, H, dh, bk, bv)))
    return out + _attention_cls_one_hot()


def _attention_cls_one_hot():
    """Built as test_attention_one_hot_rows_pick_the_right_value: key j lies on axis j % dh with length 1 + j // dh, the query of
    (sample, head) has length 300 along one axis, so that axis' longest key wins by more than 30 nats and the output is exactly
    that key's V row.  (sample 0, head 0) asks for the very last position -- the last key, or the bias_k / bias_v position --
    and (sample 0, head 1) for the last key of the token matrix when there is a bias position behind it."""
    out = []
    for (B, T, H, dh, bias) in [(2, 257, 16, 80, False), (2, 229, 12, 64, True)]:
        D, Lk = H * dh, T + (1 if bias else 0)
        g = _gen(T)
        k = torch.zeros(B, Lk, H, dh)
        for j in range(Lk):
            k[:, j, :, j % dh] = 1.0 + j // dh
        top = {j % dh: j for j in range(Lk)}                                         # the longest key of each axis
        v = torch.randn(B, Lk, H, dh, generator=g).to(torch.bfloat16).float()
        v[:, T:] = v[:1, T:]                                                         # the bias position is shared by the samples
        axis = torch.tensor([[(7 * h + 3 * b + 5) % dh for h in range(H)] for b in range(B)])
        axis[0, 0], axis[0, 1] = (Lk - 1) % dh, (T - 1) % dh
        q = torch.zeros(B, H, dh)
        for b in range(B):
            for h in range(H):
                q[b, h, axis[b, h]] = 300.0
        kv = torch.cat([k[:, :T].reshape(B * T, D), v[:, :T].reshape(B * T, D)], dim=1).to(torch.bfloat16)
        bk = k[0, T].reshape(D) if bias else None
        bv = v[0, T].reshape(D) if bias else None
        picked = torch.stack([torch.stack([v[b, top[int(axis[b, h])], h] for h in range(H)]) for b in range(B)]).reshape(B, D)
        want = R.attention_cls(q.reshape(B, D), kv, B, T, H, dh, bk, bv)
        assert torch.equal(R.to_bf16(want).float(), picked), "the one-hot construction does not select one V row"
        assert top[int(axis[0, 0])] == Lk - 1
        out.append(NS(label=f"one-hot,T={T},H={H},dh={dh},bias={bias}", B=B, T=T, H=H, dh=dh, q=q.reshape(B, D).to(torch.bfloat16), kv=kv,
                      bk=bk, bv=bv, exact=True, want=want))
    return out


def _l2norm_rows():
    out = []
    for n_out in (1, 5):
        for clips in (1, 3):
            for name, log_scale in (("none", None), ("log20", math.log(20.0)), ("log200", math.log(200.0))):   # log 200 clamps to 100
                g = _gen(n_out * 10 + clips)
                v = torch.randn(n_out, clips, 1024, generator=g) * (1.0 + torch.arange(clips).reshape(1, clips, 1))   # clips differ in length
                if n_out == 5:
                    v[1] = 0.0                                                       # all-zero: the output is 0, not NaN
                    v[2] *= 1e-22 / v[2].norm(dim=-1, keepdim=True)                  # below the 1e-12 floor
                    v[3, clips - 1] *= 1e15 / v[3, clips - 1].norm()                 # one huge clip next to ordinary ones
                    v[4, 0, 77] = float("nan")                                       # stays inside output row 4
                v = v.reshape(n_out * clips, 1024)
                ls = None if log_scale is None else torch.tensor([log_scale], dtype=torch.float32)
                c = NS(label=f"n_out={n_out},clips={clips},scale={name}", v=v, n_out=n_out, clips=clips, log_scale=ls)
                c.want = R.l2norm_rows(v, n_out, clips, None if ls is None else float(ls))
                c.yardstick = f32_yardstick(c.want, R.l2norm_rows(v, n_out, clips, None if ls is None else float(ls), dtype=torch.float32))
                out.append(c)
    return out


_BUILDERS = {"im2col_vision": _im2col_vision, "im2col_audio": _im2col_audio, "fold_conv3d": _fold_conv3d, "embed_tokens": _embed_tokens,
             "gather_rows": _gather_rows, "assemble_tokens": _assemble_tokens, "layernorm_eos": _layernorm_eos,
             "attention_cls": _attention_cls, "l2norm_rows": _l2norm_rows}
STAGES = tuple(_BUILDERS)
EXACT = ("im2col_vision", "im2col_audio", "fold_conv3d", "embed_tokens", "gather_rows")


@functools.lru_cache(maxsize=None)
def cases(stage):
    return tuple(_BUILDERS[stage]())


def case_ids(stage):
    """For parametrize: the labels, without computing a reference at collection time where that costs anything."""
    return [c.label for c in cases(stage)]


def out_dtype(stage):
    return {"embed_tokens": torch.float32, "gather_rows": torch.uint8, "assemble_tokens": torch.float32,
            "l2norm_rows": torch.float32}.get(stage, torch.bfloat16)


def cast_result(stage, value):
    """A (mutant) reference result in the stage's output type, as the kernel would deliver it."""
    dt = out_dtype(stage)
    return R.to_bf16(value) if dt == torch.bfloat16 else value.to(dt)


def check(stage, case, got):
    if stage in EXACT:
        check_exact(got, case.want)
    elif stage in ("assemble_tokens", "l2norm_rows"):
        check_f32(got, case.want, case.yardstick)
    elif stage == "attention_cls" and case.exact:
        check_exact(got, R.to_bf16(case.want))
    else:
        check_bf16(got, case.want)
