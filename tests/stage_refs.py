"""Plain references of the tower stages that are neither a GEMM nor the attention core, one function per stage, written from
the comment above each kernel in hippomm_amd/csrc/encoder_ops.hip and attention.hip.  Nothing here comes from hippomm_amd/.

torch float64 on the CPU throughout.  A result is rounded to bf16 (round to nearest even, ``Tensor.to(torch.bfloat16)``) only
where the stage's contract says its output is bf16, and to fp32 only where the contract says "one fp32 add"; the kernels'
internal fp32 is not modelled anywhere else.

Every eps, index rule and reduction is a keyword argument with the contract's value as the default, so that a wrong stage
(tests/test_cpu_stage_refs.py) is the same function with one argument changed.
"""
import math

import torch

F64 = torch.float64


def to_bf16(t):
    """Round to nearest even.  Through fp32 first: exact for everything rounded here except the float64 LayerNorm / attention
    values, where the double rounding moves a result by less than 2^-24 of itself."""
    return t.to(torch.float32).to(torch.bfloat16)


def layernorm(x, gamma, beta, eps):
    """Rows of x: (x - mean) / sqrt(biased variance + eps) * gamma + beta, float64."""
    x = x.to(F64)
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


# ---- exact stages -------------------------------------------------------------------------------------------------------
def im2col_vision(frames, order=("c", "dy", "dx"), zero_columns=(), patch_shift=0):
    """frames (B,3,224,224) -> bf16 [B*256][640]: row b*256 + py*16 + px, column c*196 + dy*14 + dx = pixel
    (c, py*14 + dy, px*14 + dx); columns 588..639 are 0."""
    B = frames.shape[0]
    t = frames.reshape(B, 3, 16, 14, 16, 14)                          # b c py dy px dx
    axes = {"c": 1, "dy": 3, "dx": 5}
    cols = t.permute(0, 2, 4, *(axes[a] for a in order)).reshape(B * 256, 588)
    cols = torch.roll(cols, patch_shift, dims=0)
    out = torch.zeros(B * 256, 640, dtype=frames.dtype)
    out[:, :588] = cols
    for k in zero_columns:
        out[:, k] = 0
    return to_bf16(out)


def im2col_audio(mels, order=("dy", "dx"), stride=10, patch_shift=0):
    """mels (N,128,204) -> bf16 [N*228][256]: row n*228 + py*19 + px (py < 12, px < 19), column dy*16 + dx = mel
    (py*stride + dy, px*stride + dx) with stride 10."""
    N = mels.shape[0]
    rows = []
    for py in range(12):
        for px in range(19):
            tile = mels[:, py * stride: py * stride + 16, px * stride: px * stride + 16]     # n dy dx
            rows.append(tile if order == ("dy", "dx") else tile.transpose(1, 2))
    cols = torch.stack(rows, dim=1).reshape(N * 228, 256)
    return to_bf16(torch.roll(cols, patch_shift, dims=0))


def fold_conv3d(w, taps=(0, 1)):
    """w (D,3,2,14,14) fp32 -> bf16 [D][640]: bf16(w[:, :, 0] + w[:, :, 1]) with the sum taken in fp32, pad columns 0."""
    D = w.shape[0]
    s = (w[:, :, taps[0]].to(torch.float32) + w[:, :, taps[1]].to(torch.float32)).reshape(D, 588)
    out = torch.zeros(D, 640, dtype=torch.float32)
    out[:, :588] = s
    return to_bf16(out)


def embed_tokens(ids, table, pos, T, lo=0, hi=None, pos_shift=0):
    """Row r = table[clamp(ids[r], lo, hi)] + pos[r % T] as ONE fp32 add; hi = vocab - 1."""
    hi = table.shape[0] - 1 if hi is None else hi
    idx = ids.reshape(-1).clamp(lo, hi)
    t = (torch.arange(idx.numel()) % T + pos_shift) % T
    return table.to(torch.float32)[idx] + pos.to(torch.float32)[t]


def gather_rows(src_bytes, stride, n_rows, row_bytes, row_shift=0):
    """dst[r] = src[r * stride .. + row_bytes) as bytes (src_bytes: a flat uint8 tensor)."""
    return torch.stack([src_bytes[(r + row_shift) * stride: (r + row_shift) * stride + row_bytes] for r in range(n_rows)])


# ---- stages compared in value -------------------------------------------------------------------------------------------
def assemble_tokens(patches, cls, pos, stem, pre, n_img, T, dtype=F64, cls_takes_stem=False, pos_shift=0, patch_shift=0):
    """x[b*T + t] = pre_ln((t == 0 ? cls : stem_ln(patches[b*(T-1) + t-1])) + pos[t]).  stem / pre: (gamma, beta, eps) or None.
    dtype: float64 is the reference; float32 is the same function as the error yardstick of the fp32 output."""
    D = cls.numel()
    p = torch.roll(patches.to(dtype), patch_shift, dims=0).reshape(n_img, T - 1, D)
    c = cls.to(dtype).reshape(1, 1, D).expand(n_img, 1, D)
    if stem is not None:
        p = _ln(p, stem, dtype)
        if cls_takes_stem:
            c = _ln(c, stem, dtype)
    x = torch.cat([c, p], dim=1) + torch.roll(pos.to(dtype), pos_shift, dims=0).reshape(1, T, D)
    if pre is not None:
        x = _ln(x, pre, dtype)
    return x.reshape(n_img * T, D)


def _ln(x, gbe, dtype):
    g, b, eps = gbe
    if dtype == F64:
        return layernorm(x, g, b, eps)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g.to(dtype), b.to(dtype), eps)


def eos_position(ids_row, pick="first"):
    """The first position of the largest id."""
    where = torch.nonzero(ids_row == ids_row.max()).flatten()
    return int(where[0] if pick == "first" else where[-1])


def layernorm_eos(x, ids, gamma, beta, eps, pick="first"):
    """y[b] = LN(x[b*T + eos(b)]), float64 (the contract's output is its bf16 rounding).  x (B*T, D), ids (B, T)."""
    B, T = ids.shape
    rows = torch.stack([x[b * T + eos_position(ids[b], pick)] for b in range(B)])
    return layernorm(rows, gamma, beta, eps)


def attention_cls(q_cls, kv, B, T, H, dh, bias_k=None, bias_v=None, keys=None, use_bias_v=True):
    """One query per (sample, head): out[b] = softmax(q k^T / sqrt(dh)) v over the sample's T keys plus, with bias_k / bias_v
    (rounded to bf16, the contract), one appended position.  q_cls (B, D), kv (B*T, 2D) = [k | v]; float64.
    keys: how many of the Lk positions take part (default all)."""
    D = H * dh
    q = q_cls.to(F64).reshape(B, H, 1, dh)
    k = kv.to(F64)[:, :D].reshape(B, T, H, dh).permute(0, 2, 1, 3)
    v = kv.to(F64)[:, D:].reshape(B, T, H, dh).permute(0, 2, 1, 3)
    if bias_k is not None:
        bk = to_bf16(bias_k).to(F64).reshape(1, H, 1, dh).expand(B, H, 1, dh)
        bv = to_bf16(bias_v).to(F64).reshape(1, H, 1, dh).expand(B, H, 1, dh)
        if not use_bias_v:
            bv = torch.zeros_like(bv)
        k, v = torch.cat([k, bk], dim=2), torch.cat([v, bv], dim=2)
    if keys is not None:
        k, v = k[:, :, :keys], v[:, :, :keys]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    return (torch.softmax(s, dim=-1) @ v).reshape(B, D)


def l2norm_rows(v, n_out, clips, log_scale=None, dtype=F64, clamp=100.0, floor=1e-12, mean_first=False):
    """out[i] = mean over the clips of scale * v / max(||v||, floor), each clip normalised FIRST; scale = min(exp(log_scale),
    clamp) or 1 without a log_scale.  A NaN in a clip makes its norm, and so the whole output row, NaN (as torch's normalize)."""
    x = v.to(dtype).reshape(n_out, clips, -1)
    scale = 1.0 if log_scale is None else min(math.exp(float(log_scale)), clamp)

    def unit(t):
        return t / t.norm(dim=-1, keepdim=True).clamp_min(floor)
    if mean_first:
        return unit(x.mean(dim=1)) * scale
    return (unit(x) * scale).mean(dim=1)
