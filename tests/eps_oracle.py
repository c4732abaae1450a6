"""The tower forwards of oracle/imagebind_oracle.py with every LayerNorm eps as a parameter (test infrastructure).

encoder.hip passes the eps values as literals at its call sites (stem 1e-5, every other site 1e-6), so an op-level test cannot
see a wrong one.  This copy of the oracle's forward takes ``eps = {site: value}`` for the sites below; with ``EPS`` it computes
what the oracle computes (tests/test_cpu_stage_refs.py asserts that), with one value changed it is the tower with a wrong
literal.  ``small_signal_cases()`` are the inputs at which such a change moves the embedding far outside the end-to-end
tolerance of tests/test_gpu_encoder.py; the GPU tests there run the real tower on them against the unmodified oracle.
"""
import torch
import torch.nn.functional as F

from oracle import imagebind_oracle as ib

SITES = ("stem", "pre", "norm_1", "norm_2", "head")
EPS = {"stem": 1e-5, "pre": 1e-6, "norm_1": 1e-6, "norm_2": 1e-6, "head": 1e-6}


def _block(x, st, prefix, spec, eps, i, attn_mask=None):
    D = spec.embed_dim
    eps = {site: eps.get(f"{site}.{i}", eps[site]) for site in ("norm_1", "norm_2")}      # "norm_1.0": that block alone
    y = F.layer_norm(x, (D,), st[prefix + "norm_1.weight"], st[prefix + "norm_1.bias"], eps["norm_1"])
    attn, _ = F.multi_head_attention_forward(
        y, y, y, D, spec.heads, st[prefix + "attn.in_proj_weight"], st[prefix + "attn.in_proj_bias"],
        st.get(prefix + "attn.bias_k"), st.get(prefix + "attn.bias_v"), False, 0.0,
        st[prefix + "attn.out_proj.weight"], st[prefix + "attn.out_proj.bias"], training=False, need_weights=False, attn_mask=attn_mask)
    x = x + attn
    y = F.layer_norm(x, (D,), st[prefix + "norm_2.weight"], st[prefix + "norm_2.bias"], eps["norm_2"])
    y = F.linear(F.gelu(F.linear(y, st[prefix + "mlp.fc1.weight"], st[prefix + "mlp.fc1.bias"])), st[prefix + "mlp.fc2.weight"],
                 st[prefix + "mlp.fc2.bias"])
    return x + y


@torch.no_grad()
def forward(name, x, st, spec, eps=EPS):
    """'vision' (B,3,224,224) / 'audio' (B,S,1,128,204) / 'text' (B,77) int64 -> what ib.forward gives when eps == EPS."""
    D = spec.embed_dim
    pp, tr, hd = f"modality_preprocessors.{name}.", f"modality_trunks.{name}.", f"modality_heads.{name}."
    mask = None
    if name == "text":
        t = F.embedding(x, st[pp + "token_embedding.weight"]) + st[pp + "pos_embed"]
        mask = torch.full((spec.tokens, spec.tokens), float("-inf")).triu_(1)
    else:
        if name == "vision":
            video = x.float().unsqueeze(2).repeat(1, 1, 2, 1, 1)
            p = F.conv3d(video, st[pp + "rgbt_stem.proj.1.weight"], stride=(2, 14, 14)).flatten(2).transpose(1, 2)
        else:
            clips = x.float().reshape(-1, *x.shape[2:])
            p = F.conv2d(clips, st[pp + "rgbt_stem.proj.weight"], stride=10).flatten(2).transpose(1, 2)
            p = F.layer_norm(p, (D,), st[pp + "rgbt_stem.norm_layer.weight"], st[pp + "rgbt_stem.norm_layer.bias"], eps["stem"])
        t = torch.cat([st[pp + "cls_token"].expand(p.shape[0], -1, -1), p], dim=1) + st[pp + "pos_embedding_helper.pos_embed"]
        if spec.pre_ln:
            t = F.layer_norm(t, (D,), st[tr + "pre_transformer_layer.0.weight"], st[tr + "pre_transformer_layer.0.bias"], eps["pre"])
    t = t.transpose(0, 1)
    for i in range(spec.depth):
        t = _block(t, st, f"{tr}blocks.{i}.", spec, eps, i, mask)
    t = t.transpose(0, 1)
    if name == "text":
        y = t[torch.arange(t.shape[0]), x.argmax(dim=-1)]
        y = F.layer_norm(y, (D,), st[hd + "proj.0.weight"], st[hd + "proj.0.bias"], eps["head"])
        y = F.normalize(F.linear(y, st[hd + "proj.1.weight"]), dim=-1)
        return y * st["modality_postprocessors.text.1.log_logit_scale"].exp().clamp(max=100.0)
    y = F.layer_norm(t[:, 0], (D,), st[hd + "0.weight"], st[hd + "0.bias"], eps["head"])
    y = F.normalize(F.linear(y, st[hd + "2.weight"]), dim=-1)
    if name == "audio":
        y = (y * st["modality_postprocessors.audio.1.log_logit_scale"].exp().clamp(max=100.0)).reshape(x.shape[0], x.shape[1], -1).mean(dim=1)
    return y


# ---- the inputs at which each literal matters ---------------------------------------------------------------------------
WRONG = {"stem": 1e-6, "pre": 1e-5, "norm_1": 1e-5, "norm_2": 1e-5, "head": 1e-5}      # the other eps of the code base
TOL_SCALE = {"vision": 1.0, "audio": 20.0, "text": 1.0 / 0.07}                          # as tests/test_gpu_encoder.py
SMALL_SIGNAL = ("vision_pre", "audio_stem", "audio_block0", "vision_small", "audio_small", "text_small")


def _scaled(st, suffixes, factor):
    return {k: (v * factor if k.endswith(suffixes) else v) for k, v in st.items()}


def _small_state(name, spec, seed):
    """A residual stream of size 1e-3 (variance near 1e-6) at EVERY LayerNorm of the blocks and at the head: weights of std 1e-3,
    the Linear biases and bias_k / bias_v brought from 0.02 / 0.5 down to that size, and the affine of the LayerNorm that
    feeds the stream (pre-LN, stem LN) or the embeddings (text) scaled to 1e-3.  gamma / beta of the other LayerNorms stay rich:
    a uniform rescaling of a LayerNorm's normalised part against its beta changes the direction of the embedding."""
    st = ib.synthetic_state(spec, seed=seed, init="rich", w_std=1e-3)
    st = _scaled(st, ("in_proj_bias", "out_proj.bias", "fc1.bias", "fc2.bias"), 0.05)
    st = _scaled(st, ("bias_k", "bias_v"), 2e-3)
    if name == "vision":
        st = _scaled(st, ("pre_transformer_layer.0.weight", "pre_transformer_layer.0.bias"), 1e-3)
    elif name == "audio":
        st = _scaled(st, ("norm_layer.weight", "norm_layer.bias"), 1e-3)
    else:
        st = _scaled(st, ("pos_embed",), 0.1)                       # 0.01 -> 1e-3, the size of the token table at w_std 1e-3
    return st


def small_signal_case(label):
    """-> (tower name, spec, state, input, the sites whose eps the case pins).  Seeded; depth 2."""
    g = torch.Generator().manual_seed(len(label))
    name = label.split("_")[0]
    spec = ib.reduced({"vision": ib.VISION_HUGE, "audio": ib.AUDIO_HUGE, "text": ib.TEXT_HUGE}[name], 2)
    if name == "vision":
        x = torch.randn(2, 3, 224, 224, generator=g)
    elif name == "audio":
        x = torch.randn(2, 3, 1, 128, 204, generator=g)
    else:
        x = torch.randint(1, 49000, (3, 77), generator=g)
        for b, n in enumerate([5, 40, 76]):                        # EOS (the largest id) at various positions, zero padding after
            x[b, n] = 49407
            x[b, n + 1:] = 0
    if label == "vision_pre":                                       # the stem's output has variance near 1e-6 in front of the pre-LN
        return name, spec, ib.synthetic_state(spec, seed=1234, init="rich", w_std=1e-3), x, ("pre",)
    if label == "audio_stem":                                       # mel x 1e-2: patch rows of variance near 1e-5 in front of the stem LN
        return name, spec, ib.synthetic_state(spec, seed=4321, init="rich"), x * 1e-2, ("stem",)
    if label == "audio_block0":                                     # ordinary weights, but tokens of size 1e-3 in front of block 0 (audio_small
        st = ib.synthetic_state(spec, seed=4321, init="rich")       # does not move with that block's norm_1: 1.0 x the tolerance)
        return name, spec, _scaled(st, ("norm_layer.weight", "norm_layer.bias", "cls_token", "pos_embed"), 1e-3), x, ("norm_1.0",)
    sites = {"vision": ("pre", "norm_1.0"), "audio": (), "text": ("norm_1.0",)}[name] + ("norm_1.1", "norm_2.0", "norm_2.1", "head")
    return name, spec, _small_state(name, spec, 99), x, sites


def wrong_eps(site):
    eps = dict(EPS)
    eps[site] = WRONG[site.split(".")[0]]
    return eps
