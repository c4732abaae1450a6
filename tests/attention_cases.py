"""The inputs, the float64 reference and the comparison of tests/test_gpu_attention_edges.py, kept apart from it so that
tests/test_cpu_attention_cases.py can run WRONG references (the same function with one argument changed) through exactly the
same inputs and the same comparison without a GPU.  Nothing here comes from hippomm_amd/.

The table walks the attention core (hippomm_amd/csrc/attention_core.h behind hmm_op_attention_bf16 and
hmm_op_attention_causal_bf16) along every edge its code has: the 32-key tile, the 96-key online-softmax chunk, the 96 / 97 key
switch between the two dh = 64 instantiations, the full LDS images (dh 64 x 256 keys, dh 80 x 288 keys), the cooperative 257th
query with and without the bias position, and the three block maps of launch_attention with their thresholds.

Three groups.  ``value``: small random cases at scales 1 and 6, compared with ``tol``.  ``route``: larger batches at scale 1,
one per block map and threshold side, same comparison.  ``onehot``: constructions whose output must equal one V row exactly.
A spec is cheap (``specs(group)`` costs nothing at collection time); ``case(spec)`` builds the inputs and the reference once per
process and the result is never modified.
"""
import functools
import math
from types import SimpleNamespace as NS

import torch

F64 = torch.float64
SCALES = (1.0, 6.0)


def to_bf16(t):
    return t.to(torch.float32).to(torch.bfloat16)


# ---- the dispatch, mirrored -----------------------------------------------------------------------------------------------
def route(B, T, H, dh, bias, causal):
    """(instantiation, q_parts, even_map, r8, coop) of one hmm_op_attention_bf16 / hmm_op_attention_causal_bf16 call, or None
    where the call is refused.  This DOCUMENTS attention_bf16 / launch_attention (attention.hip) and the coop condition of
    attention_core.h as of the commit that added this file; it is not read from the library and is to be updated with them.

    instantiation: (dh, key tiles) of the attention_kernel template.  q_parts: workgroups per (sample, head).  even_map: the
    (sample, head) list in eight contiguous runs, grid B*H; r8 = B*H % 8 is the number of runs that are one longer (0 without
    the even map).  Without the even map the legacy map is used: 8 * ceil(B/8) * H * q_parts blocks, padding blocks return.
    coop: the single query of the ninth query tile is computed by all waves, one key tile each."""
    Lk = T + (1 if bias else 0)
    if B < 1 or T < 1 or H < 1 or (causal and bias):
        return None
    if dh == 80 and Lk <= 288:
        inst = (80, 9)
    elif dh == 64 and Lk <= 96:
        inst = (64, 3)
    elif dh == 64 and Lk <= 256:
        inst = (64, 8)
    else:
        return None
    wgs = 8 * ((B + 7) // 8) * H
    q_parts = 2 if (T > 128 and 2 * wgs <= 256) else 1
    even_map = q_parts == 1 and T > 128
    r8 = (B * H) % 8 if even_map else 0
    coop = T == 257 and not causal
    return inst, q_parts, even_map, r8, coop


def _route_tag(r):
    (dh, nkt), q_parts, even_map, r8, coop = r
    return f"{dh}x{nkt}/q{q_parts}/{'even,r8=' + str(r8) if even_map else 'legacy'}{'/coop' if coop else ''}"


# ---- reference ------------------------------------------------------------------------------------------------------------
def attention_ref(qkv, B, T, H, dh, bias_k=None, bias_v=None, causal=False, *, keys=None, use_bias=True, use_bias_v=True,
                  round_bias_k=True, dup_edges=(), causal_shift=0, reverse_samples=False, head_shift=0, last_query_from=None,
                  scale_dh=None, drop_keys=(), repeat_key=None):
    """softmax(q k^T / sqrt(dh)) v per (sample, head) in float64 on the bf16 operands of the packed [B*T][q | k | v] matrix
    (each part H heads of dh).  bias_k / bias_v (fp32, H*dh) are rounded to bf16, as the kernel rounds them when it writes them
    into its K and V images, and appended as key T of every sample.  causal: query i sees keys 0..i.
    Returns (want, absv), both float64 [B*T][H*dh]: the attention output, and softmax @ |v| -- the size of the sum whose terms
    the kernel rounds.

    Every keyword after the star is a deliberate mistake for tests/test_cpu_attention_cases.py, off by default: ``keys`` keeps
    only the first so many keys; ``use_bias`` False drops the bias position, ``use_bias_v`` False appends zeros for bias_v,
    ``round_bias_k`` False appends bias_k unrounded; ``dup_edges`` copies key e over key e-1 for each e given; ``causal_shift``
    s makes key j visible iff j <= i + s; ``reverse_samples`` answers sample b with sample B-1-b; ``head_shift`` answers head h
    with head h + shift; ``last_query_from`` r answers query T-1 with query r's row; ``scale_dh`` takes 1/sqrt of another dh;
    ``drop_keys`` leaves out the keys given; ``repeat_key`` (j, count) appends count copies of key j behind the last key."""
    D = H * dh
    q, k, v = qkv.to(F64).reshape(B, T, 3, H, dh).unbind(2)                           # (B, T, H, dh)
    if bias_k is not None and use_bias:
        bk = (to_bf16(bias_k) if round_bias_k else bias_k).to(F64).reshape(1, 1, H, dh).expand(B, -1, -1, -1)
        bv = (to_bf16(bias_v).to(F64) if use_bias_v else torch.zeros(D, dtype=F64)).reshape(1, 1, H, dh).expand(B, -1, -1, -1)
        k, v = torch.cat([k, bk], 1), torch.cat([v, bv], 1)
    if dup_edges:
        k, v = k.clone(), v.clone()
        for e in dup_edges:
            k[:, e - 1], v[:, e - 1] = k[:, e], v[:, e]
    if repeat_key is not None:
        j, count = repeat_key
        k, v = (torch.cat([t, t[:, j:j + 1].expand(-1, count, -1, -1)], 1) for t in (k, v))
    if drop_keys:
        kept = [j for j in range(k.shape[1]) if j not in drop_keys]
        k, v = k[:, kept], v[:, kept]
    if keys is not None:
        k, v = k[:, :keys], v[:, :keys]
    Lk = k.shape[1]
    scale = 1.0 / math.sqrt(scale_dh or dh)
    want, absv = torch.empty(B, T, H, dh, dtype=F64), torch.empty(B, T, H, dh, dtype=F64)
    visible = torch.arange(Lk).reshape(1, Lk) <= torch.arange(T).reshape(T, 1) + causal_shift
    for b in range(B):                                                               # per sample: the scores stay small
        s = torch.einsum("ihd,jhd->hij", q[b], k[b]) * scale
        if causal:
            s = s.masked_fill(~visible, float("-inf"))
        p = torch.softmax(s, dim=-1)                                                 # a row without a visible key is NaN
        want[b] = torch.einsum("hij,jhd->ihd", p, v[b])
        absv[b] = torch.einsum("hij,jhd->ihd", p, v[b].abs())
    if reverse_samples:
        want = want.flip(0)
    if head_shift:
        want = torch.roll(want, -head_shift, dims=2)
    if last_query_from is not None:
        want = want.clone()
        want[:, T - 1] = want[:, last_query_from]
    return want.reshape(B * T, D), absv.reshape(B * T, D)


# ---- comparison -----------------------------------------------------------------------------------------------------------
def tolerance(want, absv):
    """Per element.  The kernel rounds P to bf16 once and the output once.  A bf16 rounding moves a value by at most 2^-9 of the
    power of two above it, which is 2^-9 of the value just below a power of two and 2^-8 just above one; so the two roundings
    give at most 2^-8 (|want| + sum p |v|), typically about half of that, and the 1e-4 is for the fp32 scores and sums.  This
    is the quantity that the 2^-8 * scale of test_attention stood for.  The rounded reference alone uses at most half of it
    (sum p |v| >= |want|); the kernel reaches 0.88 at scale 6 (profiles/attention_edges_parity.json)."""
    return 2.0 ** -8 * want.abs() + 2.0 ** -8 * absv + 1e-4


def ratio(case, got):
    """Worst |got - want| / tol over the elements (inf for a NaN or an infinity) of a value or route case."""
    assert got.dtype == torch.bfloat16 and got.shape == case.want.shape, (got.dtype, got.shape, case.want.shape)
    r = (got.to(F64) - case.want).abs() / case.tol
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return float(r.max())


def check(case, got):
    """Raises AssertionError when ``got`` (bf16 [B*T][H*dh] on the CPU: the kernel's output, or a mutant's result rounded to
    bf16) is not the case's result."""
    if case.group == "onehot":
        assert got.dtype == torch.bfloat16 and got.shape == case.picked.shape
        same = (got.view(torch.int16) == case.picked.view(torch.int16)).all(dim=1)
        assert bool(same.all()), (f"{case.label}: {int((~same).sum())} / {same.numel()} rows are not the picked V row; first at "
                                  f"(sample, query) {divmod(int(torch.nonzero(~same)[0]), case.T)}")
        return
    assert torch.isfinite(got.float()).all(), f"{case.label}: the output is not finite"
    r = ratio(case, got)
    assert r <= 1.0, f"{case.label}: worst error {r:.3f} of the tolerance"


# ---- random inputs --------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def planted_keys(T, Lk):
    """The keys of the token matrix that a random case makes heavy: the last one, and the last key of tile t-1 and the first
    key of tile t at every 32-key tile boundary below Lk (the bias position, key T, is planted apart)."""
    edge = {e for t in range(1, (Lk + 31) // 32) if 32 * t < Lk for e in (32 * t - 1, 32 * t)}
    return sorted(j for j in edge | {T - 1} if j < T)


def random_inputs(B, T, H, dh, bias, causal, scale, seed):
    """qkv bf16 [B*T][3*H*dh], bias_k, bias_v (fp32 H*dh, or None), built as stage_cases._attention_cls builds its own: normal
    values times ``scale`` (6: a peaky softmax), then some keys turned along a query of their head with the score of that
    query's best random key, so that they carry weight at scale 6 too and a dropped, duplicated or misplaced key shows there.
    Non-causal: the planted_keys(), each along its own query (spread over the query tiles), and sample 0's query for the bias
    position.  Causal: for every query i >= 1 key i, its last visible key, with the best score among the keys before it."""
    D, Lk = H * dh, T + (1 if bias else 0)
    g = _gen(seed)
    x = (torch.randn(B, T, 3, H, dh, generator=g) * scale).to(torch.bfloat16)
    bk = torch.randn(H, dh, generator=g) * scale if bias else None
    bv = torch.randn(H, dh, generator=g) * scale if bias else None
    if T > 1:
        q, k = x[:, :, 0].to(F64), x[:, :, 1].to(F64)
        s = torch.einsum("bihd,bjhd->bhij", q, k)                                    # raw scores of the random keys
        qq = (q * q).sum(-1).permute(0, 2, 1)                                        # (B, H, T)
        if causal:
            s = s.masked_fill(torch.arange(T).reshape(1, T) >= torch.arange(T).reshape(T, 1), float("-inf"))   # keys before i
            alpha = s[:, :, 1:].max(dim=-1).values / qq[:, :, 1:]                    # (B, H, T-1)
            x[:, 1:, 1] = to_bf16(alpha.permute(0, 2, 1).unsqueeze(-1) * q[:, 1:])
        else:
            keys = planted_keys(T, Lk)
            n = len(keys) + (1 if bias else 0)
            assert n <= T
            queries = [int((i + 0.5) * T / n) for i in range(n)]                     # distinct: n <= T
            s[:, :, :, keys] = float("-inf")
            alpha = s.max(dim=-1).values / qq                                        # (B, H, T): best random score / |q|^2
            for j, i in zip(keys, queries):
                x[:, j, 1] = to_bf16(alpha[:, :, i].unsqueeze(-1) * q[:, i])
            if bias:
                bk = (alpha[0, :, queries[-1]].unsqueeze(-1) * q[0, queries[-1]]).to(torch.float32)
    return x.reshape(B * T, 3 * D), (bk.reshape(D) if bias else None), (bv.reshape(D) if bias else None)


# ---- the table ------------------------------------------------------------------------------------------------------------
VALUE_T = {  # (dh, bias, causal) -> the T values
    (64, False, False): (1, 31, 32, 33, 64, 65, 95, 96, 97, 128, 129, 191, 192, 193, 255, 256),
    (64, True, False): (31, 32, 95, 96, 127, 128, 191, 192, 255),                    # Lk 32 33 96 97 128 129 192 193 256
    (80, False, False): (1, 32, 33, 96, 97, 129, 256, 257, 258, 287, 288),
    (80, True, False): (95, 96, 255, 256, 257, 287),
    (64, False, True): (1, 32, 33, 77, 96, 97, 128, 129, 256),
    (80, False, True): (257, 288),
}
ROUTE_SHAPES = [  # (B, T, H, dh, bias, causal)
    (9, 33, 2, 64, False, False), (17, 77, 16, 64, False, True), (9, 128, 3, 80, False, False),     # legacy map, several rounds
    (8, 257, 16, 80, False, False), (9, 257, 16, 80, False, False),                                   # the split threshold ...
    (8, 129, 16, 64, False, False), (9, 129, 16, 64, False, False),                                   # ... at both T > 128 kernels
    (9, 229, 12, 64, True, False), (131, 129, 1, 64, False, False), (41, 130, 3, 80, False, False),  # even map with a remainder
    (9, 150, 16, 64, False, True),
]


def _small_batch(T, dh):
    """B and H of a value or one-hot case: B 1 where T is 1 or a whole number of key tiles, else 2; H 3 for dh 64, 2 for dh 80."""
    return (1 if (T == 1 or T % 32 == 0) else 2), (3 if dh == 64 else 2)


def _spec(group, B, T, H, dh, bias, causal, scale=None):
    r = route(B, T, H, dh, bias, causal)
    assert r is not None, (B, T, H, dh, bias, causal)
    label = f"B={B},T={T},H={H},dh={dh}{',bias' if bias else ''}{',causal' if causal else ''}{'' if scale is None else f',scale={scale:g}'}[{_route_tag(r)}]"
    return NS(group=group, label=label, B=B, T=T, H=H, dh=dh, bias=bias, causal=causal, scale=scale, Lk=T + (1 if bias else 0),
              route=r, key=(group, B, T, H, dh, bias, causal, scale))


@functools.lru_cache(maxsize=None)
def specs(group):
    if group == "value":
        return tuple(_spec("value", _small_batch(T, dh)[0], T, _small_batch(T, dh)[1], dh, bias, causal, scale)
                     for (dh, bias, causal), ts in VALUE_T.items() for T in ts for scale in SCALES)
    if group == "route":
        return tuple(_spec("route", *shape, 1.0) for shape in ROUTE_SHAPES)
    if group == "onehot":
        return tuple(_spec("onehot", _small_batch(T, dh)[0], T, _small_batch(T, dh)[1], dh, bias, causal)
                     for (dh, bias, causal), ts in VALUE_T.items() for T in ts)
    raise KeyError(group)


GROUPS = ("value", "route", "onehot")


def all_specs():
    return tuple(s for g in GROUPS for s in specs(g))


def spec_ids(group):
    return [s.label for s in specs(group)]


def by_label(group, start):
    """The one spec of the group whose label starts with ``start`` (the part before the route tag)."""
    hit = [s for s in specs(group) if s.label.startswith(start + "[")]
    assert len(hit) == 1, (group, start, [s.label for s in hit])
    return hit[0]


def _seed(s):
    return (s.dh * 1000003 + s.T * 1009 + s.B * 101 + s.H * 11 + 5 * s.bias + 3 * s.causal + int(s.scale or 0)) % (2 ** 31)


def _random_case(s):
    qkv, bk, bv = random_inputs(s.B, s.T, s.H, s.dh, s.bias, s.causal, s.scale, _seed(s))
    want, absv = attention_ref(qkv, s.B, s.T, s.H, s.dh, bk, bv, s.causal)
    return NS(**vars(s), qkv=qkv, bk=bk, bv=bv, want=want, absv=absv, tol=tolerance(want, absv))


def _onehot_case(s):
    """Extends test_attention_one_hot_rows_pick_the_right_value to every T of the value lists.  Key j lies on axis j % dh with
    length 1 + j // dh and every query has length 300 along one axis, so the longest visible key of that axis wins by more than
    30 nats and the output row is exactly that key's V row.
    Non-causal: query i of sample b aims at axis (i + 3 b) % min(dh, Lk); query 0 of sample 0 at the very last position (the last
    key, or the bias position), and with a bias position query 1 of sample 0 at the last key of the token matrix.
    Causal: query i < dh - 1 aims at its own axis i, where key i is the only visible key; query i >= dh - 1 at axis (i + 1) % dh,
    whose longest visible key is i + 1 - dh and whose next key, i + 1, is the first invisible one: a mask one key too wide
    returns V of key i + 1, a mask one key too narrow loses key i for the queries below dh - 1."""
    B, T, H, dh, Lk = s.B, s.T, s.H, s.dh, s.Lk
    D = H * dh
    g = _gen(_seed(s))
    k = torch.zeros(Lk, H, dh)
    for j in range(Lk):
        k[j, :, j % dh] = 1.0 + j // dh
    v = to_bf16(torch.randn(B, Lk, H, dh, generator=g)).float()
    v[:, T:] = v[:1, T:]                                                             # the bias position is shared by the samples
    i, b = torch.arange(T).reshape(1, T).expand(B, T), torch.arange(B).reshape(B, 1)
    if s.causal:
        axis = torch.where(i < dh - 1, i, (i + 1) % dh)
        winner = torch.where(i < dh - 1, i, i + 1 - dh)
    else:
        axis = (i + 3 * b) % min(dh, Lk)
        axis[0, 0] = (Lk - 1) % dh
        if s.bias:
            axis[0, 1] = (T - 1) % dh
        winner = axis + dh * ((Lk - 1 - axis) // dh)                                 # the longest key of the axis
        assert winner[0, 0] == Lk - 1 and (not s.bias or winner[0, 1] == T - 1)
    q = torch.zeros(B, T, H, dh)
    q[torch.arange(B).reshape(B, 1), torch.arange(T).reshape(1, T), :, axis] = 300.0
    x = torch.zeros(B, T, 3, H, dh)
    x[:, :, 0], x[:, :, 1], x[:, :, 2] = q, k[:T], v[:, :T]
    qkv = to_bf16(x).reshape(B * T, 3 * D)
    bk, bv = (k[T].reshape(D).clone(), v[0, T].reshape(D).clone()) if s.bias else (None, None)
    picked = to_bf16(v[torch.arange(B).reshape(B, 1), winner]).reshape(B * T, D)
    # on the CPU: the winner leads every other visible key by >= 30 nats, and the float64 reference rounds to the picked row
    sc = torch.einsum("bihd,jhd->bhij", q.to(F64), k.to(F64)) / math.sqrt(dh)
    if s.causal:
        sc = sc.masked_fill(torch.arange(Lk).reshape(1, Lk) > torch.arange(T).reshape(T, 1), float("-inf"))
    top2 = sc.topk(min(2, Lk), dim=-1)
    assert torch.equal(top2.indices[..., 0], winner.reshape(B, 1, T).expand(B, H, T)), f"{s.label}: the winner is not the best key"
    assert Lk == 1 or bool((top2.values[..., 0] - top2.values[..., 1] >= 30.0).all()), f"{s.label}: a lead below 30 nats"
    want, absv = attention_ref(qkv, B, T, H, dh, bk, bv, s.causal)
    assert torch.equal(to_bf16(want).view(torch.int16), picked.view(torch.int16)), f"{s.label}: the reference does not select one V row"
    return NS(**vars(s), qkv=qkv, bk=bk, bv=bv, want=want, absv=absv, tol=tolerance(want, absv), picked=picked)


@functools.lru_cache(maxsize=None)
def _case(key):
    s = next(s for s in specs(key[0]) if s.key == key)
    return _onehot_case(s) if s.group == "onehot" else _random_case(s)


def case(spec):
    return _case(spec.key)


# ---- bit invariance across routes -------------------------------------------------------------------------------------------
INVARIANCE = [  # (T, H, dh, bias, causal, batch sizes): batch size and position in the batch change the route, never the bits
    (257, 16, 80, False, False, (1, 8, 9, 17)),
    (229, 12, 64, True, False, (1, 8, 9, 17)),
    (77, 16, 64, False, True, (1, 9, 17)),
]


@functools.lru_cache(maxsize=None)
def invariance_pool(T, H, dh, bias, causal):
    """17 distinct samples (17, T, 3*H*dh) bf16 with their bias pair; sample 0 is the one that is moved about."""
    qkv, bk, bv = random_inputs(17, T, H, dh, bias, causal, 1.0, 7919 * T + dh)
    return qkv.reshape(17, T, 3 * H * dh), bk, bv


def invariance_batch(pool, B, position):
    """B samples of the pool with sample 0 at ``position`` and the samples 1 .. B-1 around it, in order."""
    others = pool[1:B]
    return torch.cat([others[:position], pool[:1], others[position:]]).reshape(B * pool.shape[1], pool.shape[2]).contiguous()


# ---- refused calls --------------------------------------------------------------------------------------------------------
REJECTED = [  # (label, B, T, H, dh, bias_k given, bias_v given, causal)
    ("dh=64,T=257", 1, 257, 2, 64, False, False, False),
    ("dh=64,T=256,bias", 1, 256, 2, 64, True, True, False),
    ("dh=80,T=289", 1, 289, 2, 80, False, False, False),
    ("dh=80,T=288,bias", 1, 288, 2, 80, True, True, False),
    ("dh=32", 1, 33, 2, 32, False, False, False),
    ("dh=64,T=257,causal", 1, 257, 2, 64, False, False, True),
    ("bias_k without bias_v", 1, 33, 2, 64, True, False, False),
    ("bias_v without bias_k", 1, 33, 2, 64, False, True, False),
    ("B=0", 0, 33, 2, 64, False, False, False),
    ("T=0", 1, 0, 2, 64, False, False, False),
    ("H=0", 1, 33, 0, 64, False, False, False),
    ("B=0,causal", 0, 33, 2, 64, False, False, True),
]
