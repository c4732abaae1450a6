"""The inputs, the float64 reference and the mutants of tests/test_gpu_fused_attention_edges.py: the fused in_proj + attention
kernel (hippomm_amd/csrc/qkv_attention.hip behind hmm_op_qkv_attention_bf16 and hmm_op_qkv_attention_audio_bf16) against a
reference that neither the GEMM nor the attention kernel had a hand in.  Kept apart from the GPU module so that
tests/test_cpu_fused_attention_cases.py can run WRONG references through the same inputs and the same comparison without a GPU.
The reference (``attention_ref``), the tolerance and ``check`` are those of tests/attention_cases.py, unchanged; nothing here
comes from hippomm_amd/.

The lift.  T <= D in both geometries (257 <= 1280, 229 <= 768), so any wanted pre-bias qkv matrix P (T x 3D, bf16) is the exact
product of two bf16 operands: token t's row of ``a`` is a single 1.0 at column c0 + t, and w[:, c0 + t] = P[t, :].  Every dot
product has one non-zero term, so the fp32 accumulator holds P exactly whatever the order of the K loop; the kernel's stage 2 is
one fp32 add of in_proj_bias and one round-to-nearest-even, so the images it must hold are exactly
``(P.float() + bias).to(bfloat16)``.  D // T column blocks of ``w`` hold independent matrices (4 vision, 3 audio), and a
rotation r of a block's token order (token t takes row (t + r) mod T) gives further distinct images from the same ``w``.

Four groups, all at the two real geometries.  ``value``: attention_cases.random_inputs (planted heavy keys included) at scales
1 and 6 as the target, one image per block.  ``onehot``: constructions whose output is exactly one V row.  ``deal``: batch sizes
at which the (sample, head) deal of the kernel changes, every image distinct (blocks x rotations).  ``dense``: Gaussian
operands, compared with the two-kernel route only.
"""
import functools
from types import SimpleNamespace as NS

import torch

import attention_cases as A

F64 = torch.float64
BF16 = torch.bfloat16
GEOS = {
    "vision": NS(name="vision", T=257, H=16, dh=80, D=1280, bias=False, blocks=4),
    "audio": NS(name="audio", T=229, H=12, dh=64, D=768, bias=True, blocks=3),
}
DEFAULT_CUS = 256                                  # an MI355X; one workgroup of the fused kernel is resident per CU
ROTATIONS = (0, 1, 37, 128, 228, 64, 200, 100)     # of the j-th round of images over the blocks; all distinct and below 229
DEAL_NAMES = {"vision": ("1", "2", "CUs/16", "CUs/16+1"), "audio": ("1", "2", "21", "CUs/12+1", "CUs/12+2")}
ONEHOT = (("vision", "last"), ("vision", "first"), ("audio", "bias"), ("audio", "last_token"))


def deal_sizes(name, cus=DEFAULT_CUS):
    """The batch sizes of the deal group.  Vision: B*H % 8 is always 0, the sizes straddle one round of workgroups.  Audio:
    n*12 % 8 is 4, 0, 4, 0, 4 (at 256 CUs: 21, 22, 23), the last two with more workgroups than CUs."""
    return (1, 2, cus // 16, cus // 16 + 1) if name == "vision" else (1, 2, 21, cus // 12 + 1, cus // 12 + 2)


# ---- the lift -------------------------------------------------------------------------------------------------------------
def block_columns(blocks, T, D):
    """First column of each block of ``w``: side by side from column 0, the last one flush with column D - 1, so that the
    first and the last K step of the projection both carry data."""
    assert 1 <= blocks and blocks * T <= D
    return [b * T for b in range(blocks - 1)] + [D - T]


def lifted(P_blocks, rotations):
    """The pre-bias qkv matrices (n, T, 3D) that lift() encodes: image i = block b_i with token t taking row (t + r_i) mod T."""
    return torch.stack([torch.roll(P_blocks[b], -r, 0) for b, r in rotations])


def lift(P_blocks, rotations):
    """P_blocks (blocks, T, 3D) bf16, rotations [(block, r)] per image -> a (n*T, D), w (3D, D), both bf16, with
    a @ w.T == lifted(P_blocks, rotations) exactly in any summation order."""
    blocks, T, N = P_blocks.shape
    D = N // 3
    start = block_columns(blocks, T, D)
    w = torch.zeros(N, D, dtype=BF16)
    for b, c in enumerate(start):
        w[:, c:c + T] = P_blocks[b].T
    a = torch.zeros(len(rotations), T, D, dtype=BF16)
    t = torch.arange(T)
    for i, (b, r) in enumerate(rotations):
        assert 0 <= r < T
        a[i, t, start[b] + (t + r) % T] = 1.0
    return a.reshape(-1, D), w


def assert_exact(a, w, pre):
    """In float64, a @ w.T is the wanted pre-bias matrix bit for bit."""
    got = a.to(F64) @ w.to(F64).T
    assert torch.equal(got, pre.reshape(got.shape).to(F64)), "the lift does not reproduce the wanted qkv matrix"


# ---- what the kernel must hold ----------------------------------------------------------------------------------------------
BUILDER_MUTANTS = ("drop_bias", "bias_head_shift", "swap_kv", "cls_from_other", "cls_zeros", "rows_shifted", "v_tail_zero")


def expected_qkv(pre, in_bias, g, *, drop_bias=None, bias_head_shift=0, swap_kv=False, cls_from_other=False, cls_zeros=False,
                 rows_shifted=False, v_tail_zero=False):
    """pre (n, T, 3D) bf16, in_bias fp32 (3D) -> (n, T, 3D) bf16: (P.float() + bias).to(bfloat16), the q | k | v rows of every
    token.  For vision, row 0 of each image is what arrives through qkv_cls.

    Every keyword is a deliberate mistake of the kernel's stage 2 for tests/test_cpu_fused_attention_cases.py, off by default:
    ``drop_bias`` 'q' / 'k' / 'v' leaves in_proj_bias off that part; ``bias_head_shift`` s gives head h the bias of head h + s
    (both on the rows the kernel projects itself: vision's cls row comes finished from the caller); ``swap_kv`` exchanges the k
    and v slices; ``cls_from_other`` takes vision's token 0 from image n-1-b, ``cls_zeros`` leaves it zero; ``rows_shifted``
    stores the projected rows one token early (vision: tokens 2..256 land on 1..255 and 256 stays zero; audio: token 0 is lost
    and the clamped tile row repeats token 228); ``v_tail_zero`` zeroes vision's v dims 64..79 of the projected rows."""
    n, T, N = pre.shape
    assert (T, N) == (g.T, 3 * g.D) and pre.dtype == BF16 and in_bias.dtype == torch.float32
    good = (pre.float() + in_bias).to(BF16)
    b = in_bias.reshape(3, g.H, g.dh).clone()
    if bias_head_shift:
        b = torch.roll(b, -bias_head_shift, 1)
    if drop_bias is not None:
        b["qkv".index(drop_bias)] = 0.0
    x = (pre.float() + b.reshape(N)).to(BF16)
    own = 0 if g.name == "audio" else 1                                              # first token the kernel projects itself
    x[:, :own] = good[:, :own]
    x5 = x.reshape(n, T, 3, g.H, g.dh)
    if v_tail_zero:
        x5[:, own:, 2, :, 64:] = 0
    if rows_shifted:
        y = x.clone()
        if own:
            x[:, 1:T - 1], x[:, T - 1] = y[:, 2:], 0
        else:
            x[:, :T - 1] = y[:, 1:]
    if swap_kv:
        k = x5[:, :, 1].clone()
        x5[:, :, 1], x5[:, :, 2] = x5[:, :, 2].clone(), k
    if cls_from_other:
        x[:, 0] = x.flip(0)[:, 0].clone()
    if cls_zeros:
        x[:, 0] = 0
    return x


# ---- the images -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blocks(name, scale):
    """The targets of a geometry at one scale: attention_cases.random_inputs with one sample per block, a random fp32
    in_proj_bias of about 0.1 x scale, and P = bf16(target - bias)."""
    g = GEOS[name]
    seed = 977 * g.T + int(scale)
    target, bk, bv = A.random_inputs(g.blocks, g.T, g.H, g.dh, g.bias, False, scale, seed)
    in_bias = torch.randn(3 * g.D, generator=torch.Generator().manual_seed(seed + 1)) * (0.1 * scale)
    P = A.to_bf16(target.float().reshape(g.blocks, g.T, 3 * g.D) - in_bias)
    return NS(P=P, in_bias=in_bias, bk=bk, bv=bv)


@functools.lru_cache(maxsize=None)
def _image(name, scale, block, r):
    """One image of the random pool with its own float64 reference; the lift is proved on it."""
    g, s = GEOS[name], _blocks(name, scale)
    pre = lifted(s.P, [(block, r)])
    assert_exact(*lift(s.P, [(block, r)]), pre)
    qkv = expected_qkv(pre, s.in_bias, g)[0]
    want, absv = A.attention_ref(qkv, 1, g.T, g.H, g.dh, s.bk, s.bv)
    return NS(pre=pre[0], qkv=qkv, want=want, absv=absv)


def pool_rotation(name, i):
    """(block, r) of image i of the random pool: the blocks in turn, each round of them with the next rotation."""
    g = GEOS[name]
    return i % g.blocks, ROTATIONS[i // g.blocks]


def _assemble(group, label, g, P_blocks, rotations, in_bias, bk, bv, images, **more):
    n = len(rotations)
    a, w = lift(P_blocks, rotations)
    qkv = torch.cat([im.qkv for im in images])
    want, absv = torch.cat([im.want for im in images]), torch.cat([im.absv for im in images])
    return NS(group=group, label=label, geo=g, name=g.name, B=n, T=g.T, H=g.H, dh=g.dh, D=g.D, bias=g.bias, a=a, w=w, in_bias=in_bias,
              pre=torch.stack([im.pre for im in images]), qkv=qkv, bk=bk, bv=bv,
              qkv_cls=(qkv.reshape(n, g.T, 3 * g.D)[:, 0].contiguous() if g.name == "vision" else None),
              want=want, absv=absv, tol=A.tolerance(want, absv), **more)


def batch(name, indices, scale=1.0, group="deal", label=None):
    """The images ``indices`` of the random pool as one call.  Not cached: the images and their references are."""
    g, s = GEOS[name], _blocks(name, scale)
    rotations = [pool_rotation(name, i) for i in indices]
    images = [_image(name, scale, b, r) for b, r in rotations]
    return _assemble(group, label or f"{name},images={list(indices)}", g, s.P, rotations, s.in_bias, s.bk, s.bv, images, scale=scale)


def invariance_order(n, position):
    """Image 0 at ``position`` of a batch of n, the images 1 .. n-1 around it in order."""
    others = list(range(1, n))
    return others[:position] + [0] + others[position:]


# ---- one-hot ------------------------------------------------------------------------------------------------------------------
def _onehot(name, orientation):
    """Two images whose every output row is exactly one V row, in_proj_bias = 0 (all values are exact in bf16, so P is the
    target itself).
    ``last`` (vision) / ``bias`` (audio): attention_cases._onehot_case at the real head count -- the longest key of an axis wins,
    query 0 of sample 0 aims at the very last key or the bias position, and with a bias position query 1 at token T-1.
    ``first`` (vision): mirrored, key lengths fall with the key index, so the winners are keys 0 .. dh-1; query 0 of sample 0 and
    the last query of sample 1 aim at key 0, the key that arrives through qkv_cls.
    ``last_token`` (audio): the bias position lies on the axis of token 228 and is one shorter: query 0 of sample 0 picks the
    last real token, with the bias position as its runner-up."""
    g = GEOS[name]
    B, T, H, dh, D, Lk = 2, g.T, g.H, g.dh, g.D, g.T + (1 if g.bias else 0)
    label = f"{name},{orientation}"
    if orientation in ("last", "bias"):
        c = A._onehot_case(A._spec("onehot", B, T, H, dh, g.bias, False))
        target, bk, bv, picked = c.qkv, c.bk, c.bv, c.picked
    else:
        gen = torch.Generator().manual_seed(4001 + T)
        k = torch.zeros(Lk, H, dh)
        for j in range(T):
            k[j, :, j % dh] = 1.0 + ((T - 1 - j) if orientation == "first" else j) // dh
        if g.bias:
            k[T, :, (T - 1) % dh] = (T - 1) // dh                                    # one shorter than token T-1, on its axis
        v = A.to_bf16(torch.randn(B, Lk, H, dh, generator=gen)).float()
        v[:, T:] = v[:1, T:]
        i, b = torch.arange(T).reshape(1, T).expand(B, T), torch.arange(B).reshape(B, 1)
        axis = (i + 3 * b) % dh
        axis[0, 0] = 0 if orientation == "first" else (T - 1) % dh
        if orientation == "first":
            axis[1, T - 1] = 0
        q = torch.zeros(B, T, H, dh)
        q[torch.arange(B).reshape(B, 1), torch.arange(T).reshape(1, T), :, axis] = 300.0
        sc = torch.einsum("bihd,jhd->bhij", q.to(F64), k.to(F64)) / dh ** 0.5
        top2 = sc.topk(2, dim=-1)
        winner = top2.indices[:, 0, :, 0]                                            # the heads agree (asserted below)
        assert torch.equal(top2.indices[..., 0], winner.reshape(B, 1, T).expand(B, H, T))
        assert bool((top2.values[..., 0] - top2.values[..., 1] >= 30.0).all()), f"{label}: a lead below 30 nats"
        if orientation == "first":
            assert torch.equal(winner, axis) and winner[0, 0] == 0 and winner[1, T - 1] == 0 and int(winner.max()) == dh - 1
        else:
            assert winner[0, 0] == T - 1 and torch.equal(sc[0, :, 0, T], top2.values[0, :, 0, 1]), f"{label}: bias is not the runner-up"
        x = torch.zeros(B, T, 3, H, dh)
        x[:, :, 0], x[:, :, 1], x[:, :, 2] = q, k[:T], v[:, :T]
        target = A.to_bf16(x).reshape(B * T, 3 * D)
        bk, bv = (k[T].reshape(D).clone(), v[0, T].reshape(D).clone()) if g.bias else (None, None)
        picked = A.to_bf16(v[torch.arange(B).reshape(B, 1), winner]).reshape(B * T, D)
    P, in_bias = target.reshape(B, T, 3 * D), torch.zeros(3 * D)
    rotations = [(0, 0), (1, 0)]
    pre = lifted(P, rotations)
    assert_exact(*lift(P, rotations), pre)
    qkv = expected_qkv(pre, in_bias, g)
    assert torch.equal(qkv.view(torch.int16), P.view(torch.int16))
    want, absv = A.attention_ref(qkv.reshape(B * T, 3 * D), B, T, H, dh, bk, bv)
    assert torch.equal(A.to_bf16(want).view(torch.int16), picked.view(torch.int16)), f"{label}: the reference does not select one V row"
    images = [NS(pre=pre[i], qkv=qkv[i], want=want[i * T:(i + 1) * T], absv=absv[i * T:(i + 1) * T]) for i in range(B)]
    return _assemble("onehot", label, g, P, rotations, in_bias, bk, bv, images, picked=picked, orientation=orientation)


# ---- the table ----------------------------------------------------------------------------------------------------------------
GROUPS = ("value", "onehot", "deal")


def specs(group, cus=DEFAULT_CUS):
    """Cheap: names only.  ``cus`` (the device's CU count) sets the batch sizes of the deal group."""
    if group == "value":
        return tuple(NS(group=group, name=name, scale=s, label=f"{name},scale={s:g}", key=(group, name, s)) for name in GEOS for s in A.SCALES)
    if group == "onehot":
        return tuple(NS(group=group, name=name, orientation=o, label=f"{name},{o}", key=(group, name, o)) for name, o in ONEHOT)
    if group == "deal":
        return tuple(NS(group=group, name=name, n=n, label=f"{name},n={n}", key=(group, name, n), slot=f"{name},n={DEAL_NAMES[name][i]}")
                     for name in GEOS for i, n in enumerate(deal_sizes(name, cus)))
    raise KeyError(group)


def spec_ids(group):
    return [getattr(s, "slot", s.label) for s in specs(group)]


def by_label(group, label, cus=DEFAULT_CUS):
    hit = [s for s in specs(group, cus) if s.label == label]
    assert len(hit) == 1, (group, label)
    return hit[0]


@functools.lru_cache(maxsize=None)
def _small_case(key):
    group, name, what = key
    if group == "onehot":
        return _onehot(name, what)
    return batch(name, range(GEOS[name].blocks), what, "value", f"{name},scale={what:g}")


def case(spec):
    """The inputs and the float64 reference of a spec.  Value and one-hot cases are built once per process; a deal case is put
    together from images that are."""
    if spec.group == "deal":
        return batch(spec.name, range(spec.n), 1.0, "deal", spec.label)
    return _small_case(spec.key)


def wrong(c, **mistakes):
    """The float64 reference of case ``c`` with deliberate mistakes -- keywords of expected_qkv or of attention_ref -- rounded to
    bf16 as the kernel's output is."""
    built = {k: mistakes.pop(k) for k in BUILDER_MUTANTS if k in mistakes}
    qkv = expected_qkv(c.pre, c.in_bias, c.geo, **built).reshape(c.B * c.T, 3 * c.D)
    return A.to_bf16(A.attention_ref(qkv, c.B, c.T, c.H, c.dh, c.bk, c.bv, **mistakes)[0])


# ---- dense --------------------------------------------------------------------------------------------------------------------
def dense_sizes(cus=DEFAULT_CUS):
    return {"vision": cus // 16 + 1, "audio": cus // 12 + 1}


def dense_inputs(name, n):
    """Gaussian a, w, in_proj_bias (and bias_k / bias_v) as tests/test_gpu_ops.py draws them for the fused kernels."""
    g = GEOS[name]
    gen = torch.Generator().manual_seed(500 + n + g.T)
    a = A.to_bf16(torch.randn(n * g.T, g.D, generator=gen))
    w = A.to_bf16(torch.randn(3 * g.D, g.D, generator=gen) * (0.03 if name == "vision" else 0.04))
    in_bias = torch.randn(3 * g.D, generator=gen) * 0.1
    bk, bv = ((torch.randn(g.D, generator=gen) * 0.5, torch.randn(g.D, generator=gen) * 0.5) if g.bias else (None, None))
    return NS(geo=g, name=name, B=n, T=g.T, H=g.H, dh=g.dh, D=g.D, a=a, w=w, in_bias=in_bias, bk=bk, bv=bv)


# ---- refused calls ------------------------------------------------------------------------------------------------------------
FIRST_TOO_LARGE = {"vision": 6529, "audio": 12211}       # the first n with n * T * D >= 2^31; one less is the last valid one
