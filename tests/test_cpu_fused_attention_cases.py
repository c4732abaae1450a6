"""CPU: the table of tests/fused_attention_cases.py is exact, can fail, and the fused entry points refuse what they must.
No kernel runs.

1. Every case is exact: in float64 ``a @ w.T`` is the wanted pre-bias qkv matrix bit for bit (asserted by the builder for every
   image), and every one-hot winner leads by >= 30 nats with the float64 reference rounding to exactly one V row.
2. The unchanged float64 reference, rounded to bf16, stays at or below 0.5 of attention_cases.tolerance on every value and
   deal case.
3. Mutants: the reference with one deliberate mistake -- a keyword of expected_qkv or of attention_ref -- goes through the same
   inputs and the same comparison; each must be rejected on the cases named next to it.
4. Both entry points refuse null pointers and batch sizes out of range before any launch.
"""
import pytest
import torch

import attention_cases as A
import fused_attention_cases as F

V, O, D = "value", "onehot", "deal"


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------
def test_the_lift_reproduces_blocks_and_rotations_exactly():
    """A small lift by hand: 2 blocks of T = 5 in D = 12, one image per block and one rotated by 2."""
    P = A.to_bf16(torch.randn(2, 5, 36, generator=torch.Generator().manual_seed(1)))
    rotations = [(0, 0), (1, 0), (0, 2)]
    a, w = F.lift(P, rotations)
    assert a.shape == (15, 12) and w.shape == (36, 12) and F.block_columns(2, 5, 12) == [0, 7]
    assert bool((a.float().sum(1) == 1).all()) and bool(((a == 0) | (a == 1)).all())          # one 1.0 per row
    pre = F.lifted(P, rotations)
    F.assert_exact(a, w, pre)
    assert torch.equal(pre[0], P[0]) and torch.equal(pre[1], P[1]) and torch.equal(pre[2, 0], P[0, 2]) and torch.equal(pre[2, 4], P[0, 1])
    assert a[10, 2] == 1 and a[1, 1] == 1 and a[5, 7] == 1                                       # token 0 of the rotated image: row 2
    with pytest.raises(AssertionError):
        F.assert_exact(a, w, F.lifted(P, [(0, 0), (1, 0), (0, 3)]))


def test_the_real_geometries_use_every_block_and_the_first_and_last_k_step():
    for name, g in F.GEOS.items():
        assert g.blocks == g.D // g.T and g.T <= g.D
        start = F.block_columns(g.blocks, g.T, g.D)
        assert start[0] == 0 and start[-1] + g.T == g.D and all(b - a >= g.T for a, b in zip(start, start[1:]))
        c = F.case(F.specs(V)[0 if name == "vision" else 2])
        assert c.name == name and c.B == g.blocks
        used = c.w.float().abs().sum(0) > 0
        assert int(used.sum()) == g.blocks * g.T and bool(used[0]) and bool(used[-1])
        assert len({c.qkv.reshape(c.B, -1)[i].view(torch.int16).numpy().tobytes() for i in range(c.B)}) == c.B


def test_expected_qkv_is_one_fp32_add_and_one_nearest_even_rounding():
    c = F.case(F.by_label(V, "audio,scale=6"))
    want = (c.pre.double() + c.in_bias.double()).float()                            # exact sum, rounded once to fp32 ...
    assert torch.equal(c.qkv.view(torch.int16), want.to(torch.bfloat16).reshape(c.qkv.shape).view(torch.int16))
    v = F.case(F.by_label(V, "vision,scale=1"))
    assert torch.equal(v.qkv_cls, v.qkv.reshape(v.B, v.T, -1)[:, 0]) and c.qkv_cls is None


@pytest.mark.parametrize("spec", F.specs(O), ids=F.spec_ids(O))
def test_one_hot_constructions_hold(spec):
    """The builder asserts the bit-equal lift, the 30-nat lead and the exact pick of the float64 reference."""
    c = F.case(spec)
    A.check(c, A.to_bf16(c.want))
    assert c.picked.shape == (2 * c.T, c.D) and not bool(c.in_bias.any())
    rows = c.picked.reshape(2, c.T, c.H, c.dh)
    v = c.qkv.reshape(2, c.T, 3, c.H, c.dh)[:, :, 2]
    if spec.orientation == "first":                                                  # key 0, the cls row, is picked at both ends
        assert torch.equal(rows[0, 0], v[0, 0]) and torch.equal(rows[1, c.T - 1], v[1, 0])
    if spec.orientation == "last":
        assert torch.equal(rows[0, 0], v[0, c.T - 1])
    if spec.orientation == "bias":
        assert torch.equal(rows[0, 0].reshape(-1), A.to_bf16(c.bv)) and torch.equal(rows[0, 1], v[0, c.T - 1])
    if spec.orientation == "last_token":
        assert torch.equal(rows[0, 0], v[0, c.T - 1])


def test_the_deal_sizes_straddle_one_round_of_workgroups():
    assert F.deal_sizes("vision") == (1, 2, 16, 17) and F.deal_sizes("audio") == (1, 2, 21, 22, 23)
    assert [n * 12 % 8 for n in F.deal_sizes("audio")] == [4, 0, 4, 0, 4]
    assert 16 * 16 == 256 < 17 * 16 and 21 * 12 < 256 < 22 * 12 < 23 * 12
    for name, g in F.GEOS.items():
        n = max(F.deal_sizes(name))
        assert len({F.pool_rotation(name, i) for i in range(n)}) == n and n <= g.blocks * len(F.ROTATIONS)
        assert max(F.ROTATIONS) < g.T and len(set(F.ROTATIONS)) == len(F.ROTATIONS)
    assert F.dense_sizes() == {"vision": 17, "audio": 22}
    assert F.invariance_order(5, 0) == [0, 1, 2, 3, 4] and F.invariance_order(5, 2) == [1, 2, 0, 3, 4] and F.invariance_order(5, 4) == [1, 2, 3, 4, 0]


# ---- 2. the unchanged reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [V, D])
def test_the_unchanged_reference_stays_below_half_of_the_tolerance(group):
    """A condition on the inputs: the bf16 rounding of the exact result uses at most 2^-9 |want| of a tolerance of at least
    2^-8 |want|; the rest is the kernel's.  Building a case also proves every image's lift bit-equal."""
    worst = 0.0
    for s in F.specs(group):
        c = F.case(s)
        got = A.to_bf16(c.want)
        A.check(c, got)
        r = A.ratio(c, got)
        assert r <= 0.5, f"{c.label}: the rounded reference is at {r:.3f} of the tolerance"
        worst = max(worst, r)
        images = c.qkv.reshape(c.B, -1).view(torch.int16)
        assert len({images[i].numpy().tobytes() for i in range(c.B)}) == c.B, f"{c.label}: two images are the same"
    print(f"{group}: the rounded reference is at most at {worst:.3f} of the tolerance")


# ---- 3. mutants -----------------------------------------------------------------------------------------------------------
VIS, AUD = [(V, "vision,scale=1"), (V, "vision,scale=6"), (D, "vision,n=17")], [(V, "audio,scale=1"), (V, "audio,scale=6"), (D, "audio,n=23")]
BOTH = VIS + AUD
SWAPS = [(V, "vision,scale=1"), (V, "audio,scale=6"), (O, "vision,last"), (O, "audio,bias"), (D, "vision,n=2"), (D, "vision,n=16"),
         (D, "vision,n=17"), (D, "audio,n=2"), (D, "audio,n=21"), (D, "audio,n=22"), (D, "audio,n=23")]
# (name, the mistake as a function of the case, the cases that must catch it: (group, label))
MUTANTS = [
    # the new ones: stage 2 of the fused kernel
    ("in_proj_bias dropped on q", lambda c: dict(drop_bias="q"), BOTH),
    ("in_proj_bias dropped on k", lambda c: dict(drop_bias="k"), BOTH),
    ("in_proj_bias dropped on v", lambda c: dict(drop_bias="v"), BOTH),
    ("head h gets the bias of head h + 1", lambda c: dict(bias_head_shift=1), BOTH),
    ("k and v slices exchanged", lambda c: dict(swap_kv=True), BOTH + [(O, s.label) for s in F.specs(O)]),
    ("cls row from image n-1-b", lambda c: dict(cls_from_other=True),
     [(V, "vision,scale=1"), (V, "vision,scale=6"), (O, "vision,first"), (O, "vision,last"), (D, "vision,n=2"), (D, "vision,n=16"), (D, "vision,n=17")]),
    ("cls row left zero", lambda c: dict(cls_zeros=True), VIS + [(O, "vision,first"), (O, "vision,last"), (D, "vision,n=1")]),
    ("key 0 missing", lambda c: dict(drop_keys=(0,)), BOTH + [(O, "vision,first")]),
    ("key T-1 missing", lambda c: dict(drop_keys=(c.T - 1,)), BOTH + [(O, "vision,last"), (O, "audio,bias"), (O, "audio,last_token")]),
    ("projected rows stored one token early", lambda c: dict(rows_shifted=True), BOTH + [(O, s.label) for s in F.specs(O)]),
    ("vision v dims 64..79 zero", lambda c: dict(v_tail_zero=True), VIS + [(O, "vision,first"), (O, "vision,last")]),
    ("audio keys 230..255 are copies of token 228", lambda c: dict(repeat_key=(c.T - 1, 26)), AUD + [(D, "audio,n=1")]),
    # the ones attention_ref already has
    ("bias position dropped", lambda c: dict(use_bias=False), AUD + [(O, "audio,bias")]),
    ("bias_v replaced by zeros", lambda c: dict(use_bias_v=False), AUD + [(O, "audio,bias")]),
    ("bias_k not rounded to bf16", lambda c: dict(round_bias_k=False), [(V, "audio,scale=6")]),          # scale 6 only: see attention_cases
    ("samples walked in reverse order", lambda c: dict(reverse_samples=True), SWAPS),
    ("heads rotated by one", lambda c: dict(head_shift=1), BOTH + [(O, s.label) for s in F.specs(O)] + [(D, "vision,n=1"), (D, "audio,n=1")]),
    ("query T-1 answered with query T-2's row", lambda c: dict(last_query_from=c.T - 2), BOTH + [(O, "vision,first"), (O, "vision,last")]),
    ("scale 1/sqrt(dh) of the other tower", lambda c: dict(scale_dh=144 - c.dh), BOTH),
]
# What cannot show: a one-hot winner leads by 30 nats, which a bias of zero, the other scale or one dropped loser do not change;
# "reverse" and "cls from image n-1-b" need two images.


def _rejected(c, got):
    try:
        A.check(c, got)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name,mistake,caught_by", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_rejected_by_the_gpu_tests_comparison(name, mistake, caught_by):
    survived = []
    for group, label in caught_by:
        c = F.case(F.by_label(group, label))
        if not _rejected(c, F.wrong(c, **mistake(c))):
            survived.append(c.label)
    assert not survived, f"'{name}' passes the comparison on {survived}"


def test_every_mutant_of_the_issue_is_listed_and_the_unmutated_builder_passes():
    assert len(MUTANTS) == 19 and len({m[0] for m in MUTANTS}) == 19            # 12 new (bias dropped counts three) + 7 reused
    used = {k for _, mistake, _ in MUTANTS for k in mistake(F.case(F.by_label(V, "audio,scale=1")))}
    assert set(F.BUILDER_MUTANTS) <= used and {"drop_keys", "repeat_key"} <= used
    for s in F.specs(V) + F.specs(O):
        c = F.case(s)
        assert not _rejected(c, F.wrong(c)), c.label                                # wrong() without a mistake is the reference
    # every pair of images of a deal batch exchanged shows: each image has its own reference
    c = F.case(F.by_label(D, "audio,n=23"))
    got = A.to_bf16(c.want).reshape(c.B, c.T, c.D)
    for i, j in ((0, 3), (1, 22), (20, 21)):                                        # same block, another rotation; neighbours
        swapped = got.clone()
        swapped[i], swapped[j] = got[j], got[i]
        assert _rejected(c, swapped.reshape(c.B * c.T, c.D)), (i, j)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
HMM_E_INVALID = -1
ONE = 1 << 20                                                    # 16-byte aligned non-null dummies, far from each other
FAR = 1 << 40
ENTRY = {"vision": ("hmm_op_qkv_attention_bf16", 5, b"qkv_attention: "), "audio": ("hmm_op_qkv_attention_audio_bf16", 6, b"qkv_attention_audio: ")}


def _refused(name, pointers, n, say):
    """Every call here is refused before launch_fused touches the runtime: a call that launched with these addresses would be a
    failed refusal."""
    from hippomm_amd import _lib
    lib = _lib.load()
    rc = getattr(lib, ENTRY[name][0])(*pointers, n, None)
    err = lib.hmm_last_error()
    assert rc == HMM_E_INVALID and say in err, (name, pointers, n, rc, err)


@pytest.mark.parametrize("name", ["vision", "audio"])
def test_the_fused_entry_points_refuse_before_any_launch(name):
    symbol, count, prefix = ENTRY[name]
    full = [ONE + i * FAR for i in range(count)]
    for missing in range(count):
        _refused(name, [None if i == missing else p for i, p in enumerate(full)], 1, prefix + b"null pointer")
    too_large = F.FIRST_TOO_LARGE[name]
    g = F.GEOS[name]
    assert (too_large - 1) * g.T * g.D < 2 ** 31 <= too_large * g.T * g.D
    for n in (0, -1, too_large):
        _refused(name, full, n, b"qkv_attention: n_img=%d out of range" % n)
