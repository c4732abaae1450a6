"""CPU: the attention edge table of tests/attention_cases.py can fail, and reaches what it says it reaches.  No kernel runs.

1. The reference is scaled_dot_product_attention in float64.
2. Coverage: through route(), the table holds every instantiation, block map, threshold side and capacity limit.
3. Mutants: wrong references -- attention_ref with one argument changed -- go through the same inputs and the same comparison,
   rounded to bf16 as the kernel's output is; each must be rejected on the cases named next to it.
4. The unchanged reference, rounded to bf16, stays at or below 0.75 of the tolerance on every case.
5. The refusals of tests/test_gpu_attention_edges.py happen before any launch, so they are checked here as well.
"""
import pytest
import torch

import attention_cases as A


def _ref(c, **kw):
    return A.attention_ref(c.qkv, c.B, c.T, c.H, c.dh, c.bk, c.bv, c.causal, **kw)[0]


# ---- 1. the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,H,dh,bias,causal", [(2, 33, 3, 64, False, False), (1, 97, 2, 80, True, False), (2, 77, 2, 64, False, True),
                                                  (1, 257, 2, 80, True, False)])
def test_reference_is_sdpa_in_float64(B, T, H, dh, bias, causal):
    qkv, bk, bv = A.random_inputs(B, T, H, dh, bias, causal, 2.0, 5)
    want, absv = A.attention_ref(qkv, B, T, H, dh, bk, bv, causal)
    q, k, v = (t.permute(0, 2, 1, 3) for t in qkv.double().reshape(B, T, 3, H, dh).unbind(2))          # (B, H, T, dh)
    if bias:                                                                         # the bias pair, rounded, appended by hand as key T
        k = torch.cat([k, bk.bfloat16().double().reshape(1, H, 1, dh).expand(B, -1, -1, -1)], 2)
        v = torch.cat([v, bv.bfloat16().double().reshape(1, H, 1, dh).expand(B, -1, -1, -1)], 2)
    sdpa = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=causal).permute(0, 2, 1, 3).reshape(B * T, H * dh)
    assert sdpa.dtype == torch.float64
    torch.testing.assert_close(want, sdpa, rtol=1e-12, atol=1e-12)
    sdpa_abs = torch.nn.functional.scaled_dot_product_attention(q, k, v.abs(), is_causal=causal).permute(0, 2, 1, 3).reshape(B * T, H * dh)
    torch.testing.assert_close(absv, sdpa_abs, rtol=1e-12, atol=1e-12)
    assert bool((absv >= want.abs() - 1e-12).all())


def test_planted_keys_sit_on_both_sides_of_every_tile_boundary():
    assert A.planted_keys(97, 97) == [31, 32, 63, 64, 95, 96]
    assert A.planted_keys(96, 96) == [31, 32, 63, 64, 95]
    assert A.planted_keys(96, 97) == [31, 32, 63, 64, 95]            # key 96 is the bias position
    assert A.planted_keys(31, 32) == [30]
    # a planted key scores what the best random key of its query scores (up to the bf16 rounding of the key)
    c = A.case(A.by_label("value", "B=2,T=97,H=3,dh=64,scale=6"))
    q, k = (t.double() for t in c.qkv.reshape(c.B, c.T, 3, c.H, c.dh).unbind(2)[:2])
    s = torch.einsum("bihd,bjhd->bhij", q, k)
    planted = A.planted_keys(97, 97)
    rest = [j for j in range(97) if j not in planted]
    for j in planted:
        best_of_the_planted = s[:, :, :, j].max(dim=-1)
        best_random = s[:, :, :, rest].max(dim=-1).values.gather(-1, best_of_the_planted.indices.unsqueeze(-1)).squeeze(-1)
        assert bool(((best_of_the_planted.values / best_random - 1).abs() < 2.0 ** -7).all()), j


# ---- 2. coverage ----------------------------------------------------------------------------------------------------------
def _routes(pred=lambda s: True, groups=("value", "route")):
    return [s for g in groups for s in A.specs(g) if pred(s)]


def test_the_table_reaches_every_route_and_edge():
    inst = lambda s: s.route[0]
    q_parts, even, r8, coop = (lambda s: s.route[1]), (lambda s: s.route[2]), (lambda s: s.route[3]), (lambda s: s.route[4])
    for group in ("value", "onehot"):
        g = (group,)
        assert {inst(s) for s in _routes(groups=g)} == {(64, 3), (64, 8), (80, 9)}
        assert {inst(s) for s in _routes(lambda s: s.causal, g)} == {(64, 3), (64, 8), (80, 9)}
        # both sides of the 96 / 97 key switch, with and without the bias position, and causal
        assert {(s.Lk, s.bias, s.causal, inst(s)) for s in _routes(lambda s: s.dh == 64 and s.Lk in (96, 97), g)} == {
            (96, False, False, (64, 3)), (97, False, False, (64, 8)), (96, True, False, (64, 3)), (97, True, False, (64, 8)),
            (96, False, True, (64, 3)), (97, False, True, (64, 8))}
        # Lk at and one past every tile and chunk edge
        for dh, edges in ((64, (32, 64, 96, 128, 192, 256)), (80, (32, 96, 256, 288))):
            lks = {s.Lk for s in _routes(lambda s: s.dh == dh and not s.causal, g)}
            assert set(edges) <= lks and {e + 1 for e in edges if e + 1 <= (256 if dh == 64 else 288)} <= lks, (dh, sorted(lks))
        # each capacity limit, reached with and without the bias position
        assert {(s.dh, s.bias) for s in _routes(lambda s: s.Lk == (256 if s.dh == 64 else 288) and not s.causal, g)} == {
            (64, False), (64, True), (80, False), (80, True)}
        assert _routes(lambda s: s.dh == 80 and s.T == 288 and s.causal, g) and _routes(lambda s: s.dh == 64 and s.T == 256 and s.causal, g)
        # the cooperative query: with and without bias; switched off by causal; T 258 has nine query tiles and no coop
        assert {s.bias for s in _routes(coop, g)} == {False, True} and all(s.T == 257 and s.dh == 80 for s in _routes(coop, g))
        assert _routes(lambda s: s.T == 257 and s.causal and not coop(s), g)
        assert _routes(lambda s: s.T == 258 and not coop(s), g)
        assert {q_parts(s) for s in _routes(groups=g)} == {1, 2}
        assert {s.T for s in _routes(lambda s: s.T in (128, 129), g)} == {128, 129}
        assert {s.B for s in _routes(groups=g)} == {1, 2} and {s.H for s in _routes(groups=g)} == {2, 3}
    assert {s.scale for s in A.specs("value")} == {1.0, 6.0}

    rt = ("route",)
    assert {q_parts(s) for s in _routes(groups=rt)} == {1, 2}
    assert _routes(lambda s: even(s) and r8(s) == 0, rt) and _routes(lambda s: even(s) and r8(s) != 0, rt)
    assert {inst(s) for s in _routes(lambda s: even(s) and r8(s) != 0, rt)} == {(64, 8), (80, 9)}
    assert _routes(lambda s: even(s) and r8(s) != 0 and s.bias, rt) and _routes(lambda s: even(s) and s.causal, rt)
    # legacy map (no even map): a second round of samples (n / H >= 1 <=> B > 8) together with padding blocks (B % 8 != 0)
    legacy = _routes(lambda s: not even(s) and s.B > 8 and s.B % 8 != 0, rt)
    assert {inst(s) for s in legacy} == {(64, 3), (80, 9)} and any(s.causal for s in legacy) and any(s.B > 16 for s in legacy)
    # the thresholds, straddled: B 8 / 9 at H 16 with T > 128 (split <-> even map), T 128 / 129 (legacy <-> the other two)
    for T, dh in ((257, 80), (129, 64)):
        pair = {s.B: (q_parts(s), even(s)) for s in _routes(lambda s: s.T == T and s.H == 16 and s.dh == dh, rt)}
        assert pair == {8: (2, False), 9: (1, True)}, pair
    assert {coop(s) for s in _routes(lambda s: s.T == 257, rt)} == {True}
    assert _routes(lambda s: s.T == 128 and not even(s) and q_parts(s) == 1, rt) and _routes(lambda s: s.T == 129 and even(s), rt)
    assert [(s.B * s.H, r8(s)) for s in _routes(lambda s: s.T == 229, rt)] == [(108, 4)]
    # the cost bound of the GPU module: about 300 workgroups at most
    for s in A.all_specs():
        grid = s.B * s.H if even(s) else 8 * ((s.B + 7) // 8) * s.H * q_parts(s)
        assert grid <= 384, (s.label, grid)


def test_route_mirrors_the_refusals():
    for label, B, T, H, dh, bk, bv, causal in A.REJECTED:
        if bk == bv:
            assert A.route(B, T, H, dh, bk, causal) is None, label
    assert A.route(1, 256, 2, 64, False, False) is not None and A.route(1, 288, 2, 80, False, False) is not None


def test_one_hot_constructions_hold():
    """The builder asserts the 30-nat lead and the exact pick of the float64 reference; building every case runs those."""
    for s in A.specs("onehot"):
        c = A.case(s)
        A.check(c, A.to_bf16(c.want))
        assert c.picked.shape == (s.B * s.T, s.H * s.dh)


# ---- 3. mutants -----------------------------------------------------------------------------------------------------------
V, R, O = "value", "route", "onehot"
# (name, the wrong arguments as a function of the case, the cases that must catch it: (group, label up to the route tag))
MUTANTS = [
    ("last key dropped", lambda c: dict(keys=c.Lk - 1),
     [(V, "B=2,T=33,H=3,dh=64,scale=6"), (V, "B=1,T=256,H=3,dh=64,scale=6"), (V, "B=2,T=257,H=2,dh=80,scale=6"), (V, "B=1,T=288,H=2,dh=80,scale=1"),
      (O, "B=2,T=257,H=2,dh=80"), (O, "B=2,T=97,H=3,dh=64"), (R, "B=9,T=257,H=16,dh=80,scale=1")]),
    ("bias position dropped", lambda c: dict(use_bias=False),
     [(V, "B=2,T=31,H=3,dh=64,bias,scale=6"), (V, "B=1,T=96,H=3,dh=64,bias,scale=1"), (V, "B=2,T=255,H=3,dh=64,bias,scale=6"),
      (V, "B=2,T=257,H=2,dh=80,bias,scale=6"), (V, "B=2,T=287,H=2,dh=80,bias,scale=1"), (O, "B=2,T=257,H=2,dh=80,bias"),
      (O, "B=1,T=32,H=3,dh=64,bias"), (R, "B=9,T=229,H=12,dh=64,bias,scale=1")]),
    ("bias_v replaced by zeros", lambda c: dict(use_bias_v=False),
     [(V, "B=2,T=31,H=3,dh=64,bias,scale=6"), (V, "B=2,T=255,H=3,dh=64,bias,scale=1"), (V, "B=2,T=257,H=2,dh=80,bias,scale=6"),
      (O, "B=2,T=287,H=2,dh=80,bias"), (R, "B=9,T=229,H=12,dh=64,bias,scale=1")]),
    # distinguishable at scale 6 only: the planted bias_k ties with the best random key at a score of about 90 nats, and the
    # rounding moves that score by up to 2^-9 of itself -- 0.18 nats, several percent of the weight
    ("bias_k not rounded to bf16", lambda c: dict(round_bias_k=False),
     [(V, "B=2,T=255,H=3,dh=64,bias,scale=6"), (V, "B=2,T=257,H=2,dh=80,bias,scale=6")]),
    ("keys 96.. dropped", lambda c: dict(keys=96),
     [(V, "B=2,T=97,H=3,dh=64,scale=6"), (V, "B=1,T=96,H=3,dh=64,bias,scale=6"), (V, "B=2,T=97,H=2,dh=80,scale=1"),
      (V, "B=2,T=97,H=3,dh=64,causal,scale=6"), (O, "B=2,T=97,H=3,dh=64"), (O, "B=1,T=96,H=3,dh=64,bias")]),
    ("causal mask j <= i+1", lambda c: dict(causal_shift=1),
     [(V, "B=2,T=33,H=3,dh=64,causal,scale=1"), (V, "B=2,T=257,H=2,dh=80,causal,scale=1"), (O, "B=2,T=77,H=3,dh=64,causal"),
      (O, "B=2,T=97,H=3,dh=64,causal"), (O, "B=1,T=256,H=3,dh=64,causal"), (O, "B=1,T=288,H=2,dh=80,causal"),
      (R, "B=17,T=77,H=16,dh=64,causal,scale=1")]),
    ("causal mask j < i", lambda c: dict(causal_shift=-1),
     [(V, "B=1,T=32,H=3,dh=64,causal,scale=6"), (V, "B=2,T=257,H=2,dh=80,causal,scale=1"), (O, "B=1,T=32,H=3,dh=64,causal"),
      (O, "B=2,T=77,H=3,dh=64,causal"), (O, "B=2,T=257,H=2,dh=80,causal"), (R, "B=9,T=150,H=16,dh=64,causal,scale=1")]),
    ("samples walked in reverse order", lambda c: dict(reverse_samples=True),
     [(V, "B=2,T=33,H=3,dh=64,scale=1"), (V, "B=2,T=257,H=2,dh=80,scale=6"), (O, "B=2,T=129,H=3,dh=64")] +
     [(R, s.label.split("[")[0]) for s in A.specs("route")]),
    ("heads rotated by one", lambda c: dict(head_shift=1),
     [(V, "B=1,T=1,H=3,dh=64,scale=1"), (V, "B=2,T=258,H=2,dh=80,scale=6"), (O, "B=1,T=96,H=3,dh=64"),
      (R, "B=17,T=77,H=16,dh=64,causal,scale=1"), (R, "B=41,T=130,H=3,dh=80,scale=1")]),
    ("query T-1 answered with query T-2's row", lambda c: dict(last_query_from=c.T - 2),
     [(V, "B=2,T=257,H=2,dh=80,scale=1"), (V, "B=2,T=257,H=2,dh=80,bias,scale=6"), (V, "B=2,T=258,H=2,dh=80,scale=1"),
      (V, "B=2,T=33,H=3,dh=64,scale=6"), (V, "B=2,T=257,H=2,dh=80,causal,scale=6"), (O, "B=2,T=257,H=2,dh=80"),
      (R, "B=8,T=257,H=16,dh=80,scale=1"), (R, "B=9,T=257,H=16,dh=80,scale=1")]),
    ("scale 1/sqrt(dh) taken with the other dh", lambda c: dict(scale_dh=144 - c.dh),
     [(V, "B=2,T=33,H=3,dh=64,scale=1"), (V, "B=2,T=33,H=2,dh=80,scale=1"), (V, "B=2,T=257,H=2,dh=80,scale=6"),
      (V, "B=2,T=77,H=3,dh=64,causal,scale=1"), (R, "B=9,T=128,H=3,dh=80,scale=1"), (R, "B=8,T=129,H=16,dh=64,scale=1")]),
]
# "heads rotated" cannot show at H = 1 (route case B=131) and "scale with the other dh" not on the one-hot cases (a 30-nat lead
# stays one under either scale): neither is named above.


def _rejected(c, got):
    try:
        A.check(c, got)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name,wrong,caught_by", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_rejected_by_the_gpu_tests_comparison(name, wrong, caught_by):
    survived = []
    for group, start in caught_by:
        c = A.case(A.by_label(group, start))
        if not _rejected(c, A.to_bf16(_ref(c, **wrong(c)))):
            survived.append(c.label)
    assert not survived, f"'{name}' passes the comparison on {survived}"


@pytest.mark.parametrize("edge", [32, 64, 96, 128, 160, 192, 224, 256])
def test_a_key_duplicated_over_the_last_key_of_the_tile_before_it_is_rejected(edge):
    """Key 32 t copied over key 32 t - 1, one tile edge at a time: every random case with keys on both sides of that edge
    catches it at both scales, and so does every non-causal one-hot case in which key 32 t - 1 is the longest of its axis and
    every axis has a query: that axis loses its winner."""
    hit = [s for g in (V, R) for s in A.specs(g) if s.Lk > edge]
    assert len(hit) >= 4
    survived = [s.label for s in hit if not _rejected(A.case(s), A.to_bf16(_ref(A.case(s), dup_edges=(edge,))))]
    assert not survived, survived
    tops = [s for s in A.specs(O) if not s.causal and edge < s.Lk <= edge - 1 + s.dh and s.T >= s.dh]
    assert tops
    survived = [s.label for s in tops if not _rejected(A.case(s), A.to_bf16(_ref(A.case(s), dup_edges=(edge,))))]
    assert not survived, survived


def test_every_mutant_of_the_issue_is_listed():
    assert len(MUTANTS) == 11 and len({m[0] for m in MUTANTS}) == 11              # the twelfth, the duplicated key, is the test above
    for _, _, caught_by in MUTANTS:
        assert len(caught_by) >= 2


# ---- 4. the unchanged reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["value", "route"])
def test_the_unchanged_reference_stays_below_three_quarters_of_the_tolerance(group):
    """A condition on the inputs: the bf16 rounding of the exact result alone uses at most 2^-9 |want| of a tolerance that is at
    least 2^-8 |want|, and the rest is left to the kernel's rounding of P.  A case that fails this gets another seed."""
    worst = 0.0
    for s in A.specs(group):
        c = A.case(s)
        got = A.to_bf16(c.want)
        A.check(c, got)
        r = A.ratio(c, got)
        assert r <= 0.75, f"{c.label}: the rounded reference is at {r:.3f} of the tolerance"
        worst = max(worst, r)
    print(f"{group}: the rounded reference is at most at {worst:.3f} of the tolerance")


def test_the_comparison_rejects_nan_and_a_one_ulp_slip_of_a_one_hot_row():
    c = A.case(A.by_label(V, "B=2,T=33,H=3,dh=64,scale=1"))
    got = A.to_bf16(c.want)
    got[5, 7] = float("nan")
    assert _rejected(c, got)
    o = A.case(A.by_label(O, "B=2,T=33,H=3,dh=64"))
    got = o.picked.clone()
    got.view(torch.int16)[40, 3] += 1
    assert _rejected(o, got) and not _rejected(o, o.picked.clone())


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
P = 4096            # a non-null dummy address: a call that reached a launch with it would be a failed refusal
MESSAGE = {"bias_k without bias_v": b"go together", "bias_v without bias_k": b"go together", "B=0": b"bad shape", "T=0": b"bad shape",
           "H=0": b"bad shape", "B=0,causal": b"bad shape"}


@pytest.mark.parametrize("label,B,T,H,dh,bk,bv,causal", A.REJECTED, ids=[r[0] for r in A.REJECTED])
def test_attention_refuses_before_any_launch(label, B, T, H, dh, bk, bv, causal):
    from hippomm_amd import _lib
    lib = _lib.load()
    if causal:
        rc = lib.hmm_op_attention_causal_bf16(P, P, B, T, H, dh, None)
    else:
        rc = lib.hmm_op_attention_bf16(P, P, B, T, H, dh, P if bk else None, P if bv else None, None)
    err = lib.hmm_last_error()
    assert rc == -1 and MESSAGE.get(label, b"unsupported head_dim") in err, (rc, err)
