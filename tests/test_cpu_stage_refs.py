"""CPU: the stage tests can fail.  No kernel runs here.

1. Mutants.  Each wrong variant of a reference in tests/stage_refs.py -- one argument changed -- goes through the inputs and the
   comparison function of tests/test_gpu_stage_ops.py (both live in tests/stage_cases.py), cast to the type the kernel
   delivers; the comparison must reject it on every case the mutation applies to.  The unchanged reference must pass.
   A mutant that survived would mean the inputs cannot tell that mistake from the right stage.
2. Refusals.  Every new hmm_op_* wrapper refuses null pointers and bad counts with HMM_E_INVALID before any launch.
3. eps at the call sites.  tests/eps_oracle.py equals the oracle with the code base's eps values, and at every small-signal
   case of tests/test_gpu_encoder.py the other eps at any one pinned site moves it by >= 4x that file's tolerance.
"""
import math

import pytest
import torch

import eps_oracle as E
import stage_cases as S
import stage_refs as R
from oracle import imagebind_oracle as ib


def _always(c):
    return True


def _asm(**kw):
    return lambda c: R.assemble_tokens(c.patches, c.cls, c.pos, c.stem, c.pre, c.n_img, c.T, **kw)


def _asm_eps(which, eps):
    def f(c):
        stem, pre = c.stem, c.pre
        if which == "stem":
            stem = (stem[0], stem[1], eps)
        else:
            pre = (pre[0], pre[1], eps)
        return R.assemble_tokens(c.patches, c.cls, c.pos, stem, pre, c.n_img, c.T)
    return f


def _attn(**kw):
    return lambda c: R.attention_cls(c.q, c.kv, c.B, c.T, c.H, c.dh, c.bk, c.bv, **kw)


def _l2(**kw):
    return lambda c: R.l2norm_rows(c.v, c.n_out, c.clips, None if c.log_scale is None else float(c.log_scale), **kw)


def _l2_nan_through_the_floor(c):
    """fmaxf(NaN, 1e-12) is 1e-12: what l2norm_rows_kernel computed before it was corrected -- the NaN stays in its column and the
    rest of the row is x * scale / 1e-12 instead of NaN."""
    x = c.v.to(torch.float64).reshape(c.n_out, c.clips, -1)
    n = x.norm(dim=-1, keepdim=True)
    n = torch.where(torch.isnan(n), torch.full_like(n, 1e-12), n.clamp_min(1e-12))
    scale = 1.0 if c.log_scale is None else min(math.exp(float(c.log_scale)), 100.0)
    return (x / n * scale).mean(dim=1)


_low = lambda c: "low-variance" in c.label
# (stage, mutant, the wrong reference as a function of the case, the cases it must be rejected on)
MUTANTS = [
    ("im2col_vision", "dy and dx swapped", lambda c: R.im2col_vision(c.frames, order=("c", "dx", "dy")), _always),
    ("im2col_vision", "channel innermost", lambda c: R.im2col_vision(c.frames, order=("dy", "dx", "c")), _always),
    ("im2col_vision", "column 587 reads 0", lambda c: R.im2col_vision(c.frames, zero_columns=(587,)), _always),
    ("im2col_vision", "patch index off by one", lambda c: R.im2col_vision(c.frames, patch_shift=1), _always),
    ("im2col_vision", "pad column 588 holds data", lambda c: torch.cat([R.im2col_vision(c.frames)[:, :588], R.im2col_vision(c.frames)[:, :52]], 1), _always),
    ("im2col_audio", "dy and dx swapped", lambda c: R.im2col_audio(c.mels, order=("dx", "dy")), _always),
    ("im2col_audio", "stride 9", lambda c: R.im2col_audio(c.mels, stride=9), _always),
    ("im2col_audio", "patch index off by one", lambda c: R.im2col_audio(c.mels, patch_shift=1), _always),
    ("fold_conv3d", "tap 0 used twice", lambda c: R.fold_conv3d(c.w, taps=(0, 0)), _always),
    ("fold_conv3d", "tap 1 used twice", lambda c: R.fold_conv3d(c.w, taps=(1, 1)), _always),
    ("embed_tokens", "upper clamp off by one", lambda c: R.embed_tokens(c.ids, c.table, c.pos, c.T, hi=c.vocab - 2), _always),
    ("embed_tokens", "lower clamp off by one", lambda c: R.embed_tokens(c.ids, c.table, c.pos, c.T, lo=1), _always),
    ("embed_tokens", "pos[t-1] for pos[t]", lambda c: R.embed_tokens(c.ids, c.table, c.pos, c.T, pos_shift=-1), _always),
    ("gather_rows", "rows taken as packed", lambda c: R.gather_rows(c.src, c.row_bytes, c.n_rows, c.row_bytes), lambda c: c.n_rows > 1),
    ("gather_rows", "16-byte pieces of a row rotated", lambda c: torch.roll(R.gather_rows(c.src, c.stride, c.n_rows, c.row_bytes), 16, dims=1), _always),
    ("assemble_tokens", "stem eps 1e-6", _asm_eps("stem", 1e-6), lambda c: c.stem is not None and _low(c)),
    ("assemble_tokens", "pre eps 1e-5", _asm_eps("pre", 1e-5), lambda c: c.pre is not None and _low(c)),
    ("assemble_tokens", "stem and pre eps swapped", lambda c: R.assemble_tokens(c.patches, c.cls, c.pos, (c.stem[0], c.stem[1], c.pre[2]),
                                                                                 (c.pre[0], c.pre[1], c.stem[2]), c.n_img, c.T),
     lambda c: c.stem is not None and c.pre is not None and _low(c)),
    ("assemble_tokens", "cls row takes the stem LayerNorm", _asm(cls_takes_stem=True), lambda c: c.stem is not None),
    ("assemble_tokens", "pos[t-1] for pos[t]", _asm(pos_shift=1), _always),
    ("assemble_tokens", "patch index off by one", _asm(patch_shift=1), _always),
    ("layernorm_eos", "last occurrence of the largest id", lambda c: R.layernorm_eos(c.x, c.ids, c.gamma, c.beta, S.LN_EPS, pick="last"),
     lambda c: c.T > 1),
    ("attention_cls", "last key dropped", lambda c: _attn(keys=c.T + (c.bk is not None) - 1)(c), lambda c: c.T > 1),
    ("attention_cls", "bias_v dropped", _attn(use_bias_v=False), lambda c: c.bk is not None),
    ("l2norm_rows", "mean before the normalise", _l2(mean_first=True), lambda c: c.clips > 1),
    ("l2norm_rows", "logit scale without the clamp", _l2(clamp=math.inf), lambda c: "log200" in c.label),
    ("l2norm_rows", "no floor under the norm", _l2(floor=0.0), lambda c: c.n_out == 5),
    ("l2norm_rows", "a NaN norm replaced by the floor", _l2_nan_through_the_floor, lambda c: c.n_out == 5),
]
# Equivalent mutants, on purpose not in the list: "last key dropped" at T = 1 without a bias position leaves no key at all, and
# "last occurrence" at T = 1 is the first.  layernorm_eos has no eps mutant: eps is an argument of the entry point, the rows of
# its cases have variance 9, and the literal the tower passes there is pinned end to end (part 3 below).


@pytest.mark.parametrize("stage", S.STAGES)
def test_the_unchanged_reference_passes_its_own_comparison(stage):
    for c in S.cases(stage):
        S.check(stage, c, S.cast_result(stage, c.want))


@pytest.mark.parametrize("stage,name,wrong,applies", MUTANTS, ids=[f"{m[0]}: {m[1]}" for m in MUTANTS])
def test_mutant_is_rejected_by_the_gpu_tests_comparison(stage, name, wrong, applies):
    hit = [c for c in S.cases(stage) if applies(c)]
    assert hit, "the mutant applies to no case"
    survived = []
    for c in hit:
        try:
            S.check(stage, c, S.cast_result(stage, wrong(c)))
        except AssertionError:
            continue
        survived.append(c.label)
    assert not survived, f"'{name}' passes the comparison of {stage} on {survived}"


def test_every_stage_has_mutants():
    assert {m[0] for m in MUTANTS} == set(S.STAGES)


def test_layernorm_eos_cases_select_what_their_labels_say():
    main = S.cases("layernorm_eos")[0]
    assert [R.eos_position(main.ids[b]) for b in range(main.B)] == [0, 76, 70, 6, 5, 0]
    odd = S.cases("layernorm_eos")[1]
    assert (odd.ids[0] < 0).all() and R.eos_position(odd.ids[0]) == 40


# ---- 2. refusals --------------------------------------------------------------------------------------------------------
P = 4096            # a non-null dummy address: a call that reached a launch with it would be a failed refusal


def _refusals():
    f = 1e-6
    return [
        ("hmm_op_im2col_vision_bf16", (None, P, 1, None), b"null"), ("hmm_op_im2col_vision_bf16", (P, None, 1, None), b"null"),
        ("hmm_op_im2col_vision_bf16", (P, P, 0, None), b"positive"),
        ("hmm_op_im2col_audio_bf16", (None, P, 1, None), b"null"), ("hmm_op_im2col_audio_bf16", (P, None, 1, None), b"null"),
        ("hmm_op_im2col_audio_bf16", (P, P, -3, None), b"positive"),
        ("hmm_op_fold_conv3d_bf16", (None, P, 5, None), b"null"), ("hmm_op_fold_conv3d_bf16", (P, None, 5, None), b"null"),
        ("hmm_op_fold_conv3d_bf16", (P, P, 0, None), b"positive"),
        ("hmm_op_assemble_tokens", (None, P, P, P, P, f, P, P, f, P, 1, 257, 1280, None), b"null"),
        ("hmm_op_assemble_tokens", (P, None, P, P, P, f, P, P, f, P, 1, 257, 1280, None), b"null"),
        ("hmm_op_assemble_tokens", (P, P, None, P, P, f, P, P, f, P, 1, 257, 1280, None), b"null"),
        ("hmm_op_assemble_tokens", (P, P, P, P, P, f, P, P, f, None, 1, 257, 1280, None), b"null"),
        ("hmm_op_assemble_tokens", (P, P, P, P, None, f, P, P, f, P, 1, 257, 1280, None), b"stem gamma and beta"),
        ("hmm_op_assemble_tokens", (P, P, P, None, P, f, P, P, f, P, 1, 257, 1280, None), b"stem gamma and beta"),
        ("hmm_op_assemble_tokens", (P, P, P, P, P, f, None, P, f, P, 1, 257, 1280, None), b"pre gamma and beta"),
        ("hmm_op_assemble_tokens", (P, P, P, P, P, f, P, None, f, P, 1, 257, 1280, None), b"pre gamma and beta"),
        ("hmm_op_assemble_tokens", (P, P, P, P, P, f, P, P, f, P, 0, 257, 1280, None), b"positive"),
        ("hmm_op_assemble_tokens", (P, P, P, P, P, f, P, P, f, P, 1, 0, 1280, None), b"positive"),
        ("hmm_op_assemble_tokens", (P, P, P, None, None, f, None, None, f, P, 1, 257, 1024, None), b"D must be 768 or 1280"),
        ("hmm_op_layernorm_strided_bf16", (None, 1280, P, P, P, 1, 1280, f, None), b"null"),
        ("hmm_op_layernorm_strided_bf16", (P, 1280, None, P, P, 1, 1280, f, None), b"null"),
        ("hmm_op_layernorm_strided_bf16", (P, 1280, P, None, P, 1, 1280, f, None), b"null"),
        ("hmm_op_layernorm_strided_bf16", (P, 1280, P, P, None, 1, 1280, f, None), b"null"),
        ("hmm_op_layernorm_strided_bf16", (P, 1280, P, P, P, 0, 1280, f, None), b"positive"),
        ("hmm_op_layernorm_strided_bf16", (P, 1276, P, P, P, 2, 1280, f, None), b"below D"),
        ("hmm_op_layernorm_strided_bf16", (P, 1282, P, P, P, 2, 1280, f, None), b"multiple of 4"),
        ("hmm_op_layernorm_strided_bf16", (P, 2000, P, P, P, 2, 1000, f, None), b"D must be 768, 1024 or 1280"),
        ("hmm_op_gather_rows", (None, 5120, P, 1, 2560, None), b"null"), ("hmm_op_gather_rows", (P, 5120, None, 1, 2560, None), b"null"),
        ("hmm_op_gather_rows", (P, 5120, P, 0, 2560, None), b"positive"), ("hmm_op_gather_rows", (P, 5120, P, 1, 0, None), b"positive"),
        ("hmm_op_gather_rows", (P, 5120, P, 2, 2568, None), b"multiple of 16"),
        ("hmm_op_gather_rows", (P, 2544, P, 2, 2560, None), b"below row_bytes"),
        ("hmm_op_gather_rows", (P, 2568, P, 2, 2560, None), b"multiple of 16"),
        ("hmm_op_attention_cls_bf16", (None, P, P, 1, 229, 12, 64, None, None, None), b"null"),
        ("hmm_op_attention_cls_bf16", (P, None, P, 1, 229, 12, 64, None, None, None), b"null"),
        ("hmm_op_attention_cls_bf16", (P, P, None, 1, 229, 12, 64, None, None, None), b"null"),
        ("hmm_op_attention_cls_bf16", (P, P, P, 1, 229, 12, 64, P, None, None), b"go together"),
        ("hmm_op_attention_cls_bf16", (P, P, P, 1, 229, 12, 64, None, P, None), b"go together"),
        ("hmm_op_attention_cls_bf16", (P, P, P, 0, 229, 12, 64, None, None, None), b"bad shape"),
        ("hmm_op_attention_cls_bf16", (P, P, P, 1, 0, 12, 64, None, None, None), b"bad shape"),
        ("hmm_op_attention_cls_bf16", (P, P, P, 1, 229, 0, 64, None, None, None), b"bad shape"),
        ("hmm_op_attention_cls_bf16", (P, P, P, 1, 321, 12, 64, None, None, None), b"exceed 320"),
        ("hmm_op_attention_cls_bf16", (P, P, P, 1, 320, 12, 64, P, P, None), b"exceed 320"),
        ("hmm_op_attention_cls_bf16", (P, P, P, 1, 229, 12, 72, None, None, None), b"head_dim"),
        ("hmm_op_embed_tokens", (None, P, P, P, 77, 77, 50, None), b"null"), ("hmm_op_embed_tokens", (P, None, P, P, 77, 77, 50, None), b"null"),
        ("hmm_op_embed_tokens", (P, P, None, P, 77, 77, 50, None), b"null"), ("hmm_op_embed_tokens", (P, P, P, None, 77, 77, 50, None), b"null"),
        ("hmm_op_embed_tokens", (P, P, P, P, 0, 77, 50, None), b"positive"), ("hmm_op_embed_tokens", (P, P, P, P, 77, 0, 50, None), b"positive"),
        ("hmm_op_embed_tokens", (P, P, P, P, 77, 77, 0, None), b"positive"),
        ("hmm_op_layernorm_eos_bf16", (None, P, 77, P, P, P, 1, 1024, f, None), b"null"),
        ("hmm_op_layernorm_eos_bf16", (P, None, 77, P, P, P, 1, 1024, f, None), b"null"),
        ("hmm_op_layernorm_eos_bf16", (P, P, 77, None, P, P, 1, 1024, f, None), b"null"),
        ("hmm_op_layernorm_eos_bf16", (P, P, 77, P, None, P, 1, 1024, f, None), b"null"),
        ("hmm_op_layernorm_eos_bf16", (P, P, 77, P, P, None, 1, 1024, f, None), b"null"),
        ("hmm_op_layernorm_eos_bf16", (P, P, 0, P, P, P, 1, 1024, f, None), b"positive"),
        ("hmm_op_layernorm_eos_bf16", (P, P, 77, P, P, P, 0, 1024, f, None), b"positive"),
        ("hmm_op_layernorm_eos_bf16", (P, P, 77, P, P, P, 1, 512, f, None), b"D must be 768, 1024 or 1280"),
        ("hmm_op_l2norm_rows", (None, P, 1, 1, None, None), b"null"), ("hmm_op_l2norm_rows", (P, None, 1, 1, None, None), b"null"),
        ("hmm_op_l2norm_rows", (P, P, 0, 1, None, None), b"positive"), ("hmm_op_l2norm_rows", (P, P, 1, 0, None, None), b"positive"),
    ]


def test_every_new_wrapper_refuses_bad_arguments_without_a_launch():
    from hippomm_amd import _lib
    lib = _lib.load()
    seen = set()
    for entry, args, message in _refusals():
        rc = getattr(lib, entry)(*args)
        err = lib.hmm_last_error()
        assert rc == -1 and message in err, f"{entry}{args}: status {rc}, message {err!r}, expected {message!r}"
        seen.add(entry)
    new = {"hmm_op_im2col_vision_bf16", "hmm_op_im2col_audio_bf16", "hmm_op_fold_conv3d_bf16", "hmm_op_assemble_tokens",
           "hmm_op_layernorm_strided_bf16", "hmm_op_gather_rows", "hmm_op_attention_cls_bf16", "hmm_op_embed_tokens",
           "hmm_op_layernorm_eos_bf16", "hmm_op_l2norm_rows"}
    assert seen == new


# ---- 3. eps at the call sites -------------------------------------------------------------------------------------------
COS_TOL, ABS_TOL = 5e-5, 2e-3        # tests/test_gpu_encoder.py


@pytest.mark.parametrize("label", E.SMALL_SIGNAL)
def test_small_signal_case_moves_by_4x_the_tolerance_under_a_wrong_eps(label):
    name, spec, st, x, sites = E.small_signal_case(label)
    base = E.forward(name, x, st, spec)
    assert torch.equal(base, ib.forward({name: x}, {name: st}, {name: spec})[name]), "the parametrised copy is not the oracle"
    assert sites
    for site in sites:
        moved = E.forward(name, x, st, spec, E.wrong_eps(site))
        cos = torch.nn.functional.cosine_similarity(moved, base, dim=1)
        by = max((1 - cos).max().item() / COS_TOL, (moved - base).abs().max().item() / (ABS_TOL * E.TOL_SCALE[name]))
        print(f"{label}: eps {E.wrong_eps(site)[site]:g} at {site} moves the oracle by {by:.1f}x the tolerance")
        assert by >= 4.0, f"{label}: a wrong eps at {site} moves the embedding by only {by:.2f}x the tolerance"


def test_tolerance_constants_are_those_of_the_encoder_tests():
    import test_gpu_encoder as T
    assert (T.COS_TOL, T.ABS_TOL) == (COS_TOL, ABS_TOL)
