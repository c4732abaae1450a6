"""GPU: the packed text route -- every question through the text tower at its own length (hmm_encoder_forward_text_packed,
HipTower.__call__(pack=True), ImageBind(pack_text=True)) -- against the fp32 oracle and against the padded route.

Depth-2 text tower on the seeded random-init weights of test_text_tower_reduced_depth.  Bounds are the project's stated ones
(tests/test_gpu_encoder.py): cosine >= 1 - 5e-5 and |diff| <= 2e-3 on unit rows (text rows carry the logit scale 1 / 0.07).
The oracle runs once per module on the 17 questions below; nothing modifies its result.

Row thresholds of the dispatcher (encoder.hip): g_enc_splitk_rows = 700 total rows ends the few-row regime (fc2 as split-K reduced
in the next LayerNorm); g_enc_sliver_rows = 16448 total rows ends the sliver GEMM.  The bitwise tests stay inside (0, 700] or
inside (700, 16448]."""
import functools

import numpy as np
import pytest
import torch

import attention_cases as A
from oracle import imagebind_oracle as ib

pytestmark = pytest.mark.gpu

COS_TOL = 5e-5
ABS_TOL = 2e-3
SCALE = 1.0 / 0.07
SOT, EOS = 49406, 49407
FEW_ROWS = 700                                                   # g_enc_splitk_rows
SLIVER_ROWS = 16448                                              # g_enc_sliver_rows
EDGES = (1, 2, 3, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 76, 77)  # tile (32) and chunk (96) edges of the d_h = 64 short-key core
LENGTHS = EDGES + (2, 77)                                        # 17 questions; the last two are the batch that mixes 2 and 77


def _check(got, want, what=""):
    got, want = got.float().cpu(), want.float().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all()
    cos = torch.nn.functional.cosine_similarity(got, want, dim=1)
    err = (got - want).abs().max().item()
    print(f"{what}: rows {got.shape[0]}  min cos {cos.min().item():.7f}  max|diff| {err:.3e}")
    assert (1 - cos).max().item() <= COS_TOL
    assert err <= ABS_TOL * SCALE


def tokens(lengths, seed=0):
    """(B,77) ids: random tokens, EOS (the largest id) at position len - 1, zeros behind it."""
    tok = torch.randint(1, 49000, (len(lengths), 77), generator=torch.Generator().manual_seed(seed))
    for b, n in enumerate(lengths):
        tok[b, n - 1] = EOS
        tok[b, n:] = 0
    return tok


@functools.lru_cache(maxsize=None)
def _state():
    spec = ib.reduced(ib.TEXT_HUGE, 2)
    return spec, ib.synthetic_state(spec, seed=77, init="rich")


@functools.lru_cache(maxsize=None)
def _tower():
    from hippomm_amd.encoder import HipTower
    return HipTower("text", _state()[1], depth=2)


@functools.lru_cache(maxsize=None)
def _reference():
    """The 17 questions and the oracle's embeddings of them (computed once, never modified)."""
    spec, st = _state()
    tok = tokens(LENGTHS, seed=0)
    return tok, ib.text_forward(tok, st, spec)


# ---- parity with the fp32 oracle ---------------------------------------------------------------------------------------------
def test_one_question_at_every_tile_and_chunk_edge_vs_oracle():
    """B = 1: each of the 15 edge lengths alone (1 .. 77 rows: the few-row regime)."""
    tok, want = _reference()
    tower = _tower()
    got = torch.cat([tower(tok[i:i + 1], pack=True) for i in range(len(EDGES))])
    assert tower.text_stats == {"route": "packed", "rows_padded": 77, "rows_packed": EDGES[-1]}
    _check(got, want[:len(EDGES)], what="text packed depth2 B=1 x 15 lengths")


def test_a_batch_that_mixes_2_and_77_vs_oracle():
    tok, want = _reference()
    got = _tower()(tok[15:17], pack=True)
    assert _tower().text_stats["rows_packed"] == 79
    _check(got, want[15:17], what="text packed depth2 B=2 lengths (2, 77)")
    _check(_tower()(tok[[16, 15]], pack=True), want[[16, 15]], what="text packed depth2 B=2 lengths (77, 2)")


def test_seventeen_questions_of_all_edge_lengths_vs_oracle():
    """B = 17, 583 rows in all (few-row regime), two rounds of the attention block map; and the same 17 after 2 x 77 more rows
    (737 rows: the large regime)."""
    tok, want = _reference()
    assert sum(LENGTHS) == 583 <= FEW_ROWS
    got = _tower()(tok, pack=True)
    assert _tower().text_stats == {"route": "packed", "rows_padded": 17 * 77, "rows_packed": 583}
    _check(got, want, what="text packed depth2 B=17 few-row regime")
    more = torch.cat([tok, tok[[14, 14]]])
    assert FEW_ROWS < 583 + 154 <= SLIVER_ROWS
    _check(_tower()(more, pack=True)[:17], want, what="text packed depth2 B=19 large regime")


def test_full_depth_three_questions_vs_oracle():
    from hippomm_amd.encoder import HipTower
    st = ib.synthetic_state(ib.TEXT_HUGE, seed=5, init="survey")
    tok = tokens([4, 12, 77], seed=8)
    tok[0, :4] = torch.tensor([SOT, 320, 1125, EOS])
    want = ib.text_forward(tok, st)
    tower = HipTower("text", st)
    _check(tower(tok, pack=True), want, what="text packed full depth B=3")
    _check(tower(tok), want, what="text padded full depth B=3")


# ---- what stands behind EOS does not matter --------------------------------------------------------------------------------------
def test_tokens_behind_eos_do_not_change_a_bit():
    tok, _ = _reference()
    base = _tower()(tok, pack=True)
    g = torch.Generator().manual_seed(4)
    moved = tok.clone()
    for b, n in enumerate(LENGTHS):
        moved[b, n:] = torch.randint(0, EOS, (77 - n,), generator=g)
    assert not torch.equal(moved, tok)
    assert torch.equal(_tower()(moved, pack=True), base)
    assert torch.equal(_tower()(moved.cuda(), pack=True), base), "lengths read back from device ids"
    assert torch.equal(_tower()(tok, pack=True), base), "run to run"


# ---- batch invariance, bitwise, within a regime --------------------------------------------------------------------------------
def _ride(question, mates, position):
    """The question at `position` among its batch-mates -> its embedding from the packed forward of that batch."""
    batch = torch.cat([mates[:position], question, mates[position:]])
    return _tower()(batch, pack=True)[position:position + 1], int(_tower().text_stats["rows_packed"])


def test_a_question_keeps_its_bits_at_every_position_and_with_any_batch_mates_within_a_regime():
    question = tokens([9], seed=21)
    alone = _tower()(question, pack=True)
    few = [tokens([77] * 8, seed=22), tokens([1, 2, 3, 33, 64], seed=23), tokens([77] * 8 + [75], seed=24)]        # 625, 112, 700 rows
    for mates in few:
        for position in (0, len(mates) // 2, len(mates)):
            got, rows = _ride(question, mates, position)
            assert rows <= FEW_ROWS
            assert torch.equal(got, alone), f"few-row regime: {rows} rows, position {position}"
    large = [tokens([77] * 8 + [76], seed=25), tokens([5] * 150, seed=26), tokens([77] * 40 + [1, 31], seed=27)]    # 701, 759, 3121 rows
    first, _ = _ride(question, large[0], 0)
    for mates in large:
        for position in (0, len(mates) // 2, len(mates)):
            got, rows = _ride(question, mates, position)
            assert FEW_ROWS < rows <= SLIVER_ROWS
            assert torch.equal(got, first), f"large regime: {rows} rows, position {position}"
    # across the threshold only the fp32 summation order of fc2 differs: the stated tolerance, no equal bits asserted
    _check(first, alone, what="text packed depth2: large regime vs few-row regime")
    spec, st = _state()
    want = ib.text_forward(question, st, spec)
    _check(alone, want, what="text packed depth2 few-row regime vs oracle")
    _check(first, want, what="text packed depth2 large regime vs oracle")


# ---- the attention kernel on its own --------------------------------------------------------------------------------------------
def _softmax_attention_f64(qkv, T, H, dh):
    """numpy float64, one sample: causal softmax(q k^T / sqrt(dh)) v and softmax |v| per head, on the bf16 operands."""
    x = qkv.to(torch.float64).numpy().reshape(T, 3, H, dh)
    q, k, v = x[:, 0], x[:, 1], x[:, 2]
    want, absv = np.empty((T, H, dh)), np.empty((T, H, dh))
    visible = np.arange(T)[None, :] <= np.arange(T)[:, None]
    for h in range(H):
        s = q[:, h] @ k[:, h].T / np.sqrt(dh)
        s = np.where(visible, s, -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        want[:, h], absv[:, h] = p @ v[:, h], p @ np.abs(v[:, h])
    return torch.from_numpy(want.reshape(T, H * dh)), torch.from_numpy(absv.reshape(T, H * dh))


@pytest.mark.parametrize("scale", A.SCALES)
def test_packed_attention_kernel_vs_float64_softmax(scale):
    """hmm_op_attention_causal_packed_bf16 on 17 sequences of the edge lengths in one launch (three rounds of the block map with
    H = 3), at the tolerance of the attention-core tests (attention_cases.tolerance); the 77-row sequences equal
    hmm_op_attention_causal_bf16 bit for bit.  The output starts as NaN and carries one guard row behind its end."""
    from hippomm_amd import _lib as L
    lib = L.load()
    H, dh = 3, 64
    D = H * dh
    parts = [A.random_inputs(1, T, H, dh, False, True, scale, 1000 * T + i)[0] for i, T in enumerate(LENGTHS)]
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
    R = int(off[-1])
    qkv = torch.cat(parts).cuda()
    out = torch.full((R + 1, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    guard = out[R:].clone()
    off_dev = torch.from_numpy(off).cuda()
    L.check(lib.hmm_op_attention_causal_packed_bf16(qkv.data_ptr(), out.data_ptr(), off_dev.data_ptr(), len(LENGTHS), R, H, dh,
                                                    L.stream_ptr()), "hmm_op_attention_causal_packed_bf16")
    torch.cuda.synchronize()
    assert torch.equal(out[R:].view(torch.int16), guard.view(torch.int16)), "the row behind the output was written"
    got = out[:R].cpu()
    assert torch.isfinite(got.float()).all()
    worst = 0.0
    for i, T in enumerate(LENGTHS):
        want, absv = _softmax_attention_f64(parts[i], T, H, dh)
        ratio = ((got[off[i]:off[i + 1]].to(torch.float64) - want).abs() / A.tolerance(want, absv)).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"sequence {i} of {T} rows: worst error {ratio:.3f} of the tolerance"
        if T == 77:
            dense = torch.full((78, D), float("nan"), dtype=torch.bfloat16, device="cuda")
            L.check(lib.hmm_op_attention_causal_bf16(parts[i].cuda().data_ptr(), dense.data_ptr(), 1, 77, H, dh, L.stream_ptr()),
                    "hmm_op_attention_causal_bf16")
            torch.cuda.synchronize()
            assert torch.equal(dense[:77].cpu().view(torch.int16), got[off[i]:off[i + 1]].view(torch.int16)), \
                f"sequence {i}: 77 packed rows differ from the dense causal kernel"
    print(f"packed causal attention, scale {scale:g}: worst error {worst:.3f} of the tolerance")


# ---- from strings to hits -------------------------------------------------------------------------------------------------------
def _tokenizer(strings):
    """A stand-in for the CLIP BPE: SOT, one id per word (a fixed hash of the word into 1 .. 48999), EOS, zeros."""
    ids = torch.zeros(len(strings), 77, dtype=torch.int64)
    for b, text in enumerate(strings):
        words = [1 + sum(ord(ch) * 131 ** i for i, ch in enumerate(w)) % 48999 for w in text.split()]
        row = [SOT] + words + [EOS]
        ids[b, :len(row)] = torch.tensor(row)
    return ids


def _store_for(unit, seed):
    """64 unit rows whose cosine with `unit` is planted: 0.90 0.85 0.80 0.75 0.70 | 0.60 and below."""
    g = torch.Generator().manual_seed(seed)
    planted = [0.90, 0.85, 0.80, 0.75, 0.70, 0.60] + [0.5 - 0.008 * i for i in range(58)]
    noise = torch.randn(64, 1024, generator=g, dtype=torch.float64)
    u = unit.to(torch.float64)
    noise = noise - (noise @ u)[:, None] * u
    noise = noise / noise.norm(dim=1, keepdim=True)
    c = torch.tensor(planted, dtype=torch.float64)[:, None]
    rows = c * u + (1 - c * c).sqrt() * noise
    order = torch.randperm(64, generator=g)
    return rows[order].to(torch.float32).numpy()


def test_pack_text_from_strings_to_the_same_top_five_hits():
    from hippomm_amd.encoder import ImageBind, text_lengths
    from hippomm_amd.vector_ops import top_k_cosine_similarity
    spec, st = _state()
    strings = ["a red bicycle", "who opened the door", "dog", "the cat sat on the warm window sill all afternoon"]
    ids = _tokenizer(strings)
    lengths = text_lengths(ids)
    assert lengths.tolist() == [5, 6, 3, 12]
    want = ib.text_forward(ids, st, spec)
    unit = want / want.norm(dim=1, keepdim=True)
    stores, tops = [], []
    for q in range(len(strings)):                                # the gap is checked on the ORACLE's embedding: no luck, no tie
        store = _store_for(unit[q], seed=40 + q)
        sims = np.sort((store / np.linalg.norm(store, axis=1, keepdims=True)) @ unit[q].numpy())[::-1]
        assert sims[4] - sims[5] >= 1e-3 and np.all(sims[:4] - sims[1:5] >= 1e-3), sims[:7]
        stores.append(store)
        tops.append(np.argsort(-(store @ unit[q].numpy()))[:5].tolist())
    model = ImageBind(state_dict=st, towers=("text",), depth={"text": 2}, tokenizer=_tokenizer, pack_text=True)
    stats = {}
    packed = model.extract_features({"text": strings}, ["text"], stats=stats)["text"]
    assert stats == {"route": "packed", "rows_padded": 4 * 77, "rows_packed": int(lengths.sum())} and model.text_stats == stats
    model.pack_text = False
    stats = {}
    padded = model.extract_features({"text": strings}, ["text"], stats=stats)["text"]
    assert stats["route"] == "padded" and stats["rows_padded"] == 4 * 77
    _check(packed, want, what="text packed depth2 from strings")
    _check(padded, want, what="text padded depth2 from strings")
    for q in range(len(strings)):
        hits_packed, _ = top_k_cosine_similarity(packed[q], stores[q], 5)
        hits_padded, _ = top_k_cosine_similarity(padded[q], stores[q], 5)
        assert list(hits_packed) == list(hits_padded) == tops[q], (q, list(hits_packed), list(hits_padded), tops[q])


def test_without_the_keyword_the_padded_route_is_taken():
    tok, _ = _reference()
    tower = _tower()
    plain = tower(tok[:3])
    assert tower.text_stats == {"route": "padded", "rows_padded": 3 * 77, "rows_packed": None}
    out = torch.empty(3, 1024, device="cuda")
    tower.forward_into(tok[:3].cuda(), out)
    assert torch.equal(out, plain)


# ---- stream capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [(9,), (77,) * 9 + (5, 9, 12)], ids=["few-row", "large"])
def test_packed_forward_is_graph_capturable(lengths):
    """One capture and one replay of a packed forward equal the eager result; the lengths (launch sizes) are baked into the graph,
    the ids and the table are read from the device at replay."""
    from hippomm_amd.encoder import text_lengths
    tower = _tower()
    tok = tokens(lengths, seed=31)
    host_lengths = text_lengths(tok)
    x = tok.cuda()
    table = tower.upload_text_table(host_lengths)
    out = torch.empty(len(lengths), 1024, device="cuda")
    eager = tower(x, pack=True)                                  # also warms up (LDS attributes, workspace) outside the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tower.forward_text_packed_into(x, host_lengths, table, out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tower.forward_text_packed_into(x, host_lengths, table, out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(tokens(lengths, seed=32).cuda())                     # new questions of the same lengths, same graph
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, tower(x, pack=True))
