"""CPU: the host side of the packed text route (every question through the text tower at its own length).

  * hippomm_amd.encoder.text_lengths / text_offsets: len = (first index of the row's largest id) + 1, the EOS rule of the tower's
    head, and the exclusive prefix sum that is the device table of hmm_encoder_forward_text_packed;
  * the C entry: declared, exported, bound, ABI version unchanged, and every refusal that needs no device reported as a status
    code on a host without a GPU (dummy non-null pointers, as tests/test_cpu_audio_levels_abi.py passes them);
  * the premise of the route, on the fp32 oracle and not on our argument: the tokens behind EOS never change an embedding."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import imagebind_oracle as ib

ROOT = Path(__file__).resolve().parent.parent
HMM_OK, HMM_E_INVALID = 0, -1
ONE = 1 << 20                                                    # 16-byte aligned non-null dummies, far from each other
FAR = 1 << 40
SOT, EOS = 49406, 49407


def _rows():
    """(ids row, length) for the edge rows of the EOS rule."""
    rows = []
    r = np.zeros(77, np.int64); r[0] = EOS; rows.append((r, 1))                                  # EOS at position 0
    r = np.zeros(77, np.int64); r[:2] = (SOT, EOS); rows.append((r, 2))                          # [SOT, EOS]
    r = np.arange(1, 78, dtype=np.int64); r[0] = SOT - 1000; r[76] = EOS; rows.append((r, 77))   # EOS at 76
    r = np.zeros(77, np.int64); r[0] = SOT; r[5] = EOS; r[9] = EOS; rows.append((r, 6))          # two equal maxima: the first wins
    rows.append((np.zeros(77, np.int64), 1))                                                     # a row of zeros
    return rows


def test_lengths_follow_the_eos_rule_at_its_edges():
    from hippomm_amd.encoder import text_lengths
    ids = np.stack([r for r, _ in _rows()])
    want = np.array([n for _, n in _rows()], dtype=np.int32)
    for given in (ids, torch.from_numpy(ids), ids.tolist()):
        got = text_lengths(given)
        assert got.dtype == np.int32 and got.tolist() == want.tolist()
    for i, (row, n) in enumerate(_rows()):                       # one at a time: no dependence on the batch
        assert text_lengths(row[None]).tolist() == [n], i
    with pytest.raises(ValueError):
        text_lengths(np.zeros((2, 76), np.int64))


def test_offsets_are_the_exclusive_prefix_sum_with_the_total_behind():
    from hippomm_amd.encoder import text_lengths, text_offsets
    ids = np.stack([r for r, _ in _rows()])
    off = text_offsets(text_lengths(ids))
    assert off.dtype == np.int32 and off.tolist() == [0, 1, 3, 80, 86, 87]
    assert text_offsets([77] * 3).tolist() == [0, 77, 154, 231]
    assert text_offsets([1]).tolist() == [0, 1]
    for bad in ([0], [78], [5, -1], [3, 77, 100]):
        with pytest.raises(ValueError):
            text_offsets(bad)


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(str(build.build()))
    for name in ("hmm_encoder_text_packed_workspace_bytes", "hmm_encoder_forward_text_packed", "hmm_op_attention_causal_packed_bf16"):
        assert name in declared and hasattr(lib, name) and name in _lib._SIGNATURES, name
    assert _lib.load().hmm_abi_version() == 7


def test_the_forward_refuses_bad_arguments_without_a_gpu():
    """Every refusal below is made before the handle is read and before any HIP call: null arguments, the batch, and the HOST
    lengths (the table the kernels read lives on the device and is never read back)."""
    lib = _lib()
    call = lib.hmm_encoder_forward_text_packed
    good = np.array([1, 77, 5], dtype=np.int32)

    def refused(*args, say):
        assert call(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert b"encoder_forward_text_packed" in msg and say in msg, msg

    #       handle, ids, lengths_host, offsets_dev, batch, out, workspace, workspace_bytes, stream
    full = (ONE, FAR, good.ctypes.data, 2 * FAR, 3, 3 * FAR, 4 * FAR, 1 << 30, None)
    for missing in (0, 1, 2, 3, 5, 6):
        args = [None if i == missing else v for i, v in enumerate(full)]
        refused(*args, say=b"null argument")
    for batch in (0, -1, 65536):
        refused(ONE, FAR, good.ctypes.data, 2 * FAR, batch, 3 * FAR, 4 * FAR, 1 << 30, None, say=b"batch=")
    refused(ONE, FAR + 4, good.ctypes.data, 2 * FAR, 3, 3 * FAR, 4 * FAR, 1 << 30, None, say=b"aligned")
    refused(ONE, FAR, good.ctypes.data, 2 * FAR + 2, 3, 3 * FAR, 4 * FAR, 1 << 30, None, say=b"aligned")
    for bad in ([0, 5, 5], [5, 78, 5], [5, 5, -3], [5, 5, 2 ** 31 - 1]):
        lengths = np.array(bad, dtype=np.int32)
        refused(ONE, FAR, lengths.ctypes.data, 2 * FAR, 3, 3 * FAR, 4 * FAR, 1 << 30, None, say=b"outside 1 .. 77")
    assert lib.hmm_encoder_text_packed_workspace_bytes(None, 3, 30) == 0


def test_oracle_embeddings_do_not_depend_on_the_tokens_behind_eos():
    """The packed route leaves out the rows behind EOS.  That is sound only if they cannot change what the tower returns; here
    the fp32 oracle says so itself: every token behind EOS replaced by a random id below the EOS id (EOS stays the row's
    largest id) moves no embedding by more than the oracle moves between two runs on the same input -- which is not at all."""
    spec = ib.reduced(ib.TEXT_HUGE, 2)
    st = ib.synthetic_state(spec, seed=77, init="rich")
    g = torch.Generator().manual_seed(3)
    lengths = [1, 2, 3, 9, 33, 64, 76, 77]
    tok = torch.randint(1, 49000, (len(lengths), 77), generator=g)
    for b, n in enumerate(lengths):
        tok[b, n - 1] = EOS
        tok[b, n:] = 0
    base = ib.text_forward(tok, st, spec)
    noise = (ib.text_forward(tok, st, spec) - base).abs().max().item()
    assert noise == 0.0, f"the oracle is not deterministic run to run: {noise:.3e}"
    moved = tok.clone()
    for b, n in enumerate(lengths):
        moved[b, n:] = torch.randint(0, EOS, (77 - n,), generator=g)
    assert not torch.equal(moved, tok) and torch.equal(moved.argmax(dim=1), tok.argmax(dim=1))
    got = ib.text_forward(moved, st, spec)
    worst = (got - base).abs().max().item()
    print(f"oracle depth 2: rerun noise {noise:.3e}, tokens behind EOS replaced: max |diff| {worst:.3e}")
    assert worst <= noise
