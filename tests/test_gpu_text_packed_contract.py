"""GPU: the memory contract of hmm_encoder_forward_text_packed in the guarded arena (tests/arena.py).  The ids, the offsets table,
the output and the workspace are carved at exactly their size -- the workspace at exactly hmm_encoder_text_packed_workspace_bytes --
and after the call every guard still holds its pattern, the ids and the table keep their bytes, and the embeddings are the same
bits under all three patterns: a byte read outside what the call owns, or a workspace byte read before it is written, would
differ between two of them.  With one byte fewer the call is refused before anything is written."""
import functools

import numpy as np
import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu

HMM_OK, HMM_E_WORKSPACE = 0, -2
EOS = 49407
# few-row regime (<= 700 rows: split-K slabs in the workspace), one question, the large regime, and lengths at both ends
CASES = {"few": (1, 77, 2, 9, 33), "one": (7,), "large": (77,) * 9 + (1, 12, 64)}


@functools.lru_cache(maxsize=None)
def _tower():
    from hippomm_amd.encoder import HipTower
    from oracle import imagebind_oracle as ib
    spec = ib.reduced(ib.TEXT_HUGE, 2)
    return HipTower("text", ib.synthetic_state(spec, seed=1234, init="rich"), depth=2)


def _ids(lengths):
    tok = torch.randint(1, 49000, (len(lengths), 77), generator=torch.Generator().manual_seed(len(lengths)))
    for b, n in enumerate(lengths):
        tok[b, n - 1] = EOS                                      # the tokens behind EOS stay random: they must not be read
    return tok


def _run(pattern, lengths, short=0):
    from hippomm_amd import _lib
    from hippomm_amd.encoder import text_offsets
    t = _tower()
    lib, dev = t._lib, _lib.require_gpu()
    batch = len(lengths)
    host_lengths = np.array(lengths, dtype=np.int32)
    off = text_offsets(host_lengths)
    rows = int(off[-1])
    need = lib.hmm_encoder_text_packed_workspace_bytes(t._h, batch, rows)
    assert need > 0
    tok = _ids(lengths)
    ar = A.GuardedArena(A.needed_bytes([tok.numel() * 8, off.nbytes, batch * 4096, need]), dev, A.PATTERNS[pattern])
    ids = ar.put(tok, "ids")
    table = ar.put(torch.from_numpy(off), "offsets table", align=16)
    out = ar.carve(batch * 4096, "embeddings")
    ws = ar.carve(need, "workspace")
    rc = lib.hmm_encoder_forward_text_packed(t._h, ar.address(ids), host_lengths.ctypes.data, ar.address(table), batch,
                                             ar.address(out), ar.address(ws), need - short, _lib.stream_ptr())
    torch.cuda.synchronize()
    ar.check_guards()
    assert torch.equal(ids.cpu(), tok.reshape(-1).view(torch.uint8)), "the ids were written"
    assert torch.equal(table.cpu(), torch.from_numpy(off).view(torch.uint8)), "the offsets table was written"
    if short:
        assert rc == HMM_E_WORKSPACE, f"workspace_bytes = need - {short} = {need - short} gave status {rc}"
        assert b"workspace" in lib.hmm_last_error()
        assert ar.is_pattern(ws) and ar.is_pattern(out), "a refused call wrote to its workspace or its output"
        return None
    _lib.check(rc, "hmm_encoder_forward_text_packed")
    return out.clone().view(torch.int32).cpu(), tok


@pytest.mark.parametrize("case", list(CASES))
def test_guards_hold_and_embeddings_do_not_depend_on_the_poison(case):
    lengths = CASES[case]
    runs = {pattern: _run(pattern, lengths) for pattern in A.PATTERNS}
    first, tok = runs["ones"]
    for pattern, (bits, _) in runs.items():
        assert torch.equal(bits, first), pattern
    want = _tower()(tok, pack=True)                              # and they are the Python route's bits
    assert torch.equal(first.view(torch.float32).reshape(len(lengths), 1024), want.cpu())


@pytest.mark.parametrize("case", list(CASES))
def test_one_byte_fewer_is_refused_before_anything_is_written(case):
    _run("ones", CASES[case], short=1)
    _run("big", CASES[case], short=1)


def test_workspace_size_is_a_function_of_batch_and_rows_and_zero_outside_them():
    t = _tower()
    size = t._lib.hmm_encoder_text_packed_workspace_bytes
    assert size(t._h, 3, 30) > 0 and size(t._h, 3, 30) == size(t._h, 3, 30)
    assert size(t._h, 0, 0) == 0 and size(t._h, 3, 2) == 0 and size(t._h, 3, 3 * 77 + 1) == 0
    assert size(t._h, 3, 3 * 77) > size(t._h, 3, 3)
