"""GPU: the memory contract of hmm_keyframe_extend in the guarded arena (tests/arena.py).  The new rows, kept_rows, kept_idx, n_kept
and the workspace are carved at exactly their documented sizes (capacity = kept_bound + m, the least the call accepts).  After the
call every guard holds its pattern; the count, the kept indices and the appended rows are the same bits under all three patterns
and after another m has used the workspace (no uninitialised workspace or state byte decides anything); slots of kept_rows /
kept_idx outside [old n_kept, new n_kept) hold what they held; one byte short of the workspace query is refused and writes nothing."""
import numpy as np
import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu
HMM_E_WORKSPACE = -2
OTHER_M = {1: 1, 64: 33, 65: 64}                              # what dirties the workspace first: same and different layouts


def _rows(m, k):
    """k unrelated rows (all kept) and m new rows: a third unrelated, a third scaled copies of state rows (of earlier new rows
    when the state is empty), a third scaled copies of the new row two places earlier."""
    rng = np.random.default_rng(100 * m + k)
    base = rng.standard_normal((k, 1024)).astype(np.float32)
    new = rng.standard_normal((m, 1024)).astype(np.float32)
    for i in range(m):
        if i % 3 == 1 and k:
            new[i] = base[(5 * i) % k] * np.float32(1.5)
        elif i % 3 == 2:
            new[i] = new[i - 2] * np.float32(0.5)
    return base, new


def _extend(lib, L, ar, rows, m, state, n_seen, bound, ws, ws_bytes=None):
    kept_rows, kept_idx, n_kept, capacity = state
    return lib.hmm_keyframe_extend(ar.address(rows), m, 1024, float(np.float32(0.9)), ar.address(kept_rows), ar.address(kept_idx),
                                   capacity, ar.address(n_kept), n_seen, bound, ar.address(ws),
                                   ws.numel() if ws_bytes is None else ws_bytes, L.stream_ptr())


def _run(pattern, m, k, dirty=False, poison_count=None):
    from hippomm_amd import _lib as L
    lib = L.load()
    dev = L.require_gpu()
    base, new = _rows(m, k)
    other = np.random.default_rng(9).standard_normal((OTHER_M[m], 1024)).astype(np.float32)
    capacity = k + m
    need, need_k, need_o = (lib.hmm_keyframe_extend_workspace_bytes(x) for x in (m, max(k, 1), OTHER_M[m]))
    assert need_o <= need
    sizes = [new.nbytes, base.nbytes, other.nbytes, capacity * 4096, capacity * 8, 8, need, need_k,
             OTHER_M[m] * 4096, OTHER_M[m] * 8, 8]
    ar = A.GuardedArena(A.needed_bytes(sizes), dev, A.PATTERNS[pattern])
    new_dev = ar.put(torch.from_numpy(new), "new rows")
    state = (ar.carve(capacity * 4096, "kept_rows"), ar.carve(capacity * 8, "kept_idx"), ar.carve(8, "n_kept"), capacity)
    ws = ar.carve(need, "workspace")

    # one byte short: refused, nothing written
    assert _extend(lib, L, ar, new_dev, m, state, 0, 0, ws, need - 1) == HMM_E_WORKSPACE
    assert b"keyframe_extend" in lib.hmm_last_error()
    torch.cuda.synchronize()
    assert all(ar.is_pattern(v) for v in (*state[:3], ws))

    if dirty:                                                # another m through the same workspace, into a state of its own
        other_dev = ar.put(torch.from_numpy(other), "other rows")
        scratch = (ar.carve(OTHER_M[m] * 4096, "other kept_rows"), ar.carve(OTHER_M[m] * 8, "other kept_idx"),
                   ar.carve(8, "other n_kept"), OTHER_M[m])
        L.check(_extend(lib, L, ar, other_dev, OTHER_M[m], scratch, 0, 0, ws), "hmm_keyframe_extend")
    if k:                                                    # the state: k rows, all kept
        base_dev = ar.put(torch.from_numpy(base), "state rows")
        ws_k = ar.carve(need_k, "workspace of the state's call")
        L.check(_extend(lib, L, ar, base_dev, k, state, 0, 0, ws_k), "hmm_keyframe_extend")
        torch.cuda.synchronize()
        assert int(state[2].view(torch.int64).item()) == k
    if poison_count is not None:
        state[2].view(torch.int64).fill_(poison_count)
    before_rows, before_idx = state[0].clone(), state[1].clone()

    L.check(_extend(lib, L, ar, new_dev, m, state, k, k, ws), "hmm_keyframe_extend")
    torch.cuda.synchronize()
    ar.check_guards()
    assert torch.equal(new_dev.cpu(), torch.from_numpy(new).view(-1).view(torch.uint8))          # inputs are not written
    count = int(state[2].view(torch.int64).item())
    assert k <= count <= capacity
    rows, idx = state[0].view(-1, 4096), state[1].view(-1, 8)
    for lo, hi in ((0, k), (count, capacity)):               # outside [old n_kept, new n_kept): what they held
        assert torch.equal(rows[lo:hi], before_rows.view(-1, 4096)[lo:hi]), (lo, hi)
        assert torch.equal(idx[lo:hi], before_idx.view(-1, 8)[lo:hi]), (lo, hi)
    return count, idx[:count].clone().view(torch.int64).flatten().cpu(), rows[:count].clone().cpu()


@pytest.mark.parametrize("k", [0, 63, 64, 65])
@pytest.mark.parametrize("m", [1, 64, 65])
def test_guards_hold_and_results_do_not_depend_on_the_poison(m, k):
    from hippomm_amd.consolidation import select_key_frames_device
    runs = {pattern: _run(pattern, m, k) for pattern in A.PATTERNS}
    runs["dirty workspace"] = _run("ones", m, k, dirty=True)
    count, idx, rows = runs["ones"]
    for label, (c, i, r) in runs.items():
        assert c == count and torch.equal(i, idx) and torch.equal(r, rows), label
    base, new = _rows(m, k)
    want = select_key_frames_device(torch.from_numpy(np.concatenate([base, new])).cuda()).cpu()
    assert torch.equal(idx, want)
    if m > 2:
        assert k < count < k + m                             # rows were kept and rows were dropped


def test_a_device_count_above_the_bound_is_contained():
    """*n_kept poisoned far above kept_bound: the kernels work with min(count, bound, capacity).  Containment only: _run checks
    the guards and that no slot below the old count or past the new one changed."""
    for pattern in A.PATTERNS:
        count, idx, rows = _run(pattern, 65, 65, poison_count=1 << 40)
        assert 65 <= count <= 130 and idx.numel() == count
