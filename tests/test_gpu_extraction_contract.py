"""GPU: the memory contract of hmm_extract_walk and hmm_extract_carry in the guarded arena (tests/arena.py).  The gray slots, the
state, the records and the workspace are carved at exactly their sizes under the three poison patterns.  After the calls every
guard holds; the walk writes the state and records[0:count] and nothing else, the carry slot 0 and the state; records and final
state are the same bits under all three patterns (no byte the call does not own, and no uninitialised workspace byte, decides
anything); one byte short of the workspace query is refused and writes nothing; and a planted anchor_slot one past the end, or -1,
still gives the same records under every pattern, which only the clamp to [0, n_slots) can."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import arena as A

sys.path.insert(0, str(Path(__file__).resolve().parent / "golden"))
import segmentation_recipes as R  # noqa: E402

pytestmark = pytest.mark.gpu
HMM_E_WORKSPACE = -2
REC, STATE = 40, 24
SHAPES = [(48, 64), (43, 263), (7, 7)]


def _frames(h, w, n):
    """n candidates: a drifting scene with a cut, so the walk compares, accumulates and saves."""
    return np.stack([R.gray_frame(740 + (i >= n // 2), i, h, w, noise=2.0, shift=2) for i in range(n)])


def _run(pattern, h, w, planted=None, first=1, count=None):
    from hippomm_amd import _lib as L, frame_extraction as seg
    lib = L.load()
    dev = L.require_gpu()
    n = 9
    count = n - first + 1 if count is None else count
    gray = _frames(h, w, n + 1)                                   # slot 0: an anchor carried in
    times = np.arange(first, first + count, dtype=np.float64) * 1.5
    check = np.ones(count, np.int32)
    check[1] = 0                                                  # one candidate that is not due
    deny = np.zeros(count, np.int32)
    deny[2] = 1                                                   # and one whose save fails
    need = lib.hmm_extract_walk_workspace_bytes(h, w)
    ar = A.GuardedArena(A.needed_bytes([gray.nbytes, STATE, n * REC, need]), dev, A.PATTERNS[pattern])
    slots = ar.put(torch.from_numpy(gray), "gray slots")
    state = ar.carve(STATE, "state")
    records = ar.carve(n * REC, "records")
    ws = ar.carve(need, "workspace")
    start = seg._state_record(1, 0, 0.125, 0.0) if planted is None else seg._state_record(1, planted, 0.125, 0.0)
    state.copy_(torch.from_numpy(start.view(np.uint8).copy()))

    def walk(ws_bytes):
        return lib.hmm_extract_walk(ar.address(slots), n + 1, h, w, first, count, times.ctypes.data, check.ctypes.data,
                                    deny.ctypes.data, 0.3, 1.0, ar.address(state), ar.address(records) + (first - 1) * REC,
                                    ar.address(ws), ws_bytes, L.stream_ptr())

    assert walk(need - 1) == HMM_E_WORKSPACE and b"extract_walk" in lib.hmm_last_error()
    torch.cuda.synchronize()
    assert ar.is_pattern(records) and ar.is_pattern(ws) and state.cpu().numpy().tobytes() == start.tobytes()

    untouched = records.clone()
    L.check(walk(need), "hmm_extract_walk")
    torch.cuda.synchronize()
    ar.check_guards()
    assert slots.cpu().numpy().tobytes() == gray.tobytes()                       # the inputs are not written
    lo, hi = (first - 1) * REC, (first - 1 + count) * REC                        # only records[0:count] of the pointer handed in
    assert torch.equal(records[:lo], untouched[:lo]) and torch.equal(records[hi:], untouched[hi:])
    rec = records.cpu().numpy()[lo:hi].view(seg.EXTRACT_RECORD).copy()
    after_walk = state.cpu().numpy().view(seg.EXTRACT_STATE).copy()
    assert after_walk.tobytes() == seg._state_after(rec[-1]).tobytes()

    L.check(lib.hmm_extract_carry(ar.address(slots), n + 1, h, w, ar.address(state), L.stream_ptr()), "hmm_extract_carry")
    torch.cuda.synchronize()
    ar.check_guards()
    final = state.cpu().numpy().view(seg.EXTRACT_STATE).copy()
    got = slots.cpu().numpy().reshape(n + 1, h, w)
    anchor = int(after_walk["anchor_slot"][0])
    assert final["anchor_slot"][0] == 0 and final["has_anchor"][0] == 1
    for f in ("cumulative_diff", "last_save_time"):
        assert final[f].tobytes() == after_walk[f].tobytes(), f
    assert np.array_equal(got[1:], gray[1:]) and np.array_equal(got[0], gray[min(max(anchor, 0), n)])
    assert records.cpu().numpy()[lo:hi].tobytes() == rec.tobytes()              # the carry leaves the records alone
    return rec.tobytes(), final.tobytes(), rec


@pytest.mark.parametrize("shape", SHAPES)
def test_guards_hold_and_results_do_not_depend_on_the_poison(shape):
    runs = {pattern: _run(pattern, *shape) for pattern in A.PATTERNS}
    rec = runs["ones"][2]
    for pattern, run in runs.items():
        assert run[:2] == runs["ones"][:2], pattern
    assert list(rec["compared"]) == [1, 0, 1, 1, 1, 1, 1, 1, 1] and rec["saved"][2] == 0
    assert 2 <= rec["saved"].sum() < 8 and rec["anchor_slot_after"].max() > 0    # it compared, accumulated, saved and moved the anchor


def test_only_the_counted_records_are_written():
    a = _run("ones", 48, 64, first=3, count=4)
    b = _run("big", 48, 64, first=3, count=4)
    assert a[:2] == b[:2]


@pytest.mark.parametrize("planted", [10, -1])
def test_an_anchor_slot_out_of_range_is_clamped(planted):
    """n_slots is 10: slot 10 is one past the end, -1 one before the start.  A slot is 3 KiB, far inside the 64 KiB guard, so even
    an unclamped read stays in the arena; it would read poison, and the records would differ between the patterns."""
    runs = {pattern: _run(pattern, 48, 64, planted=planted) for pattern in A.PATTERNS}
    for pattern, run in runs.items():
        assert run[0] == runs["ones"][0], pattern
    clamped = _run("ones", 48, 64, planted=9 if planted == 10 else 0)
    rec, want = runs["ones"][2], clamped[2]
    for f in ("compared", "saved", "diff", "cumulative_after", "last_save_time_after"):
        assert rec[f].tobytes() == want[f].tobytes(), f
