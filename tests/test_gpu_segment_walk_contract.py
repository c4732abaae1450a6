"""GPU: the memory contract of hmm_segment_walk in the guarded arena (tests/arena.py).  Scores, flags, times and the track are put at
exactly their sizes, records, state and workspace carved at exactly theirs, under the three poison patterns.  After the call every
guard holds; only records[0 .. n_segments) and the state are written (the rest of the records is still poison, the inputs are
untouched); records and state are the same bits under all three patterns (no byte the call does not own, and no workspace byte it
has not written itself, decides anything) and equal the numpy model of the walk (tests/segment_walk_model.py) field by field; one
byte short of the workspace query is refused with nothing written; and device tables that are pure poison -- times, scores and
flags that disagree with the validated host copy -- still leave every guard intact and every frame index inside the video."""
import numpy as np
import pytest
import torch

import arena as A
import segment_walk_model as model

pytestmark = pytest.mark.gpu
HMM_E_WORKSPACE = -2
REC, STATE = 40, 24
RATE = 1000


def _inputs(kind: str, dtype):
    rng = np.random.default_rng(77)
    n = 40
    times = 0.75 + np.cumsum(rng.choice([0.0, 0.5, 1.0, 1.5], size=n))            # 0.75 s before the first frame, repeated times
    scores = rng.choice([0.99, 0.97, 0.95, 0.9, np.nan], size=n - 1, p=[0.5, 0.2, 0.1, 0.1, 0.1])
    flags = np.zeros(n - 1, np.int32)
    total = float(times[-1] - times[0])
    x = (rng.choice([0.3, 0.3, 0.3, 0.004, 0.0], size=200).repeat(250) * rng.standard_normal(50_000))[:int(total * RATE) - 4_321]
    x = x.astype(dtype)                                                            # the track ends 4.3 s before the video
    if kind == "audio":
        times, scores, flags, total = times[:0], scores[:0], flags[:0], len(x) / RATE
    if kind == "video":
        x = None
    return times, scores, flags, x, total


def _run(pattern, kind, dtype, poisoned_tables=False, flag_pair=None):
    from hippomm_amd import _lib as L, segmentation as seg
    lib = L.load()
    dev = L.require_gpu()
    times, scores, flags, x, total = _inputs(kind, dtype)
    if flag_pair is not None:
        flags[flag_pair] = 1
    max_dur, min_dur, thr = 10.0, 3.0, 0.95
    max_steps = int(np.ceil(total / min_dur)) + 2
    max_windows = 0 if x is None else int((max_dur * RATE + 2) // (RATE // 2)) + 1
    cut, without = seg.silence_cut(dtype, -40) if x is not None else (0.0, False)
    need = lib.hmm_segment_walk_workspace_bytes(max_windows, max_steps)
    sizes = [scores.nbytes, flags.nbytes, times.nbytes, 0 if x is None else x.nbytes, max_steps * REC, STATE, need]
    ar = A.GuardedArena(A.needed_bytes(sizes), dev, A.PATTERNS[pattern])
    if poisoned_tables:                                                            # what the kernels read is the pattern itself
        d_scores, d_flags, d_times = (ar.carve(a.nbytes, name) for a, name in ((scores, "scores"), (flags, "flags"), (times, "times")))
    else:
        d_scores, d_flags, d_times = (ar.put(torch.from_numpy(a), name) for a, name in ((scores, "scores"), (flags, "flags"),
                                                                                         (times, "times")))
    track = None if x is None else ar.put(torch.from_numpy(x), "track")
    records = ar.carve(max_steps * REC, "records")
    state = ar.carve(STATE, "state")
    ws = ar.carve(need, "workspace")
    addr = lambda v: ar.address(v) if v is not None and v.numel() else None       # noqa: E731

    def walk(ws_bytes):
        return lib.hmm_segment_walk(addr(d_scores), addr(d_flags), addr(d_times), times.ctypes.data if len(times) else None, len(times),
                                    addr(track), 1 if dtype is np.float64 else 0, 0 if x is None else len(x), RATE, total, max_dur, min_dur,
                                    thr, cut, int(without), max_windows, max_steps, ar.address(records), ar.address(state), addr(ws),
                                    ws_bytes, L.stream_ptr())

    if need:
        assert walk(need - 1) == HMM_E_WORKSPACE and b"segment_walk" in lib.hmm_last_error()
        torch.cuda.synchronize()
        assert ar.is_pattern(records) and ar.is_pattern(state) and ar.is_pattern(ws)
    L.check(walk(need), "hmm_segment_walk")
    torch.cuda.synchronize()
    ar.check_guards()
    st = state.cpu().numpy().view(seg.SEGMENT_STATE)[0]
    n_seg = int(st["n_segments"])
    assert 0 <= n_seg <= max_steps and ar.high_water(records) < n_seg * REC        # nothing past the counted records
    rec = records.cpu().numpy()[:n_seg * REC].view(seg.SEGMENT_RECORD).copy()
    if not poisoned_tables:
        for view, a in ((d_scores, scores), (d_flags, flags), (d_times, times)):
            assert view.cpu().numpy().tobytes() == a.tobytes()                     # the inputs are not written
    if track is not None:
        assert track.cpu().numpy().tobytes() == x.tobytes()
    return rec, st, (times, scores, flags, x, total, max_dur, min_dur, thr, cut, without, max_steps)


def _model(inputs):
    times, scores, flags, x, total, max_dur, min_dur, thr, cut, without, max_steps = inputs
    p = model.Params(total=total, max_dur=max_dur, min_dur=min_dur, sim_threshold=thr)
    if x is not None:
        p.rate, p.track_len, p.dtype, p.rms_cut, p.silent_without_rms = RATE, len(x), x.dtype.type, cut, without
    window_sum = None if x is None else (lambda lo, count: np.sum(np.square(x[lo:lo + count])))
    return model.walk(p, scores, flags, times, window_sum, max_steps)


CASES = [("both", np.float64), ("both", np.float32), ("video", np.float64), ("audio", np.float64), ("audio", np.float32)]


@pytest.mark.parametrize("kind,dtype", CASES, ids=[f"{k}-{np.dtype(d).name}" for k, d in CASES])
def test_guards_hold_and_records_are_the_models_under_every_poison(kind, dtype):
    runs = {pattern: _run(pattern, kind, dtype) for pattern in A.PATTERNS}
    rec, st, inputs = runs["ones"]
    for pattern, (r, s, _) in runs.items():
        assert r.tobytes() == rec.tobytes() and s.tobytes() == st.tobytes(), pattern
    want, status, flagged = _model(inputs)
    assert (int(st["status"]), int(st["flagged_pair"]), int(st["steps"])) == (status, flagged, len(want)) and status == model.DONE
    assert [tuple(r) for r in rec.tolist()] == want
    assert len(want) >= 4 and (kind == "audio" or any(r[4] >= 0 for r in want)) and (kind == "video" or any(r[5] >= 0 for r in want))
    assert st["current_start"] == want[-1][1]


def test_a_flagged_pair_stops_the_walk_where_the_model_stops():
    rec0, _, inputs = _run("ones", "video", np.float64)
    consulted = int(next(r["cut_pair"] for r in rec0[1:] if r["cut_pair"] >= 0))   # a pair a later step reads for certain: it cut there
    runs = {pattern: _run(pattern, "video", np.float64, flag_pair=consulted) for pattern in A.PATTERNS}
    rec, st, inputs = runs["ones"]
    want, status, flagged = _model(inputs)
    assert status == model.FLAGGED and (int(st["status"]), int(st["flagged_pair"])) == (status, flagged)
    assert [tuple(r) for r in rec.tolist()] == want and int(st["steps"]) == len(want) + 1
    for pattern, (r, s, _) in runs.items():
        assert r.tobytes() == rec.tobytes() and s.tobytes() == st.tobytes(), pattern


@pytest.mark.parametrize("pattern", list(A.PATTERNS))
def test_poisoned_device_tables_read_less_never_elsewhere(pattern):
    """The host copy of the times is valid, the device copies of times, scores and flags are the poison: NaN, zero or huge.  The
    walk then decides nonsense, but inside its buffers: guards intact (checked in _run), frame indices inside the video."""
    rec, st, inputs = _run(pattern, "both", np.float64, poisoned_tables=True)
    n = len(inputs[0])
    assert int(st["status"]) in (model.DONE, model.FLAGGED, model.BOUND)
    for r in rec:
        assert 0 <= r["first_frame"] <= n and -1 <= r["last_frame"] < n and -1 <= r["cut_pair"] < n - 1
        assert 0 <= r["pairs_consulted"] < n and 0 <= r["windows_consulted"] <= 21
