"""CPU: the plan and decide steps of hmm_segment_walk, stated as a numpy model (tests/segment_walk_model.py), give the segments of
segmentation.walk_segments -- fed with a table-backed score_window and the host's audio levels -- on a few hundred seeded cases:
video only, audio only and both, float32 and float64 tracks, frame_times[0] != 0, repeated times, a track shorter than the video,
NaN scores, int and float silence thresholds.  The silence rule the device uses instead of a log10 (segmentation.silence_cut:
rms < rms_cut) is checked against the host's scalar expression on the 200 000 floats either side of the cut and on 200 000 random
ones, so a libm whose log10 is not monotonic there shows up here.  Five planted mistakes of the model each change a planted
case, so the comparison can see what it is there to pin."""
import struct

import numpy as np
import pytest

import segment_walk_model as model

N_RANDOM = 360


def _bits(x) -> bytes:
    return struct.pack("<d", float(x))


def _track(rng, n, dtype):
    """Quarter-second blocks (at 100 Hz) that are loud, faint (below -40 dB) or exactly silent, so that levels fall on both sides."""
    amp = rng.choice([0.3, 0.3, 0.3, 0.004, 0.0], size=n // 25 + 1).repeat(25)[:n]
    return (amp * rng.standard_normal(n)).astype(dtype)


def random_case(seed: int) -> dict:
    rng = np.random.default_rng(1000 + seed)
    kind = ("video", "audio", "both")[seed % 3]
    c = dict(kind=kind, times=[], scores=[], audio=None, rate=0, flags=[],
             max_dur=float(rng.choice([3.0, 5.5, 10.0])), min_dur=float(rng.choice([0.5, 1.0, 2.5, 5.0])), sim_threshold=0.95,
             silence=[-40, -35.5, -40.0][seed % 3 if seed % 5 else 1])
    duration = float(rng.uniform(4.0, 40.0))
    if kind != "audio":
        n = int(rng.integers(1, 32))
        steps = rng.choice([0.0, 0.4, 0.7, 1.0, 1.0, 2.3], size=n - 1) * duration / max(n, 1) * 1.2
        t0 = float(rng.choice([0.0, 0.0, 0.3, 1.5]))
        c["times"] = [float(t) for t in t0 + np.concatenate([[0.0], np.cumsum(steps)])]
        c["scores"] = [float(s) for s in rng.choice([0.99, 0.97, 0.95, 0.9, 0.5, np.nan], size=n - 1)]
        c["flags"] = [0] * (n - 1)
        duration = c["times"][-1] - c["times"][0]
    if kind != "video":
        c["rate"] = int(rng.choice([100, 100, 1000, 37]))
        shorter = kind == "both" and seed % 4 == 0
        n_samples = int((duration * (0.6 if shorter else 1.0) + float(rng.uniform(0, 1))) * c["rate"])
        c["audio"] = _track(rng, max(n_samples, 1), np.float32 if seed % 2 else np.float64)
    return c


def params_of(c: dict) -> model.Params:
    from hippomm_amd.segmentation import silence_cut
    has_video = bool(c["times"])
    total = c["times"][-1] - c["times"][0] if has_video else len(c["audio"]) / c["rate"]
    p = model.Params(total=total, max_dur=c["max_dur"], min_dur=c["min_dur"], sim_threshold=c["sim_threshold"])
    if c["audio"] is not None:
        p.rate, p.track_len, p.dtype = c["rate"], len(c["audio"]), c["audio"].dtype.type
        p.rms_cut, p.silent_without_rms = silence_cut(c["audio"].dtype, c["silence"])
    return p


def run_model(c: dict, mutant=None):
    p = params_of(c)
    x = c["audio"]
    window_sum = None if x is None else (lambda lo, count: np.sum(np.square(x[lo:lo + count])))
    max_steps = int(np.ceil(max(p.total, 0.0) / p.min_dur)) + 2
    return model.walk(p, c["scores"], c["flags"], c["times"], window_sum, max_steps, mutant)


def run_host(c: dict):
    """walk_segments on the same case: scores from the table, levels by the reference's numpy expression on host slices."""
    from hippomm_amd.segmentation import walk_segments
    frames = [f"frame_{i}" for i in range(len(c["times"]))] or None
    table = c["scores"]
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                        # numpy's "Mean of empty slice" past a short track's end
            return walk_segments(frames, c["times"] or None, c["audio"], c["rate"] or None,
                                 lambda pairs: (np.float64(table[later - 1]) for later, earlier in pairs),
                                 c["max_dur"], c["min_dur"], c["sim_threshold"], c["silence"])


def assert_same(c: dict, records, segments):
    assert len(records) == len(segments), (len(records), len(segments))
    frames = [f"frame_{i}" for i in range(len(c["times"]))]
    for rec, seg in zip(records, segments):
        start, end, first, last = rec[:4]
        assert _bits(start) == _bits(seg.start_time) and _bits(end) == _bits(seg.end_time), (rec, seg.start_time, seg.end_time)
        if c["times"]:
            assert frames[first:last + 1] == seg.frames and c["times"][first:last + 1] == seg.frame_times, rec
        if c["audio"] is not None:
            lo, hi = int(start * c["rate"]), int(end * c["rate"])
            assert seg.audio_data.shape == c["audio"][lo:hi].shape
            assert seg.audio_data.size == 0 or np.shares_memory(seg.audio_data, c["audio"][lo:hi])


@pytest.mark.parametrize("block", range(6))
def test_model_gives_the_segments_of_walk_segments_on_seeded_cases(block):
    seen = {"cut_pair": 0, "cut_window": 0, "clamped": 0, "empty_window": 0}
    for seed in range(block * N_RANDOM // 6, (block + 1) * N_RANDOM // 6):
        c = random_case(seed)
        records, status, _ = run_model(c)
        assert status == model.DONE, seed
        try:
            assert_same(c, records, run_host(c))
        except AssertionError as exc:
            raise AssertionError(f"seed {seed} ({c['kind']}): {exc}") from exc
        seen["cut_pair"] += sum(r[4] >= 0 for r in records)
        seen["cut_window"] += sum(r[5] >= 0 for r in records)
        seen["clamped"] += sum(r[1] - r[0] == c["min_dur"] for r in records)
        seen["empty_window"] += c["audio"] is not None and bool(records) and len(c["audio"]) / c["rate"] < records[-1][1] - 1
    print(seen)
    assert all(seen.values()), seen                                # every branch of the walk was taken in this block


# ---- planted cases: 21 frames at 1 fps, max 10 s, min 2 s, a loud 100 Hz float64 track with one planted stretch ------------------
def planted(name: str) -> dict:
    c = dict(kind="both", times=[float(i) for i in range(21)], scores=[0.99] * 20, flags=[0] * 20, rate=100,
             audio=np.full(2000, 0.5), max_dur=10.0, min_dur=2.0, sim_threshold=0.95, silence=-40)
    if name == "audio_does_not_override":                          # the video cuts at 8.0, a silent window at 3.0 overrides it
        c["scores"][7] = 0.5
        c["audio"][300:350] = 0.0
    elif name == "le_for_lt":                                      # a score that equals the threshold does not cut
        c["scores"][6] = 0.95
    elif name == "offset_zero_included":                           # silence at offset 0 of the step is never looked at
        c["audio"][0:50] = 0.0
    elif name == "clamp_before_audio":                             # silence at 0.5 s: the clamp to 2.0 comes after it
        c["audio"][50:100] = 0.0
    elif name == "unclipped_length_in_mean":                       # the track ends inside the window at 9.5 s: 25 samples of 0.012
        c["audio"] = np.full(975, 0.012)                           # (-38.4 dB) are loud; spread over 50 they would be -41.4 dB
    else:
        raise KeyError(name)
    return c


@pytest.mark.parametrize("name", model.MUTANTS)
def test_planted_cases_equal_the_host_and_notice_each_mutant(name):
    c = planted(name)
    records, status, _ = run_model(c)
    assert status == model.DONE
    assert_same(c, records, run_host(c))
    changed = [other for other in model.MUTANTS if run_model(planted(other), mutant=name)[0] != run_model(planted(other))[0]]
    print(f"{name}: changes {changed}")
    assert name in changed, changed


def test_a_flagged_pair_stops_the_walk_only_when_consulted():
    c = planted("le_for_lt")
    c["scores"][15] = 0.5                                          # step 2 (10 .. 20) cuts at pair 15 before it reaches pair 12
    c["flags"][12] = 1
    records, status, _ = run_model(c)
    assert status == model.DONE and all(r[4] != 12 for r in records)
    c["scores"][15] = 0.99
    records, status, pair = run_model(c)
    assert (status, pair) == (model.FLAGGED, 12) and len(records) == 1


def test_window_rows_are_numpy_slices():
    c = planted("unclipped_length_in_mean")
    p = params_of(c)
    rows = model.window_rows(p, 0.0)
    assert rows[0] == (950, 25) and rows[1] == (900, 50) and rows[-1] == (50, 50) and len(rows) == 19
    assert all(n == 0 and lo == 975 for lo, n in model.window_rows(p, 10.0))
    for lo, n in rows:
        assert n == len(c["audio"][lo:lo + p.window])


# ---- the silence rule without a log10 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_rms_cut_reproduces_the_host_decision(dtype):
    from hippomm_amd.segmentation import silence_cut
    threshold = -40
    cut, without = silence_cut(dtype, threshold)
    assert without is True and abs(cut - 0.01) < 1e-8
    U = np.uint32 if dtype is np.float32 else np.uint64
    at = int(dtype(cut).view(U))
    near = np.arange(at - 200_000, at + 200_000, dtype=np.int64).astype(U).view(dtype)
    rng = np.random.default_rng(7)
    spread = np.exp(rng.uniform(np.log(1e-30), np.log(1e3), 200_000)).astype(dtype)
    wrong = 0
    for values in (near, spread):
        for rms in values:                                         # numpy scalars, through the host's own scalar expression
            wrong += bool(20 * np.log10(rms) < threshold) != bool(rms < cut)
    assert wrong == 0
    for rms in (dtype(0), dtype(np.nan), dtype(-1)):               # no rms > 0: the int -100, as the host has it
        assert bool((20 * np.log10(rms) if rms > 0 else -100) < threshold) is without
    assert silence_cut(dtype, -120.5)[1] is False and silence_cut(dtype, np.inf)[0] == np.inf
