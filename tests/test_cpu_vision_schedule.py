"""CPU: the integer decisions of preprocess.vision_pipeline -- which range the consumer gets next (_next_range), where an upload
run ends (_run_end) -- and the pinned staging type every upload path shares (_pinned.PinnedStage / stage)."""
import itertools
import random

import pytest
import torch

from hippomm_amd import _pinned
from hippomm_amd import preprocess as pp


def _clamped(n, workers, first_chunk, upload_min, max_chunk):
    """vision_pipeline's own clamping of its arguments."""
    workers = min(workers, n)
    first_chunk = max(2, min(first_chunk if first_chunk > 0 else min(workers, 8), n)) if n > 1 else 1
    return first_chunk, max(1, upload_min), max(max_chunk, 3)


def _simulate(n, first_chunk, upload_min, depth, max_chunk, tail_wait, seed):
    """The main loop of vision_pipeline with seeded decoders and a seeded GPU -> the ranges handed to the consumer."""
    rng = random.Random(seed)
    prefix = uploaded = issued = ready = 0
    running, ranges, after_all_decoded = [], [], 0                  # running: iterations each range still takes, oldest first
    while issued < n:
        if prefix == n:
            after_all_decoded += 1
            assert after_all_decoded <= 4 * n + 8, "the loop does not end"          # a hang guard, not a measurement
        prefix = min(n, prefix + rng.randint(0, 3))
        if prefix > uploaded and (prefix - uploaded >= upload_min or prefix == n or uploaded < first_chunk <= prefix):
            uploaded = prefix
        running = [left - 1 for left in running]
        if uploaded > issued:
            while running and running[0] <= 0:
                running.pop(0)

            def ready_upto():
                nonlocal ready
                ready = rng.randint(max(ready, issued), uploaded)    # in [issued, uploaded], never back
                return ready

            hi = pp._next_range(n, issued, uploaded, len(running), ready_upto, first_chunk, depth, max_chunk, tail_wait)
            if hi:
                ranges.append((issued, hi))
                running.append(rng.randint(1, 4))
                issued = hi
    return ranges


@pytest.mark.parametrize("n", range(1, 13))
def test_next_range_covers_the_call_in_order_and_never_cuts_a_single_frame(n):
    for first_chunk0, upload_min0, depth, max_chunk0, tail_wait, seed in itertools.product(
            (0, 2, 5), (1, 3, 8), (1, 3), (3, 4, 256), (0, 2), (1, 2, 3)):
        first_chunk, upload_min, max_chunk = _clamped(n, 4, first_chunk0, upload_min0, max_chunk0)
        ranges = _simulate(n, first_chunk, upload_min, depth, max_chunk, tail_wait, seed)
        case = (n, first_chunk0, upload_min0, depth, max_chunk0, tail_wait, seed, ranges)
        assert [lo for lo, _ in ranges] == [0] + [hi for _, hi in ranges[:-1]] and ranges[-1][1] == n, case
        assert all(hi - lo >= 2 for lo, hi in ranges) or n == 1, case
        assert all(hi - lo <= max_chunk for lo, hi in ranges), case


def test_next_range_asks_for_finished_uploads_only_where_it_needs_them():
    def never():
        raise AssertionError("queried")
    assert pp._next_range(8, 2, 8, 1, never, 2, 1, 256, 0) == 8           # everything uploaded: the rest at once
    assert pp._next_range(8, 2, 6, 0, never, 2, 1, 256, 2) == 0           # the tail is about to arrive
    assert pp._next_range(8, 2, 5, 1, never, 2, 1, 256, 0) == 0           # the GPU has no room
    assert pp._next_range(8, 0, 3, 0, never, 4, 1, 256, 0) == 0           # fewer than the first range needs
    assert pp._next_range(8, 2, 7, 0, lambda: 7, 2, 1, 256, 0) == 6       # would leave one frame: one less
    assert pp._next_range(8, 5, 7, 0, lambda: 7, 2, 1, 256, 0) == 0       # ... and not by cutting a single frame


@pytest.mark.parametrize("cap", range(1, 6))
def test_run_end_cuts_a_prefix_into_runs_of_one_kind_that_do_not_wrap(cap):
    kinds = (pp._RGB, pp._COEF, pp._BITS, pp._OWN)
    for length in range(1, 7):
        for kind in itertools.product(kinds, repeat=length):
            a, runs = 0, []
            while a < length:
                b = pp._run_end(a, length, cap, kind)
                assert a < b <= length, (kind, a, b)
                runs.append((a, b))
                a = b
            assert [lo for lo, _ in runs] == [0] + [hi for _, hi in runs[:-1]] and runs[-1][1] == length, (kind, runs)
            for lo, hi in runs:
                assert len(set(kind[lo:hi])) == 1, (kind, runs)
                assert kind[lo] != pp._OWN or hi - lo == 1, (kind, runs)
                assert all(b % cap != 0 for b in range(lo + 1, hi)), (kind, runs)


class _Event:
    """Stands in for torch.cuda.Event: notes what was waited on, and in which order."""
    log = []

    def __init__(self, name=None):
        self.name, self.stream = name, "unrecorded"

    def record(self, stream=None):
        self.stream = stream

    def synchronize(self):
        _Event.log.append(self.name)


@pytest.fixture
def unpinned(monkeypatch):
    """pin_memory needs a GPU; the bookkeeping under test does not."""
    real = torch.empty
    monkeypatch.setattr(_pinned.torch, "empty", lambda *a, pin_memory=False, **k: real(*a, **k))
    monkeypatch.setattr(_pinned.torch.cuda, "Event", _Event)
    _Event.log = []


def test_pinned_stage_waits_for_its_last_upload_and_marks_a_fresh_event(unpinned):
    st = _pinned.PinnedStage((4, 3, 2), torch.int32)
    assert st.capacity == 4 and st.host.shape == (4, 3, 2) and st.pinned.dtype == torch.int32 and st.last_upload is None
    st.host[1, 2, 1] = 7
    assert int(st.pinned[1, 2, 1]) == 7                                  # one memory
    st.wait()                                                            # nothing uploaded yet: nothing to wait for
    assert _Event.log == []
    ev = st.mark("side")
    assert ev is st.last_upload and ev.stream == "side"
    assert st.mark() is not ev and st.last_upload.stream is None         # the current stream
    st.last_upload.name = "second"
    st.wait()
    assert _Event.log == ["second"]


def test_stage_reuses_what_fits_and_replaces_what_is_too_small_in_any_dimension(unpinned):
    table = {}
    st = _pinned.stage(table, "k", (4, 8))
    assert st.pinned.shape == (4, 8) and st.pinned.dtype == torch.uint8 and table == {"k": st}
    assert _pinned.stage(table, "k", (4, 8)) is st and _pinned.stage(table, "k", (2, 5)) is st
    for shape in ((5, 8), (4, 9), (1, 16)):
        old = table["k"]
        old.last_upload = _Event(shape)
        _Event.log = []
        new = _pinned.stage(table, "k", shape)
        assert new is not old and new.pinned.shape == shape and table == {"k": new}
        assert _Event.log == [shape]                                     # the replaced buffer's upload was waited for


@pytest.mark.parametrize("keep,left", [(1, ["e"]), (3, ["c", "d", "e"]), (None, ["a", "b", "c", "d", "e"])])
def test_stage_keeps_the_newest_entries_and_waits_on_those_it_drops(unpinned, keep, left):
    table = {}
    for key in "abcd":
        _pinned.stage(table, key, (2,), keep=None).last_upload = _Event(key)
    _Event.log = []
    _pinned.stage(table, "e", (2,), keep=keep)
    assert list(table) == left
    assert _Event.log == [k for k in "abcd" if k not in left]            # oldest first, each waited on before it goes
    _Event.log = []
    assert _pinned.stage(table, left[0], (2,), keep=keep) is table[left[0]] and list(table) == left and _Event.log == []
