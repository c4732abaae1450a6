"""CPU: retrieval with the reference's row and fallback rules (hmm_rank_segment_hits_filtered[_multi], EventStore.relevant_hits,
hippomm_amd.retrieval) -- everything that can be pinned without a GPU.

  * tests/relevant_hits_model.py, fed with the reference-pinned oracle's per-event hits, reproduces every case of
    tests/golden/retrieval_segments_golden.json (the unmodified reference's answers; deferred events replay the recorded entries);
  * hippomm_amd.retrieval -- feature_entries, the host merge, the callable protocol -- gives the same segments on a fake-library
    route: the two C entry points are replaced by the oracle and the model writing through the pointers they are handed, the
    store lives on the CPU, so the host layer runs as it is (argument order, packed layouts, both read-backs);
  * the new symbols are declared, exported and bound, and their argument errors name the function.
"""
import ctypes
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import relevant_hits_model as model
import retrieval_recipes as R
from oracle.vector_ops_oracle import top_k_cosine_similarity_oracle

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "retrieval_segments_golden.json").read_text())
CASES = sorted(GOLDEN["cases"])
NEW = ["hmm_rank_segment_hits_filtered", "hmm_rank_segment_hits_filtered_multi"]
HMM_E_INVALID = -1
CPU = torch.device("cpu")


def _case(case_id):
    g = GOLDEN["cases"][case_id]
    events, query, _ = R.build(g["recipe"], g["modality"])
    having = [e for e in events if g["modality"] in e.features]
    return g, events, having, query


def _fields(segment):
    return {"start_time": segment.start_time, "end_time": segment.end_time, "frames": segment.frames,
            "frame_times": segment.frame_times, "audio_data": segment.audio_data}


def test_the_golden_covers_the_cases_and_margins_the_generator_asserts():
    assert set(CASES) == {f"{m}/{name}" for m in R.MODALITIES for name in R.CASES} and GOLDEN["keep"] == 5
    for case_id in CASES:
        g = GOLDEN["cases"][case_id]
        assert g["threshold_margin"] is None or g["threshold_margin"] >= 1e-4
        assert g["min_gap_top"] is None or g["min_gap_top"] >= 1e-4
    for m in R.MODALITIES:
        assert len(GOLDEN["cases"][f"{m}/fewer_than_five"]["segments"]) < 5
        assert GOLDEN["cases"][f"{m}/deferred_parsable"]["asked"] and len(GOLDEN["cases"][f"{m}/deferred_error"]["asked"]) == 2
        assert not GOLDEN["cases"][f"{m}/not_deferred"]["asked"]


@pytest.mark.parametrize("case_id", CASES)
def test_model_on_the_oracle_hits_reproduces_the_reference(case_id):
    g, _, having, query = _case(case_id)
    per_event = [top_k_cosine_similarity_oracle(query, e.features[g["modality"]], 5) for e in having]
    answers = {pos: [(sim, fields) for sim, fields in g["deferred_entries"][e.name]]
               for pos, e in enumerate(having) if e.name in g["deferred_entries"]}
    assert model.find_segments(having, per_event, g["modality"], answers, keep=5) == g["segments"]
    # the deferred set itself: exactly the events the reference asked the LLM about, in event order
    flag = "frame_captions" if g["modality"] == "vision" else "holistic_audio_transcription"
    _, deferred = model.relevant_hits(per_event, 5, [len(model.kept_times(e, g["modality"])) for e in having],
                                      [bool(getattr(e, flag, None)) for e in having])
    assert [having[e].name for e, _, _ in deferred] == g["asked"]


# ---- the fake-library route -----------------------------------------------------------------------------------------------------
def _write(ptr, array):
    ctypes.memmove(ptr, array.ctypes.data, array.nbytes)


class _FakeLibrary:
    """hmm_cosine_topk_segmented answered by the oracle, hmm_rank_segment_hits_filtered by the model: both write through the
    pointers they receive, in the C argument order."""

    def __init__(self, matrices, query):
        self.matrices, self.query, self.calls = matrices, query, []
        self.hmm_cosine_topk_segmented_workspace_bytes = lambda n, e, k: 256

    def hmm_cosine_topk_segmented(self, store, n, dim, q, offsets, E, k, idx_out, sim_out, n_out, ws, ws_bytes, stream):
        self.calls.append("hmm_cosine_topk_segmented")
        assert E == len(self.matrices) and dim == 1024
        self.idx, self.sims = np.full((E, k), -1, np.int64), np.zeros((E, k), np.float32)
        self.counts = np.zeros(E, np.int32)
        for e, mat in enumerate(self.matrices):
            i, s = top_k_cosine_similarity_oracle(self.query, mat, k)
            self.idx[e, :len(i)], self.sims[e, :len(i)], self.counts[e] = i, s, len(i)
        _write(idx_out, self.idx), _write(sim_out, self.sims), _write(n_out, self.counts)
        return 0

    def hmm_rank_segment_hits_filtered(self, idx, sims, counts, E, k, keep, limits, defer, min_similarity, ev, row, val, n, d_ev, n_d,
                                       d_idx, d_sims, d_cnt, stream):
        self.calls.append("hmm_rank_segment_hits_filtered")
        limits = np.ctypeslib.as_array(ctypes.cast(limits, ctypes.POINTER(ctypes.c_int64)), (E,)) if limits else None
        defer = np.ctypeslib.as_array(ctypes.cast(defer, ctypes.POINTER(ctypes.c_uint8)), (E,)) if defer else None
        assert min_similarity == float(np.float32(0.4))
        out = model.rank_filtered(self.idx, self.sims, self.counts, keep, limits, defer, min_similarity)
        _write(ev, out["event"]), _write(row, out["row"]), _write(val, out["sim"]), _write(n, np.int32([out["n"]]))
        _write(d_ev, out["deferred_event"]), _write(n_d, np.int32([out["n_deferred"]]))
        if out["n_deferred"]:                                     # the compacted front only, as the kernel writes it
            _write(d_idx, np.ascontiguousarray(out["deferred_idx"])), _write(d_sims, np.ascontiguousarray(out["deferred_sim"]))
            _write(d_cnt, out["deferred_count"])
        return 0


@pytest.mark.parametrize("case_id", CASES)
def test_retrieval_functions_on_a_fake_library_reproduce_the_reference(case_id, monkeypatch):
    from hippomm_amd import _lib, retrieval
    from hippomm_amd.segmentation import SequenceSegment
    from hippomm_amd.vector_ops import EventStore
    g, events, having, query = _case(case_id)
    modality = g["modality"]
    fake = _FakeLibrary([e.features[modality] for e in having], query)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: None)
    store = EventStore([e.features[modality] for e in having], device=CPU)
    replayed = []

    def deferred(event, idx, sims):
        replayed.append(event.name)
        e = having.index(event)
        assert idx.dtype == np.int64 and sims.dtype == np.float32
        assert idx.tolist() == fake.idx[e, :fake.counts[e]].tolist() and sims.tobytes() == fake.sims[e, :fake.counts[e]].tobytes()
        return [(sim, [SequenceSegment(**fields)]) for sim, fields in g["deferred_entries"][event.name]]

    find = retrieval.find_relevant_video_segments if modality == "vision" else retrieval.find_relevant_audio_segments
    segments = find(events, torch.from_numpy(query), store=store, deferred=deferred)
    assert all(isinstance(s, SequenceSegment) for s in segments)
    assert [_fields(s) for s in segments] == g["segments"]
    assert replayed == g["asked"]
    assert fake.calls == ["hmm_cosine_topk_segmented", "hmm_rank_segment_hits_filtered"]
    if "deferred_error" in case_id:
        # the error branch is feature_entries: the recorded entries of such an event are exactly what the helper builds
        for e, event in enumerate(having):
            if event.name in g["asked"]:
                built = retrieval.feature_entries(event, fake.idx[e, :fake.counts[e]], fake.sims[e, :fake.counts[e]], modality)
                assert [[float(sim), _fields(segs[0])] for sim, segs in built] == g["deferred_entries"][event.name]
        # and it is what stands in when no callable is given
        assert [_fields(s) for s in find(events, query, store=store)] == g["segments"]


def test_a_vision_query_of_another_size_returns_nothing_and_events_without_the_modality_are_skipped(monkeypatch):
    from hippomm_amd import _lib, retrieval
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("nothing may be launched"))
    events = R.build("sizes_all_kept", "vision")[0]
    assert retrieval.find_relevant_video_segments(events, np.zeros(512, np.float32)) == []
    assert retrieval.find_relevant_audio_segments(events, np.zeros(1024, np.float32)) == []        # no event has audio features
    with pytest.raises(ValueError, match="modality"):
        retrieval.feature_entries(events[0], [0], [0.5], "text")


def test_merge_is_similarity_descending_then_event_then_in_event_order_nan_first():
    from hippomm_amd.retrieval import merge_entries
    entries = [(0.5, 2, 0, ["c"]), (0.5, 0, 1, ["b"]), (0.7, 3, 0, ["top"]), (0.5, 0, 0, ["a"]), (float("nan"), 4, 0, ["nan"]),
               (np.float32(0.5), 1, 0, ["between"]), (-0.0, 5, 0, ["z0"]), (0.0, 6, 0, ["z1"])]
    assert merge_entries(entries, 8) == ["nan", "top", "a", "b", "between", "c", "z0", "z1"]
    assert merge_entries(entries, 3) == ["nan", "top", "a"]


# ---- host-side validation of the store methods -----------------------------------------------------------------------------------
def test_store_methods_validate_before_anything_is_launched(monkeypatch):
    from hippomm_amd import _lib
    from hippomm_amd.vector_ops import EventStore
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("nothing may be launched"))
    rng = np.random.default_rng(0)
    mats = [rng.standard_normal((n, 1024)).astype(np.float32) for n in (3, 2, 4)]
    store, q = EventStore(mats, device=CPU), np.ones(1024, np.float32)
    for call, args in ((store.relevant_hits, (q,)), (store.relevant_hits_multi, (np.ones((2, 1024), np.float32),))):
        name = call.__name__
        with pytest.raises(ValueError, match=f"{name}: keep must be between 1 and 1024"):
            call(*args, keep=1025)
        with pytest.raises(ValueError, match=f"{name}: keep"):
            call(*args, keep=0)
        with pytest.raises(ValueError, match=f"{name}: row_limits has 2 entries for 3 events"):
            call(*args, row_limits=[1, 2])
        with pytest.raises(ValueError, match=f"{name}: row_limits must be >= 0"):
            call(*args, row_limits=[1, -1, 2])
        with pytest.raises(ValueError, match=f"{name}: row_limits must be integers"):
            call(*args, row_limits=[1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match=f"{name}: defer has 4 entries for 3 events"):
            call(*args, defer=[1, 0, 0, 1])
        with pytest.raises(ValueError, match=f"{name}: k must be >= 1"):
            call(*args, k=0)
    empty = EventStore([mats[0], np.zeros((0, 1024), np.float32), mats[2]], device=CPU)
    with pytest.raises(ValueError, match="relevant_hits: event 1 has no rows"):
        empty.relevant_hits(q)
    with pytest.raises(ValueError, match="relevant_hits_multi: event 1 has no rows"):
        empty.relevant_hits_multi(np.ones((2, 1024), np.float32))
    none = EventStore([], device=CPU)
    assert none.relevant_hits(q, row_limits=[], defer=[]) == ([], [])
    with pytest.raises(ValueError, match="relevant_hits: row_limits has 1 entries for 0 events"):
        none.relevant_hits(q, row_limits=[3])
    assert none.relevant_hits(q) == ([], []) and none.relevant_hits_multi(np.ones((2, 1024), np.float32)) == [([], []), ([], [])]


def test_relevant_layout_packs_hits_counts_and_the_deferred_list():
    from hippomm_amd import vector_ops as vo
    for lead, Q in (((), 1), ((3,), 3)):
        layout = vo._relevant_layout(*lead, 7, 5)
        assert layout.offsets == [0, Q * 40, Q * 80, Q * 100, Q * 104, Q * 132, Q * 136] and layout.nbytes == Q * 164
        views = layout.device_views(torch.zeros(layout.nbytes, dtype=torch.uint8))
        assert [tuple(v.shape) for v in views] == [lead + (5,)] * 3 + [lead + (1,), lead + (7,), lead + (1,), lead + (7,)]
        assert [v.dtype for v in views] == [torch.int64, torch.int64, torch.float32] + [torch.int32] * 4


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    import hippomm_amd
    from hippomm_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(build.build()))
    for name in NEW:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _lib._SIGNATURES, name
    assert len(_lib._SIGNATURES[NEW[0]][1]) == 19 and len(_lib._SIGNATURES[NEW[1]][1]) == 20
    assert _lib.load().hmm_abi_version() == 7
    assert "hmm_rank_segment_hits_filtered" in (ROOT / "hippomm_amd" / "csrc" / "hmm_api.cpp").read_text()
    for name in ("find_relevant_video_segments", "find_relevant_audio_segments", "feature_entries"):
        assert callable(getattr(hippomm_amd, name))
    assert callable(hippomm_amd.vector_ops.EventStore.relevant_hits) and callable(hippomm_amd.vector_ops.EventStore.relevant_hits_multi)


def test_argument_errors_name_the_function_without_a_gpu():
    lib = _lib()
    one = 4096                                                   # a non-null dummy: nothing is dereferenced before the checks
    outs = (one,) * 9

    def err():
        return lib.hmm_last_error()

    for name, lead in (("rank_segment_hits_filtered", ()), ("rank_segment_hits_filtered_multi", (3,))):
        call = getattr(lib, "hmm_" + name)
        tag = (name + ":").encode()
        assert call(one, one, one, *lead, 4, 5, 1025, None, None, 0.4, *outs, None) == HMM_E_INVALID
        assert tag in err() and b"keep" in err() and b"1024" in err()
        assert call(one, one, one, *lead, 4, 5, 0, None, None, 0.4, *outs, None) == HMM_E_INVALID and tag in err()
        assert call(one, one, one, *lead, 0, 5, 5, None, None, 0.4, *outs, None) == HMM_E_INVALID and tag in err()
        assert call(one, one, one, *lead, 4, 0, 5, None, None, 0.4, *outs, None) == HMM_E_INVALID and tag in err()
        assert call(one, one, one, *lead, 1 << 30, 4, 5, None, None, 0.4, *outs, None) == HMM_E_INVALID      # 2^32 slots
        assert tag in err() and b"2^32" in err()
        assert call(None, one, one, *lead, 4, 5, 5, None, None, 0.4, *outs, None) == HMM_E_INVALID
        assert tag in err() and b"null pointer" in err()
        for missing in range(9):                                  # every output is required; row_limits and defer alone may be null
            args = tuple(None if i == missing else one for i in range(9))
            assert call(one, one, one, *lead, 4, 5, 5, one, one, 0.4, *args, None) == HMM_E_INVALID, missing
            assert tag in err() and b"null pointer" in err()
    assert lib.hmm_rank_segment_hits_filtered_multi(one, one, one, 0, 4, 5, 5, None, None, 0.4, *outs, None) == HMM_E_INVALID
    assert b"rank_segment_hits_filtered_multi:" in err() and b"n_queries" in err()
