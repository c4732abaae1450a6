"""CPU: the block algorithm of the device span finder (csrc/event_json_find_core.h), run on the host through
hmm_json_find_matrices_blocks -- the same per-byte rules, summaries and compositions the gfx950 kernels call, the same group size
and decline rules -- against the host finder hmm_json_find_matrices on every corpus of event_json_find_cases and on seeded random
texts; when it may decline; the ABI and the argument checks of hmm_json_find_matrices_device, which need no GPU; and the Python
entry points' defaults."""
import ctypes as C
import inspect
import re

import pytest

import event_json_find_cases as fc


def _agree(raw, min_values, what, may_decline=False):
    want, n = fc.host_find(raw, min_values)
    got, rep = fc.blocks_find(raw, min_values)
    if may_decline:
        assert rep["status"] == fc.FIND_DECLINED and rep["n_found"] == 0 and got == [], (what, rep)
        assert 0 <= rep["first_declined"] < len(raw) and raw[rep["first_declined"]:rep["first_declined"] + 1] == b"[", (what, rep)
        return
    assert rep["status"] == fc.FIND_OK and rep["first_declined"] == fc.NO_OFFSET, (what, rep)
    assert rep["n_found"] == n and got == want, (what, raw[:120], min_values, want[:4], got[:4], rep)


@pytest.mark.parametrize("corpus", ["event_texts", "strings", "edits", "failures", "boundaries", "long_tokens"])
def test_the_blocks_equal_the_host_finder_on_every_corpus(corpus):
    cases = getattr(fc, corpus)()
    assert len(cases) >= 10
    for name, raw, min_values in cases:
        _agree(raw, min_values, name, may_decline=name in fc.DECLINE)
    if corpus == "long_tokens":
        assert {name for name, _, _ in cases} >= fc.DECLINE


def test_the_corpora_hold_what_they_are_meant_to():
    cases = {name: (raw, mv) for name, raw, mv in fc.all_cases()}
    assert len(cases) == len(fc.all_cases()), "case names are unique"
    found = lambda name: fc.host_find(*cases[name])[1]                                  # noqa: E731
    assert found("event-new-1-2-min1") == 2 and found("event-new-2-2-min12") == 2 and found("event-new-4-4-min1") == 5
    assert found("event-new-small-1d-3d-2-min1") == 5 and found("event-new-small-1d-3d-2-min12") == 3 and found("event-new-small-1d-3d-2-min13") == 0
    assert found("matrix-over-256-groups") == 1 and found("matrix-over-256-groups-ragged") == 0
    assert found("long-64-inside") == 1 and found("long-65-inside") == 1 and found("ws-run-candidate") == 1 and found("ws-run-inside") == 1
    assert len(cases["matrix-over-256-groups"][0]) > 256 * fc.GROUP and len(cases["ws-run-inside"][0]) > 2 * fc.GROUP
    assert sum(1 for name in cases if name.startswith("edit-")) > 700


def test_two_hundred_thousand_random_short_texts():
    texts = fc.random_short(101, 200_000)
    assert len(texts) == 200_000
    some = 0
    for raw, min_values in texts:
        want, n = fc.host_find(raw, min_values)
        got, rep = fc.blocks_find(raw, min_values)
        assert rep["status"] == fc.FIND_OK and rep["n_found"] == n and got == want, (raw, min_values, want, got, rep)
        some += n > 0
    assert some > 10_000                                           # the alphabet does produce matrices


def test_two_thousand_random_texts_of_8_to_20_kib():
    texts = fc.random_long(102, 2_000)
    total = 0
    for raw, min_values in texts:
        assert 8 * 1024 <= len(raw) <= 20 * 1024
        want, n = fc.host_find(raw, min_values, cap=512)
        got, rep = fc.blocks_find(raw, min_values, cap=512)
        assert rep["status"] == fc.FIND_OK and rep["n_found"] == n and got == want, (raw[:80], min_values, rep)
        total += n
    assert total > 20_000


def test_hypothesis_drives_the_same_comparison():
    hypothesis = pytest.importorskip("hypothesis")
    from hypothesis import strategies as st

    @hypothesis.settings(max_examples=1000, deadline=None, derandomize=True, database=None)
    @hypothesis.given(st.lists(st.sampled_from(fc.PIECES), min_size=1, max_size=40), st.integers(1, 6))
    def run(pieces, min_values):
        _agree(b"".join(pieces), min_values, "hypothesis")
    run()


def test_cap_limits_what_is_written_not_what_is_counted():
    raw = b"[[1,2]],[[3],[4]] [[5]]"
    want, n = fc.host_find(raw, 1)
    assert n == 3
    for cap in (0, 1, 2, 3):
        got, rep = fc.blocks_find(raw, 1, cap=cap)
        assert rep["n_found"] == 3 and rep["n_candidates"] == 3 and got == want[:cap]


def test_more_candidates_than_the_event_list_holds_decline_and_fewer_do_not():
    fits = b"[[1]]" * fc.MAX_CANDIDATES
    got, rep = fc.blocks_find(fits, 1, cap=4)
    assert rep["status"] == fc.FIND_OK and rep["n_found"] == fc.MAX_CANDIDATES == rep["n_candidates"] and got == fc.host_find(fits, 1, cap=4)[0]
    over = fits + b" [[2]]"
    got, rep = fc.blocks_find(over, 1, cap=4)
    assert rep["status"] == fc.FIND_DECLINED and rep["n_found"] == 0 and rep["first_declined"] == len(fits) + 1
    lone = b"[[," * (fc.MAX_CANDIDATES - 1) + b"[[7]]"               # candidates that no closer follows take one entry each
    got, rep = fc.blocks_find(lone, 1, cap=4)
    assert rep["status"] == fc.FIND_OK and rep["n_candidates"] == fc.MAX_CANDIDATES
    assert got == fc.host_find(lone, 1, cap=4)[0] == [(len(lone) - 5, len(lone), 1, 1)]


def test_abi_symbols_are_declared_exported_and_bound():
    from hippomm_amd import _lib
    header = (fc.ROOT / "include" / "hippomm_hip.h").read_text()
    lib = _lib.load()
    for name in ("hmm_json_find_matrices_device_workspace_bytes", "hmm_json_find_matrices_device", "hmm_json_find_matrices_blocks"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib._SIGNATURES and getattr(lib, name).argtypes is not None, name
    assert "typedef struct hmm_json_find_report { uint64_t n_found, n_candidates, status, first_declined; } hmm_json_find_report;" in header
    assert lib.hmm_abi_version() == 7                                # new entries only: nothing that existed changed


def test_workspace_query_is_monotone_and_refuses_what_the_call_refuses():
    from hippomm_amd import _lib
    q = _lib.load().hmm_json_find_matrices_device_workspace_bytes
    assert q(0) == 0 and q(fc.MAX_SPAN + 1) == 0 and q(fc.MAX_SPAN) > 0
    sizes = [q(n) for n in (1, 2, fc.GROUP - 1, fc.GROUP, fc.GROUP + 1, 2 * fc.GROUP, 10 ** 6, 10 ** 8, 10 ** 9, fc.MAX_SPAN)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[4] > sizes[3] == sizes[0]
    assert all(s % 8 == 0 for s in sizes)


def test_every_argument_error_is_reported_without_a_gpu():
    from hippomm_amd import _lib
    lib = _lib.load()
    n = 100
    ws_bytes = lib.hmm_json_find_matrices_device_workspace_bytes(n)
    base = 1 << 20                                                   # addresses that are never dereferenced: every call must refuse
    good = dict(text=base + 3, len=n, min_values=1, out=base + 4096, cap=4, report=base + 8192, ws=base + 16384, ws_bytes=ws_bytes)

    def call(**change):
        a = dict(good, **change)
        return lib.hmm_json_find_matrices_device(a["text"], a["len"], a["min_values"], a["out"], a["cap"], a["report"], a["ws"], a["ws_bytes"], None)

    for change in (dict(text=None), dict(report=None), dict(ws=None), dict(out=None), dict(cap=-1), dict(len=0), dict(len=fc.MAX_SPAN + 1),
                   dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0), dict(ws=good["ws"] + 4), dict(report=good["report"] + 1), dict(out=good["out"] + 2),
                   dict(len=n + 10 * fc.GROUP)):
        assert call(**change) == -1, change
        assert b"json_find_matrices_device" in lib.hmm_last_error(), change
    # the host twin checks its own arguments too
    report = (C.c_uint64 * 4)()
    assert lib.hmm_json_find_matrices_blocks(None, 5, 1, None, 0, C.cast(report, C.c_void_p)) == -1
    assert lib.hmm_json_find_matrices_blocks(b"[[1]]", 0, 1, None, 0, C.cast(report, C.c_void_p)) == -1
    assert lib.hmm_json_find_matrices_blocks(b"[[1]]", 5, 1, None, 1, C.cast(report, C.c_void_p)) == -1
    assert lib.hmm_json_find_matrices_blocks(b"[[1]]", 5, 1, None, -1, C.cast(report, C.c_void_p)) == -1
    assert lib.hmm_json_find_matrices_blocks(b"[[1]]", 5, 1, None, 0, C.cast(report, C.c_void_p)) == 0 and report[0] == 1


def test_python_entry_points_default_to_the_host_finder_and_refuse_a_device_finder_without_a_device_parser(tmp_path):
    from hippomm_amd import event_store as es
    for fn in (es.parse_event_features, es.build_event_store, es.refresh_event_store):
        assert inspect.signature(fn).parameters["find"].default == "host", fn.__name__
    assert inspect.signature(es.find_matrices_device).parameters["min_values"].default == es.NATIVE_MIN_VALUES
    assert set(es.matrix_find_stats()) == {"device", "declined", "host"}
    path = tmp_path / "e.json"
    path.write_text('{"features": {"vision": [[1.0, 2.0]]}, "feature_times": {"vision": [0.0]}}')
    with pytest.raises(ValueError, match="find='device'"):
        es.parse_event_features(path, find="device")
    with pytest.raises(ValueError, match="find must be"):
        es.parse_event_features(path, find="gpu")
    with pytest.raises(ValueError, match="find='device'"):
        es.build_event_store(tmp_path, find="device")
    with pytest.raises(ValueError, match="find='device'"):
        es.refresh_event_store(None, [], tmp_path, find="device")
    with pytest.raises(TypeError):
        es.find_matrices_device("not bytes")
    feats, _ = es.parse_event_features(path)                         # the defaults: the host route, untouched
    assert feats["vision"].tolist() == [[1.0, 2.0]]
