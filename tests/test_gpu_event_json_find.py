"""GPU: hmm_json_find_matrices_device against the host finder hmm_json_find_matrices on every corpus of event_json_find_cases --
list, n_found and status, the text at byte shifts 0, 1, 3 and 15 from an aligned base --, what `cap` limits, and the Python route
end to end: parse_event_features(find="device") and build_event_store(find="device") give the bits of their find="host" calls, and a
text the device declines is searched by the host finder and counted."""
import json
import logging
import shutil

import numpy as np
import pytest
import torch

import event_json_find_cases as fc

pytestmark = pytest.mark.gpu

SHIFTS = (0, 1, 3, 15)
_expected = {}


@pytest.fixture(autouse=True)
def _fresh_route():
    """Every test starts with both device routes on and their self-checks already passed, unless it says otherwise."""
    from hippomm_amd import event_store as es
    es._parse_route["on"], es._parse_check["ok"] = True, True
    es._find_route["on"], es._find_check["ok"] = True, True
    yield
    es._parse_route["on"], es._parse_check["ok"] = True, None
    es._find_route["on"], es._find_check["ok"] = True, None


def _host(name, raw, min_values):
    if name not in _expected:
        _expected[name] = fc.host_find(raw, min_values)
    return _expected[name]


def device_find(raw, min_values=1, cap=fc.CAP, shift=0):
    """One call on a text that starts `shift` bytes behind an aligned base -> (the list, the report, the words behind the list)."""
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    buf = torch.full((len(raw) + shift,), ord("["), dtype=torch.uint8, device=dev)
    buf[shift:] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    out = torch.full((4 + 4 * max(cap, 1),), -1, dtype=torch.int64, device=dev)
    ws_bytes = lib.hmm_json_find_matrices_device_workspace_bytes(len(raw))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    assert lib.hmm_json_find_matrices_device(buf.data_ptr() + shift, len(raw), min_values, out.data_ptr() + 32 if cap else None, cap, out.data_ptr(),
                                             ws.data_ptr(), ws_bytes, _lib.stream_ptr()) == 0, lib.hmm_last_error()
    torch.cuda.synchronize()
    w = out.cpu().numpy().view(np.uint64)
    rep = dict(n_found=int(w[0]), n_candidates=int(w[1]), status=int(w[2]), first_declined=int(w[3]))
    listed = min(rep["n_found"], cap)
    return [tuple(int(v) for v in e) for e in w[4:4 + 4 * listed].reshape(-1, 4)], rep, w[4 + 4 * listed:]


@pytest.mark.parametrize("corpus", ["event_texts", "strings", "edits", "failures", "boundaries", "long_tokens"])
def test_the_device_equals_the_host_finder_on_every_corpus_at_every_shift(corpus):
    for name, raw, min_values in getattr(fc, corpus)():
        want, n = _host(name, raw, min_values)
        for shift in SHIFTS:
            got, rep, _ = device_find(raw, min_values, shift=shift)
            if name in fc.DECLINE:
                assert rep["status"] == fc.FIND_DECLINED and rep["n_found"] == 0, (name, shift, rep)
                assert raw[rep["first_declined"]:rep["first_declined"] + 1] == b"[", (name, shift, rep)
                continue
            assert rep["status"] == fc.FIND_OK and rep["first_declined"] == fc.NO_OFFSET, (name, shift, rep)
            assert rep["n_found"] == n and got == want, (name, shift, min_values, want[:4], got[:4], rep)
            assert rep == fc.blocks_find(raw, min_values)[1], (name, shift)           # the host twin reports the same words


def test_random_texts_as_one_long_text_and_alone():
    texts = fc.random_long(103, 12)
    for raw, min_values in texts:
        want, n = fc.host_find(raw, min_values, cap=512)
        got, rep, _ = device_find(raw, min_values, cap=512, shift=3)
        assert rep["status"] == fc.FIND_OK and rep["n_found"] == n and got == want, (raw[:80], rep)
    joined = b"\n".join(raw for raw, _ in texts)
    want, n = fc.host_find(joined, 3, cap=4096)
    got, rep, _ = device_find(joined, 3, cap=4096, shift=1)
    assert n > 100 and rep["status"] == fc.FIND_OK and rep["n_found"] == n and got == want


@pytest.mark.parametrize("cap", [0, 1])
def test_cap_against_three_matrices(cap):
    raw = b'{"a":[[1,2]],"b":[[3],[4]],"c": [[5]]}'
    want, n = fc.host_find(raw, 1)
    assert n == 3
    got, rep, behind = device_find(raw, 1, cap=cap)
    assert rep["n_found"] == 3 and rep["status"] == fc.FIND_OK and got == want[:cap]
    assert (behind == np.uint64(2 ** 64 - 1)).all()                  # only `cap` entries are written


def test_more_candidates_than_the_event_list_holds():
    fits = b"[[1]]" * fc.MAX_CANDIDATES
    got, rep, _ = device_find(fits, 1, cap=4)
    assert rep["status"] == fc.FIND_OK and rep["n_found"] == fc.MAX_CANDIDATES and got == fc.host_find(fits, 1, cap=4)[0]
    got, rep, _ = device_find(fits + b" [[2]]", 1, cap=4)
    assert rep["status"] == fc.FIND_DECLINED and rep["n_found"] == 0 and rep["first_declined"] == len(fits) + 1 and got == []


# ---- the Python route ---------------------------------------------------------------------------------------------------------------
def test_find_matrices_device_takes_bytes_and_tensors():
    from hippomm_amd import event_store as es
    raw = dict((name, raw) for name, raw, _ in fc.event_texts())["event-new-4-2-min1"]
    want, n = fc.host_find(raw, 1)
    assert n == 5
    stats = {}
    before = es.matrix_find_stats()
    assert es.find_matrices_device(raw, 1, stats=stats) == want
    assert stats == dict(route="device", n_found=5, n_candidates=5, status=fc.FIND_OK, first_declined=fc.NO_OFFSET)
    t = torch.frombuffer(bytearray(b"xyz" + raw), dtype=torch.uint8).cuda()[3:]
    assert es.find_matrices_device(t, 1) == want and es.find_matrices_device(t, 12) == fc.host_find(raw, 12)[0]
    assert es.find_matrices_device(raw) == []                          # nothing reaches the default min_values
    many = b",".join([b"[[1,2],[3,4]]"] * 40)                          # more than the first read-back brings
    assert es.find_matrices_device(many, 1) == fc.host_find(many, 1)[0] and len(es.find_matrices_device(many, 1)) == 40
    after = es.matrix_find_stats()
    assert after["device"] - before["device"] == 6 and after["declined"] == before["declined"] and after["host"] == before["host"]


def test_a_declined_text_is_searched_by_the_host_finder_and_counted():
    from hippomm_amd import event_store as es
    raw = dict((name, raw) for name, raw, _ in fc.long_tokens())["long-65-inside"]
    before = es.matrix_find_stats()
    for text in (raw, torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()):
        stats = {}
        assert es.find_matrices_device(text, 1, stats=stats) == fc.host_find(raw, 1)[0] != []
        assert stats["route"] == "host" and stats["status"] == fc.FIND_DECLINED and stats["first_declined"] == raw.index(b"[[")
    after = es.matrix_find_stats()
    assert after["declined"] - before["declined"] == 2 and after["device"] == before["device"]


def test_self_check_runs_once_and_a_failed_one_turns_the_route_off(monkeypatch, caplog):
    from hippomm_amd import event_store as es
    raw = b'{"m":[[1,2],[3,4]]}'
    es._find_check["ok"] = None
    calls = []
    real = es._find_by_host
    monkeypatch.setattr(es, "_find_by_host", lambda *a: calls.append(1) or real(*a))
    assert es.find_matrices_device(raw, 1) == [(5, 18, 2, 2)] and es.find_matrices_device(raw, 1) == [(5, 18, 2, 2)]
    assert calls == [1] and es._find_check["ok"] is True
    es._find_check["ok"] = None
    monkeypatch.setattr(es, "_find_by_host", lambda *a: calls.append(2) or real(*a) + ([(0, 1, 1, 1)] if len(calls) == 2 else []))
    stats = {}
    with caplog.at_level(logging.WARNING, logger=es._log.name):
        assert es.find_matrices_device(raw, 1, stats=stats) == [(5, 18, 2, 2)]
    assert es._find_check["ok"] is False and stats["route"] == "host" and "span finder disagrees" in caplog.text
    before = es.matrix_find_stats()
    assert es.find_matrices_device(raw, 1, stats=stats) == [(5, 18, 2, 2)] and stats["route"] == "host"
    assert es.matrix_find_stats()["host"] == before["host"] + 1


@pytest.fixture(scope="module")
def memory_store(tmp_path_factory):
    """Three events without sidecars: a two-modality new-format file, an old-format file, and one without vision."""
    from hippomm_amd import event_store as es
    base = tmp_path_factory.mktemp("find_store")
    rng = np.random.default_rng(14)
    index = {}
    vision, audio = rng.standard_normal((40, 1024)).astype(np.float32), rng.standard_normal((3, 1024)).astype(np.float32)
    new = {"features": {"vision": vision, "audio": audio, "vision_times": (np.arange(40) * 0.5).tolist(), "audio_times": [0.0, 1.0, 2.0]},
           "summary": 'new "format" [[1, 2], [3, 4]]'}
    path = es.save_event(new, base / "events" / "v" / "e0.json", write_sidecars=False)
    index["e0"] = {"file_path": str(path), "video_id": "v"}
    old = {"event_id": "e1", "summary": "old \\ format", "features": {
        "vision": {"features": rng.standard_normal((7, 1024)).astype(np.float32).astype(np.float64).tolist(), "times": (np.arange(7) * 0.25).tolist()},
        "audio": {"features": audio.astype(np.float64).tolist(), "times": [0.0, 1.0, 2.0]}}}
    path = base / "events" / "v" / "e1.json"
    path.write_text(json.dumps(old, indent=2))
    index["e1"] = {"file_path": str(path), "video_id": "v"}
    path = es.save_event({"features": {"audio": audio, "audio_times": [0.0, 1.0, 2.0]}, "summary": "no vision"}, base / "events" / "v" / "e2.json",
                         write_sidecars=False)
    index["e2"] = {"file_path": str(path), "video_id": "v"}
    (base / "event_index.json").write_text(json.dumps(index))
    return base, index


@pytest.mark.parametrize("name", ["e0", "e1"], ids=["new-format-two-modalities", "old-format"])
def test_event_file_end_to_end(memory_store, name):
    from hippomm_amd import event_store as es
    base, _ = memory_store
    path = base / "events" / "v" / f"{name}.json"
    host_stats, dev_stats = {}, {}
    before = es.matrix_find_stats()
    want, want_times = es.parse_event_features(path, matrices="device", find="host", stats=host_stats)
    assert es.matrix_find_stats() == before                            # find="host" never touches the device finder
    got, got_times = es.parse_event_features(path, matrices="device", find="device", stats=dev_stats)
    assert es.matrix_find_stats()["device"] == before["device"] + 1
    assert dev_stats == host_stats == {"device": 2, "host": 0, "json": 0} and set(got) == set(want) == {"vision", "audio"}
    for modality in want:
        assert got[modality].is_cuda and got[modality].dtype == want[modality].dtype and got[modality].shape == want[modality].shape
        assert got[modality].cpu().numpy().tobytes() == want[modality].cpu().numpy().tobytes(), modality
    assert set(got_times) == set(want_times) and all(np.array_equal(got_times[k], want_times[k]) for k in want_times)
    plain, _ = es.parse_event_features(path)                           # and both are the host route's bits
    assert all(got[m].cpu().numpy().tobytes() == plain[m].tobytes() for m in plain)


def test_store_built_and_refreshed_with_the_device_finder(memory_store, tmp_path):
    from hippomm_amd import event_store as es
    base, index = memory_store

    def copy(to, names):
        shutil.copytree(base / "events", to / "events")
        (to / "event_index.json").write_text(json.dumps({k: dict(index[k], file_path=str(to / "events" / "v" / f"{k}.json")) for k in names}))
        return to
    a, b = copy(tmp_path / "a", ("e0", "e1")), copy(tmp_path / "b", ("e0", "e1"))
    before = es.matrix_find_stats()
    host, host_ids = es.build_event_store(a, parse="device", find="host")
    assert es.matrix_find_stats() == before
    dev, dev_ids = es.build_event_store(b, parse="device", find="device")
    assert es.matrix_find_stats()["device"] == before["device"] + 2
    assert host_ids == dev_ids and host.lengths == dev.lengths == [40, 7]
    assert torch.equal(host.offsets, dev.offsets) and host.rows.cpu().numpy().tobytes() == dev.rows.cpu().numpy().tobytes()
    for d in (a, b):
        (d / "event_index.json").write_text(json.dumps({k: dict(index[k], file_path=str(d / "events" / "v" / f"{k}.json")) for k in index}))
    host_ids = es.refresh_event_store(host, host_ids, a, parse="device", find="host")
    dev_ids = es.refresh_event_store(dev, dev_ids, b, parse="device", find="device")
    assert host_ids == dev_ids == ["e0", "e1", "e2"] and dev.lengths == [40, 7, 0]
    assert host.rows.cpu().numpy().tobytes() == dev.rows.cpu().numpy().tobytes()
    for name in dev_ids:
        for modality in ("vision", "audio"):
            pa, pb = (es._sidecar_paths(d / "events" / "v" / f"{name}.json", modality)[0] for d in (a, b))
            assert pa.exists() == pb.exists() and (not pa.exists() or np.load(pa).tobytes() == np.load(pb).tobytes()), (name, modality)


def test_a_declined_event_file_takes_the_host_finder(tmp_path):
    from hippomm_amd import event_store as es
    rng = np.random.default_rng(15)
    m = rng.standard_normal((2, 1024)).astype(np.float32).astype(np.float64).tolist()
    m[0][0] = 0.5
    text = json.dumps({"features": {"vision": m}, "feature_times": {"vision": [0.0, 0.5]}}, indent=2)
    first = json.dumps(m[0][0])
    text = text.replace(first, first + "0" * (fc.TOKEN_MAX + 1 - len(first)), 1)            # the same value, 65 bytes long
    path = tmp_path / "long.json"
    path.write_text(text)
    before = es.matrix_find_stats()
    want, _ = es.parse_event_features(path, matrices="device", find="host")
    got, _ = es.parse_event_features(path, matrices="device", find="device")
    after = es.matrix_find_stats()
    assert after["declined"] == before["declined"] + 1 and after["device"] == before["device"]
    assert got["vision"].is_cuda and got["vision"].cpu().numpy().tobytes() == want["vision"].cpu().numpy().tobytes()
    assert tuple(got["vision"].shape) == (2, 1024)
