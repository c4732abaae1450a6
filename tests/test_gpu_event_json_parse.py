"""GPU: the device JSON parser (hmm_json_parse_matrix_device behind event_store.parse_matrix_device /
parse_event_features(matrices="device") / build_event_store(parse="device")) gives the bits of the host parser
(hmm_json_parse_matrix_f32) for fp32 and of np.array(json.loads(span)) for fp64 -- per matrix at every seam of its launch plan,
for every alignment of the text, with flagged values patched, with every status handed to the host route -- and per event file
and store."""
import json
import logging
import shutil

import numpy as np
import pytest
import torch

import event_json_parse_cases as pc

pytestmark = pytest.mark.gpu

G = pc.GROUP_BYTES
ROUND = pc.SCAN_GROUPS_PER_ROUND * G                               # bytes of text one round of the scan kernel covers
STYLES = ("indent", "compact", "crlf")
ODD = [b"NaN", b"-Infinity", b"Infinity", b"-0.0", b"-0", b"0", b"1e-05", b"5e-324", b"1.7976931348623157e308", b"-0e0", b"1E5", b"12"]


@pytest.fixture(autouse=True)
def _fresh_route():
    """Every test starts with the route on and the self-check already passed, unless it says otherwise."""
    from hippomm_amd import event_store as es
    es._parse_route["on"], es._parse_check["ok"] = True, True
    yield
    es._parse_route["on"], es._parse_check["ok"] = True, None


@pytest.fixture(scope="module")
def tokens():
    """fp32-origin literals, as an event file holds them, with the odd spellings in between; made once."""
    out = pc.f32_origin(np.random.default_rng(11), 60_000)[:60_000]
    out[::97] = (ODD * (len(out[::97]) // len(ODD) + 1))[:len(out[::97])]
    return out


def _lib():
    from hippomm_amd import _lib
    return _lib.load()


def _agrees(raw, span, stats_want=None, dtype_list=(np.float32, np.float64), raw_for_device=None):
    """The public function on (raw, span) against the host parser (fp32) and json (fp64), as bits."""
    from hippomm_amd import event_store as es
    for dtype in dtype_list:
        want = pc.host_f32(_lib(), raw, span) if dtype == np.float32 else pc.json_f64(raw, span)
        assert want is not None
        stats = {}
        got = es.parse_matrix_device(raw if raw_for_device is None else raw_for_device, span, dtype, stats=stats)
        assert got.is_cuda and tuple(got.shape) == want.shape and got.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
        assert got.cpu().numpy().tobytes() == want.tobytes(), (span, np.dtype(dtype).name, stats)
        for key, value in (stats_want or {"route": "device", "status": pc.OK}).items():
            assert stats[key] == value, (key, stats)


def _padded(tokens, cols, style, length) -> bytes:
    """text_of(...) with spaces in front of its last bracket, `length` bytes in all."""
    base = pc.text_of(tokens, cols, style)
    assert len(base) <= length, (len(base), length)
    return base[:-1] + b" " * (length - len(base)) + b"]"


def _raw_call(raw, span, f64=False, cap=8, shift=0):
    """The C ABI itself, the text `shift` bytes into its allocation -> (out as bits, report, flagged entries)."""
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    begin, end, rows, cols = span
    buf = torch.zeros(shift + len(raw), dtype=torch.uint8, device=dev)
    buf[shift:] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    out = torch.full((rows * cols,), 0x5A5A5A5A5A5A5A5A if f64 else 0x5A5A5A5A, dtype=torch.int64 if f64 else torch.int32, device=dev)
    report = torch.full((4 + 4 * cap,), -7, dtype=torch.int64, device=dev)
    ws_bytes = lib.hmm_json_parse_matrix_device_workspace_bytes(end - begin)
    ws = torch.full((ws_bytes // 8,), -1, dtype=torch.int64, device=dev)
    rc = lib.hmm_json_parse_matrix_device(buf.data_ptr() + shift, begin, end, rows, cols, 1 if f64 else 0, out.data_ptr(), report.data_ptr(),
                                          report.data_ptr() + 32, cap, ws.data_ptr(), ws_bytes, _lib.stream_ptr())
    assert rc == 0, lib.hmm_last_error()
    torch.cuda.synchronize()
    words = report.cpu().numpy().view(np.uint64)
    rep = dict(n_tokens=int(words[0]), n_flagged=int(words[1]), first_bad=int(words[2]), status=int(words[3]))
    entries = sorted(tuple(e) for e in words[4:4 + 4 * min(rep["n_flagged"], cap)].reshape(-1, 4).tolist())
    assert (words[4 + 4 * min(rep["n_flagged"], cap):] == np.uint64(2 ** 64 - 7)).all()           # nothing behind the entries
    return out.cpu().numpy().view(np.uint64 if f64 else np.uint32), rep, entries


# ---- per matrix -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", STYLES)
def test_smallest_shapes(tokens, style):
    for shape in ((1, 1), (1, 7), (7, 1), (3, 5)):
        for first in (0, 97 * 3 - 2):                                # plain literals, and a stretch with odd spellings in it
            raw = pc.text_of(tokens[first:first + shape[0] * shape[1]], shape[1], style)
            span = pc.find_span(_lib(), raw)
            assert span == (0, len(raw)) + shape
            _agrees(raw, span)


@pytest.mark.parametrize("length", [G - 1, G, G + 1, 2 * G, ROUND + G, ROUND + G + 1], ids=lambda n: f"{n}B")
def test_text_lengths_around_a_group_and_a_scan_round(tokens, length):
    cols = 7
    n = (length - 64) // 27 // cols * cols                          # compact: at most 25 bytes per literal and 2 of separator
    raw = _padded(tokens[:n], cols, "compact", length)
    span = pc.find_span(_lib(), raw)
    assert span == (0, length, n // cols, cols)
    _agrees(raw, span, dtype_list=(np.float32,) if length > 4 * G else (np.float32, np.float64))


def test_tokens_on_the_seam_between_two_groups(tokens):
    """A token that starts on the last byte of a group, one that ends on the first byte of the next, a one-byte token on either
    side of a seam, and the longest token the device takes starting on a group's last byte."""
    longest =(b"0." + b"1234567890" * 7)[:pc.TOKEN_MAX]
    placed = [(G - 1, tokens[5]), (2 * G - len(tokens[6]) + 1, tokens[6]), (3 * G - 1, b"7"), (4 * G, b"8"), (5 * G - 1, longest),
              (6 * G - 1, b"-1.5"), (7 * G - 2, b"1e5")]
    text = b"[[0.5,"
    for at, token in placed:
        assert len(text) < at
        text += b" " * (at - len(text)) + token + b","
    raw = text + b"2.5]]"
    span = pc.find_span(_lib(), raw)
    assert span == (0, len(raw), 1, len(placed) + 2)
    for at, token in placed:
        assert raw[at:at + len(token)] == token
    _agrees(raw, span, stats_want={"route": "device"})


def test_every_alignment_of_the_span_and_of_the_text(tokens):
    """The span begins at every offset modulo 16 of a larger buffer whose neighbouring bytes would be numbers if they were read,
    and the text tensor itself starts 0 to 3 bytes into its allocation."""
    small = pc.text_of(tokens[:15], 5, "indent")
    large = pc.text_of(tokens[:5 * 70], 70, "compact")
    assert G < len(large) < 3 * G
    lib = _lib()
    for body, shape in ((small, (3, 5)), (large, (5, 70))):
        for lead in range(16):
            raw = b"12345678,1234567"[:lead] + body + b"12345,6.5,[7]"
            span = (lead, lead + len(body)) + shape
            want = pc.host_f32(lib, raw, span).view(np.uint32).reshape(-1)
            for shift in ((0, 1, 2, 3) if lead < 4 else (lead % 4,)):
                got, rep, entries = _raw_call(raw, span, shift=shift)
                assert rep == dict(n_tokens=shape[0] * shape[1], n_flagged=0, first_bad=pc.NO_OFFSET, status=pc.OK), (lead, shift, rep)
                assert (got == want).all(), (lead, shift)
    from hippomm_amd import event_store as es
    raw = b"{\"a\": " + large + b"}"
    on_device = torch.frombuffer(bytearray(b"#" + raw), dtype=torch.uint8).cuda()[1:]
    _agrees(raw, (6, 6 + len(large), 5, 70), raw_for_device=on_device)
    assert es.matrix_parse_stats()["device"] >= 2


def test_token_lengths(tokens):
    def of_length(n):
        return b"1234567890123456789"[:n] if n <= 19 else b"1." + b"23456789012345678"[:n - 7] + b"e-105"
    toks = [of_length(n) for n in range(1, 25)]
    assert [len(t) for t in toks] == list(range(1, 25))
    too_long = b"0." + b"3" * (pc.TOKEN_MAX - 1)
    assert len(too_long) == pc.TOKEN_MAX + 1
    toks.insert(11, too_long)
    raw = pc.text_of(toks, 5, "indent")
    span = pc.find_span(_lib(), raw)
    got, rep, entries = _raw_call(raw, span)
    at = raw.index(too_long)
    assert rep == dict(n_tokens=25, n_flagged=1, first_bad=pc.NO_OFFSET, status=pc.OK)
    assert entries == [(11, at, at + len(too_long), pc.TOO_LONG)] and got[11] == 0
    want = pc.host_f32(_lib(), raw, span).view(np.uint32).reshape(-1)
    assert (np.delete(got, 11) == np.delete(want, 11)).all()
    _agrees(raw, span, stats_want={"route": "device", "n_flagged": 1})


# ---- flags and statuses -----------------------------------------------------------------------------------------------------------
def _midpoint_literal(x: float) -> bytes:
    lit = pc._written_out(pc._midpoint(x))
    assert 19 < len(lit) <= pc.TOKEN_MAX and pc.expected_flag(lit) == pc.UNDECIDED
    return lit


def test_flagged_values_are_patched(tokens, monkeypatch):
    from hippomm_amd import event_store as es
    toks = list(tokens[:15])
    toks[4], toks[13] = _midpoint_literal(2.0 ** 70 * 1.2345), b"-" + _midpoint_literal(0.0123456789)
    raw = pc.text_of(toks, 5, "indent")
    span = pc.find_span(_lib(), raw)
    got, rep, entries = _raw_call(raw, span, f64=True)
    assert rep["n_flagged"] == 2 and rep["status"] == pc.OK and [e[0] for e in entries] == [4, 13]
    assert [e[3] for e in entries] == [pc.UNDECIDED] * 2 and [raw[e[1]:e[2]] for e in entries] == [toks[4], toks[13]]
    assert got[4] == 0 and got[13] == 0                             # their slots are defined
    _, short, listed = _raw_call(raw, span, cap=1)                  # one entry short: both are counted, one is listed
    assert short["n_flagged"] == 2 and len(listed) == 1
    _agrees(raw, span, stats_want={"route": "device", "n_flagged": 2})
    monkeypatch.setattr(es, "FLAGGED_CAP", 1)
    _agrees(raw, span, stats_want={"route": "host", "n_flagged": 2}, dtype_list=(np.float32,))


def test_a_literal_outside_the_double_range_goes_to_json(tokens):
    from hippomm_amd import event_store as es
    toks = list(tokens[:15])
    toks[7] = b"1e400"
    raw = pc.text_of(toks, 5, "indent")
    span = pc.find_span(_lib(), raw)
    assert pc.host_f32(_lib(), raw, span) is None                   # the host route declines as well
    stats = {}
    got = es.parse_matrix_device(raw, span, stats=stats)
    assert stats["route"] == "json" and stats["n_flagged"] == 1 and stats["status"] == pc.OK
    with np.errstate(over="ignore"):
        assert got.cpu().numpy().tobytes() == pc.json_f64(raw, span).astype(np.float32).tobytes() and bool(torch.isinf(got[1, 2]))


def test_statuses_hand_the_matrix_to_the_other_routes(tokens):
    from hippomm_amd import event_store as es
    toks = list(tokens[:15])
    raw = pc.text_of(toks, 5, "indent")
    begin, end, rows, cols = pc.find_span(_lib(), raw)
    # rows overstated by one: nothing behind the tokens that exist is written, json answers with the rows it finds
    got, rep, _ = _raw_call(raw, (begin, end, rows + 1, cols))
    assert rep["status"] == pc.COUNT and rep["n_tokens"] == 15 and (got[15:] == 0x5A5A5A5A).all()
    assert (got[:15] == pc.host_f32(_lib(), raw, (begin, end, rows, cols)).view(np.uint32).reshape(-1)).all()
    stats = {}
    out = es.parse_matrix_device(raw, (begin, end, rows + 1, cols), stats=stats)
    assert stats["route"] == "json" and stats["status"] == pc.COUNT
    assert out.cpu().numpy().tobytes() == pc.json_f64(raw, (begin, end)).astype(np.float32).tobytes()
    # a foreign byte inside a token, and a token that is no JSON number: json raises, as it would for the file
    # the foreign byte goes where what is left in front of it is still a number: only the byte itself is wrong
    at = raw.index(toks[8]) + max(i for i in range(1, len(toks[8])) if pc.NUMBER.fullmatch(toks[8][:i]))
    for broken, status, where in ((raw[:at] + b"x" + raw[at + 1:], pc.BAD_BYTE, at),
                                  (raw.replace(toks[8], b"1." + b" " * (len(toks[8]) - 2)), pc.BAD_TOKEN, raw.index(toks[8]))):
        assert len(broken) == len(raw)
        _, rep, _ = _raw_call(broken, (begin, end, rows, cols))
        assert rep["status"] == status and rep["first_bad"] == where and rep["n_tokens"] == 15, rep
        stats = {}
        with pytest.raises(ValueError):
            es.parse_matrix_device(broken, (begin, end, rows, cols), stats=stats)
        assert stats["status"] == status and "route" not in stats


# ---- self-check -------------------------------------------------------------------------------------------------------------------
def test_self_check_runs_once_and_a_failed_one_turns_the_route_off(tokens, monkeypatch, caplog):
    from hippomm_amd import event_store as es
    raw = pc.text_of(tokens[:15], 5, "indent")
    span = pc.find_span(_lib(), raw)
    es._parse_check["ok"] = None
    calls = []
    real = es._edge_rows_agree
    monkeypatch.setattr(es, "_edge_rows_agree", lambda *a: calls.append(1) or real(*a))
    for _ in range(2):
        _agrees(raw, span)
    assert calls == [1] and es._parse_check["ok"] is True
    es._parse_check["ok"] = None
    monkeypatch.setattr(es, "_edge_rows_agree", lambda *a: False)
    with caplog.at_level(logging.WARNING, logger="hippomm_amd.event_store"):
        _agrees(raw, span, stats_want={"route": "host"}, dtype_list=(np.float32,))
    assert es._parse_check["ok"] is False and any("disagrees" in r.getMessage() for r in caplog.records)
    stats = {}
    es.parse_matrix_device(raw, span, stats=stats)
    assert stats == {"route": "host"}                                # the device is not asked again


# ---- an event file and a store ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def memory_store(tmp_path_factory):
    """Three events without sidecars -- 600 x 1024 fp32 vision features, one event without vision, one with 37 rows -- and a
    fourth file that the index does not name yet."""
    from hippomm_amd import event_store as es
    base = tmp_path_factory.mktemp("store")
    rng = np.random.default_rng(12)
    index = {}
    for i, rows in enumerate((600, None, 37, 5)):
        feats = {"audio": rng.standard_normal((3, 1024)).astype(np.float32), "audio_times": [0.0, 1.0, 2.0]}
        if rows is not None:
            feats.update(vision=rng.standard_normal((rows, 1024)).astype(np.float32), vision_times=(np.arange(rows) * 0.5).tolist())
        path = es.save_event({"features": feats, "summary": f"event {i}"}, base / "events" / "v" / f"e{i}.json", write_sidecars=False)
        index[f"e{i}"] = {"file_path": str(path), "video_id": "v"}
    (base / "event_index.json").write_text(json.dumps({k: index[k] for k in ("e0", "e1", "e2")}))
    return base, index


def _copy_of(store_dir, to, index, names):
    shutil.copytree(store_dir / "events", to / "events")
    (to / "event_index.json").write_text(json.dumps({k: dict(index[k], file_path=str(to / "events" / "v" / f"{k}.json")) for k in names}))
    return to


def test_event_file_end_to_end(memory_store):
    from hippomm_amd import event_store as es
    base, _ = memory_store
    path = base / "events" / "v" / "e0.json"
    want, want_times = es.parse_event_features(path)
    stats = {}
    got, got_times = es.parse_event_features(path, matrices="device", stats=stats)
    assert stats == {"device": 2, "host": 0, "json": 0} and set(got) == set(want) == {"vision", "audio"}
    for modality in want:
        assert got[modality].is_cuda and got[modality].dtype == torch.float32 and tuple(got[modality].shape) == want[modality].shape
        assert got[modality].cpu().numpy().tobytes() == want[modality].tobytes(), modality
    assert set(got_times) == set(want_times) and all(np.array_equal(got_times[k], want_times[k]) for k in want_times)


def test_store_built_and_refreshed_from_device_tensors(memory_store, tmp_path):
    from hippomm_amd import event_store as es
    base, index = memory_store
    a, b = _copy_of(base, tmp_path / "a", index, ("e0", "e1", "e2")), _copy_of(base, tmp_path / "b", index, ("e0", "e1", "e2"))
    host, host_ids = es.build_event_store(a)
    dev, dev_ids = es.build_event_store(b, parse="device")
    query = np.random.default_rng(13).standard_normal(1024).astype(np.float32)

    def same():
        assert host_ids == dev_ids and host.lengths == dev.lengths and host.lengths[1] == 0
        assert torch.equal(host.offsets, dev.offsets) and torch.equal(host.rows, dev.rows)
        for (hi, hs), (di, ds) in zip(host.top_k_per_event(query, 5), dev.top_k_per_event(query, 5)):
            assert np.array_equal(hi, di) and hs.tobytes() == ds.tobytes()
        for name in host_ids:
            for modality in ("vision", "audio"):
                pa, pb = (es._sidecar_paths(d / "events" / "v" / f"{name}.json", modality)[0] for d in (a, b))
                assert pa.exists() == pb.exists() and (not pa.exists() or np.load(pa).tobytes() == np.load(pb).tobytes()), (name, modality)
            assert es._fresh_manifest(b / "events" / "v" / f"{name}.json") is not None
    same()
    for d in (a, b):
        (d / "event_index.json").write_text(json.dumps({k: dict(index[k], file_path=str(d / "events" / "v" / f"{k}.json")) for k in index}))
    host_ids = es.refresh_event_store(host, host_ids, a)
    dev_ids = es.refresh_event_store(dev, dev_ids, b, parse="device")
    assert dev_ids == ["e0", "e1", "e2", "e3"] and dev.lengths == [600, 0, 37, 5]
    same()
    # without sidecars on request, and events whose sidecars are fresh load from them
    c = _copy_of(base, tmp_path / "c", index, ("e0", "e1", "e2"))
    again, _ = es.build_event_store(c, parse="device", write_sidecar=False)
    assert torch.equal(again.rows, host.rows[:637]) and not list((c / "events" / "v").glob("*.npy"))
    warm, _ = es.build_event_store(b, parse="device")
    assert torch.equal(warm.rows, host.rows)
