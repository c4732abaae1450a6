"""CPU: the checkpoint file and its base64 core, without a GPU.

* The host route (``matrices="host"``), the streamed file and the format as tests/checkpoint_cases.py states it each equal
  tests/golden/checkpoint_golden.json, which the unmodified reference's ``_save_checkpoint`` wrote.
* The core of csrc/base64_core.h, run on the host (``hmm_base64_encode_host`` / ``hmm_base64_decode_host``), equals
  ``base64.b64encode`` at every size at which the kernels take another path, round-trips, counts inexact narrowing and refuses
  what the strict rules refuse, with the right offset and nothing written.
* The loader returns what was saved."""
import base64
import ctypes as C
import json
import logging

import numpy as np
import pytest

import checkpoint_cases as K


def _lib():
    from hippomm_amd import _lib as L
    return L.load(), L


def encode_host(a: np.ndarray, cap_extra: int = 0) -> bytes:
    lib, L = _lib()
    a = np.ascontiguousarray(a)
    dtype = {np.dtype(np.float32): K.DTYPE_F32, np.dtype(np.float64): K.DTYPE_F64, np.dtype(np.uint8): K.DTYPE_U8}[a.dtype]
    n = lib.hmm_base64_encoded_length(a.size * (1 if dtype == K.DTYPE_U8 else 8))
    buf = np.full(n + 64, 0xA5, np.uint8)
    L.check(lib.hmm_base64_encode_host(a.ctypes.data, dtype, a.size, buf.ctypes.data, n + cap_extra), "hmm_base64_encode_host")
    assert (buf[n:] == 0xA5).all()                                   # nothing behind the encoded length
    return buf[:n].tobytes()


def decode_host(text: bytes, dtype: int, cap=None):
    """-> (report words, the output buffer with its poison, the values' dtype)"""
    lib, L = _lib()
    np_dtype = {K.DTYPE_F32: np.float32, K.DTYPE_F64: np.float64, K.DTYPE_U8: np.uint8}[dtype]
    quads = len(text) // 4
    room = (quads * 3 if dtype == K.DTYPE_U8 else quads * 3 // 8) if cap is None else cap
    out = np.full((room + 8) * np.dtype(np_dtype).itemsize, 0xA5, np.uint8)
    report = np.full(K.REPORT_WORDS, 0xA5A5A5A5A5A5A5A5, np.uint64)
    L.check(lib.hmm_base64_decode_host(text, len(text), dtype, out.ctypes.data, room, report.ctypes.data), "hmm_base64_decode_host")
    return report, out, np_dtype


def test_the_host_route_the_streamed_file_and_the_stated_format_equal_the_reference_file(tmp_path):
    from hippomm_amd import checkpoint as ck
    g, text = K.golden()
    assert g["recipe"] == json.loads(json.dumps(K.RECIPE))
    assert len(text) < 100_000
    memories = K.recipe_memories()
    assert K.expected_text(g["recipe"]["video_id"], memories, g["timestamp"]) == text
    assert ck.checkpoint_bytes(g["recipe"]["video_id"], memories, g["timestamp"], matrices="host") == text
    assert ck.checkpoint_bytes(g["recipe"]["video_id"], [vars(m) | {"segment_info": vars(m.segment_info)} for m in memories],
                               g["timestamp"]) == text               # mappings as well as objects
    clock = iter([1234.9, g["timestamp"]])
    path = ck.save_checkpoint(tmp_path, g["recipe"]["video_id"], memories, now=lambda: next(clock))
    assert path == str(tmp_path / "checkpoints" / g["file_name_pattern"].replace("{int(now)}", "1234"))
    assert open(path, "rb").read() == text


def test_drop_ins_write_the_same_serialisation(tmp_path):
    import types
    from hippomm_amd import checkpoint as ck
    g, text = K.golden()
    owner = types.SimpleNamespace(storage_dir=tmp_path, checkpoint_matrices="host", short_term_buffer={"v1": K.recipe_memories()})
    path = ck._save_checkpoint(owner, g["recipe"]["video_id"], K.recipe_memories())
    body = json.loads(open(path).read())
    assert body["memories"] == json.loads(text)["memories"] and body["video_id"] == g["recipe"]["video_id"]
    paths = ck.save_short_term_buffer(owner)
    assert list(paths) == ["v1"] and paths["v1"].startswith(str(tmp_path / "temp_short_term" / "short_term_v1_"))
    assert json.loads(open(paths["v1"]).read())["memories"] == body["memories"]
    loaded = ck._load_checkpoint(owner, path)
    assert len(loaded) == 2
    assert ck._load_checkpoint(owner, str(tmp_path / "missing.json")) is None


@pytest.mark.parametrize("n", K.byte_lengths())
def test_core_encodes_bytes_as_python_does(n):
    a = K.sample(np.uint8, n)
    assert encode_host(a) == base64.b64encode(a.tobytes())
    assert _lib()[0].hmm_base64_encoded_length(n) == len(base64.b64encode(a.tobytes()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", K.value_counts())
def test_core_encodes_floats_as_the_reference_expression_does(n, dtype):
    a = K.sample(dtype, n)
    assert encode_host(a) == base64.b64encode(np.array(a.tolist()).tobytes())


def test_core_passes_special_values_bit_for_bit():
    for a in (K.special_doubles(), K.special_floats()):
        with np.errstate(all="ignore"):
            want = a.astype(np.float64)
        assert encode_host(a) == base64.b64encode(want.tobytes())
        report, out, _ = decode_host(encode_host(a), K.DTYPE_F64)
        assert report[0] == K.OK and report[3] == a.size
        assert (out[:8 * a.size].view(np.uint64) == want.view(np.uint64)).all()


@pytest.mark.parametrize("n", K.byte_lengths())
def test_core_decode_round_trips_bytes(n):
    a = K.sample(np.uint8, n)
    report, out, _ = decode_host(base64.b64encode(a.tobytes()), K.DTYPE_U8)
    assert list(report[:4]) == [K.OK, 0, 0, n]
    assert out[:n].tobytes() == a.tobytes() and (out[n:] == 0xA5).all()


@pytest.mark.parametrize("n", K.value_counts())
def test_core_decode_round_trips_floats_and_counts_inexact_narrowing(n):
    f32 = K.sample(np.float32, n)
    text = K.python_base64(f32)
    report, out, _ = decode_host(text, K.DTYPE_F64)
    assert list(report[:4]) == [K.OK, 0, 0, n]
    assert (out[:8 * n].view(np.float64) == f32.astype(np.float64)).all() and (out[8 * n:] == 0xA5).all()
    report, out, _ = decode_host(text, K.DTYPE_F32)                  # widened fp32 narrows exactly
    assert list(report[:4]) == [K.OK, 0, 0, n]
    assert (out[:4 * n].view(np.uint32) == f32.view(np.uint32)).all() and (out[4 * n:] == 0xA5).all()
    f64 = K.sample(np.float64, n)                                    # random doubles need more bits
    f64[::2] = f32[::2]                                              # ... except these
    report, out, _ = decode_host(K.python_base64(f64), K.DTYPE_F32)
    assert list(report[:4]) == [K.OK, 0, n // 2, n]
    assert (out[:4 * n].view(np.float32) == f64.astype(np.float32)).all()


def test_narrowing_of_special_doubles_counts_only_what_does_not_widen_back():
    d = K.special_doubles()
    report, out, _ = decode_host(K.python_base64(d), K.DTYPE_F32)
    with np.errstate(all="ignore"):
        f = d.astype(np.float32)
        inexact = int((f.astype(np.float64).view(np.uint64) != d.view(np.uint64)).sum())
    assert inexact > 0 and report[2] == inexact
    ok = ~np.isnan(d)
    assert (out[:4 * d.size].view(np.uint32)[ok] == f.view(np.uint32)[ok]).all()


@pytest.mark.parametrize("dtype", [K.DTYPE_U8, K.DTYPE_F64, K.DTYPE_F32], ids=["u8", "f64", "f32"])
@pytest.mark.parametrize("case", K.refusals(), ids=lambda c: c[0].replace(" ", "_"))
def test_core_refuses_what_the_strict_rules_refuse_and_writes_nothing(case, dtype):
    _, text, status, offset = case
    report, out, _ = decode_host(text, dtype, cap=64)
    assert (int(report[0]), int(report[1])) == (status, offset)
    assert report[2] == 0 and report[3] == 0
    assert (out == 0xA5).all()


def test_float_output_needs_whole_doubles_and_byte_output_needs_room():
    text = base64.b64encode(bytes(range(20)))                        # 20 bytes: two and a half doubles
    report, out, _ = decode_host(text, K.DTYPE_F64, cap=8)
    assert (int(report[0]), int(report[1])) == (K.PARTIAL_VALUE, len(text) - 4) and (out == 0xA5).all()
    text = base64.b64encode(bytes(range(30)))                        # no padding: 30 bytes, the least accepted cap is 28
    report, out, _ = decode_host(text, K.DTYPE_U8, cap=28)
    assert (int(report[0]), int(report[1])) == (K.CAPACITY, len(text) - 4) and (out == 0xA5).all()


def test_python_lenient_decoder_accepts_what_the_core_refuses():
    """Why the caller falls back to base64.b64decode on a refusal: Python skips the newline."""
    _, text, status, _ = next(c for c in K.refusals() if c[0] == "embedded newline")
    assert status == K.BAD_CHAR and base64.b64decode(text) == bytes(range(30))


def test_argument_errors_of_the_new_exports_are_reported_without_a_gpu():
    lib, L = _lib()
    buf = np.zeros(256, np.uint8)
    report = np.zeros(K.REPORT_WORDS, np.uint64)
    r = report.ctypes.data
    base = (buf.ctypes.data + 15) // 16 * 16                         # a 16-byte aligned address inside buf
    for fn, tag in ((lib.hmm_base64_encode_host, b"base64_encode_host"), (lambda *a: lib.hmm_base64_encode_device(*a, None), b"base64_encode_device")):
        assert fn(None, K.DTYPE_U8, 3, base, 4) == -1 and b"null pointer" in lib.hmm_last_error() and tag in lib.hmm_last_error()
        assert fn(base, K.DTYPE_U8, 3, None, 4) == -1
        assert fn(base, K.DTYPE_U8, 4, base + 16, 7) == -1 and b"need 8" in lib.hmm_last_error()
        assert fn(base, 3, 1, base + 16, 16) == -1 and b"dtype" in lib.hmm_last_error()
        assert fn(base + 4, K.DTYPE_F64, 1, base + 16, 16) == -1 and b"aligned" in lib.hmm_last_error()
        assert fn(base + 2, K.DTYPE_F32, 1, base + 16, 16) == -1 and b"aligned" in lib.hmm_last_error()
        assert fn(base, K.DTYPE_F64, 1 << 40, base + 16, 16) == -1
    assert lib.hmm_base64_encode_device(base, K.DTYPE_U8, 3, base + 17, 4, None) == -1 and b"16-byte" in lib.hmm_last_error()
    for fn, tag in ((lib.hmm_base64_decode_host, b"base64_decode_host"), (lambda *a: lib.hmm_base64_decode_device(*a, None), b"base64_decode_device")):
        assert fn(None, 4, K.DTYPE_U8, base + 16, 3, r) == -1 and tag in lib.hmm_last_error()
        assert fn(base, 4, K.DTYPE_U8, None, 3, r) == -1
        assert fn(base, 4, K.DTYPE_U8, base + 16, 3, None) == -1 and b"report" in lib.hmm_last_error()
        assert fn(base, 8, K.DTYPE_U8, base + 16, 3, r) == -1 and b"need 4" in lib.hmm_last_error()
        assert fn(base, 32, K.DTYPE_F64, base + 16, 2, r) == -1 and b"need 3" in lib.hmm_last_error()
        assert fn(base, 4, 7, base + 16, 3, r) == -1 and b"dtype" in lib.hmm_last_error()
        assert fn(base, 32, K.DTYPE_F64, base + 20, 3, r) == -1 and b"aligned" in lib.hmm_last_error()
        assert fn(base, 4, K.DTYPE_U8, base + 16, 3, r + 4) == -1 and b"aligned" in lib.hmm_last_error()
    assert lib.hmm_base64_decode_device(base + 4, 4, K.DTYPE_U8, base + 16, 3, r, None) == -1 and b"16-byte" in lib.hmm_last_error()
    assert (buf == 0).all() and (report == 0).all()


# ---- the loader ----
def _assert_recipe(memories, saved):
    assert len(memories) == len(saved)
    for got, want in zip(memories, saved):
        assert list(got.features) == list(want.features)
        for k, v in want.features.items():
            f = got.features[k]
            f = f.cpu().numpy() if hasattr(f, "cpu") else f
            assert f.dtype == np.float32 and f.shape == v.shape
            assert (f.view(np.uint32) == v.view(np.uint32)).all()
        assert got.segment_info.audio_data is None
        assert got.segment_info.start_time == want.segment_info.start_time and got.segment_info.end_time == want.segment_info.end_time
        assert got.segment_info.frames == want.segment_info.frames and got.segment_info.frame_times == want.segment_info.frame_times
        assert got.content == dict(want.content, audio=dict(want.content["audio"], data=want.content["audio"]["data"].tolist()))
        assert (got.timestamp, got.source_time, got.modalities, got.transcription) == (want.timestamp, want.source_time, want.modalities,
                                                                                       want.transcription)


def test_loader_returns_what_the_reference_file_holds(tmp_path):
    from hippomm_amd import checkpoint as ck
    _, text = K.golden()
    path = tmp_path / "golden.json"
    path.write_bytes(text)
    memories = ck.load_checkpoint(path)
    assert all(isinstance(m, ck.ShortTermMemory) and isinstance(m.segment_info, ck.SequenceSegment) for m in memories)
    _assert_recipe(memories, K.recipe_memories())


def test_loader_never_parses_the_waveforms(tmp_path, monkeypatch):
    """The text json.loads sees holds no waveform: it is shorter than the file by about the waveforms' text."""
    from hippomm_amd import checkpoint as ck
    _, text = K.golden()
    path = tmp_path / "golden.json"
    path.write_bytes(text)
    seen = []
    real = json.loads
    monkeypatch.setattr(ck.json, "loads", lambda s, *a, **k: (seen.append(len(s)), real(s, *a, **k))[1])
    ck.load_checkpoint(path)
    waveforms = sum(len(json.dumps(m.segment_info.audio_data.tolist(), indent=2)) for m in K.recipe_memories())
    assert len(seen) == 1 and seen[0] < len(text) - waveforms


def test_loader_on_null_waveforms_odd_counts_and_inexact_blocks(tmp_path):
    from hippomm_amd import checkpoint as ck
    memories = K.recipe_memories()
    for m in memories:
        m.segment_info.audio_data = None
    rng = np.random.default_rng(3)
    odd, wide = rng.standard_normal(1000).astype(np.float32), rng.standard_normal((2, 1024))
    memories[0].features = {"vision": memories[0].features["vision"], "odd": odd, "wide": wide}
    body = json.loads(K.expected_text("v", memories, 5.0))
    for m in body["memories"]:
        m["segment_info"]["audio_data"] = None                       # a file whose waveforms were already null
    path = tmp_path / "c.json"
    path.write_text(json.dumps(body, indent=2))
    got = ck.load_checkpoint(path)
    assert got[0].segment_info.audio_data is None and got[1].segment_info.audio_data is None
    f = got[0].features
    assert f["vision"].dtype == np.float32 and f["vision"].shape == (2, 1024)
    assert f["odd"].dtype == np.float64 and f["odd"].shape == (1000,) and (f["odd"] == odd.astype(np.float64)).all()
    assert f["wide"].dtype == np.float64 and f["wide"].shape == (2, 1024) and (f["wide"].view(np.uint64) == wide.view(np.uint64)).all()


def test_save_then_load_round_trips(tmp_path):
    from hippomm_amd import checkpoint as ck
    saved = K.recipe_memories()
    path = ck.save_checkpoint(tmp_path, "v", saved)
    assert path is not None
    _assert_recipe(ck.load_checkpoint(path), saved)


def test_an_unwritable_directory_gives_none_and_a_log_line(tmp_path, caplog):
    from hippomm_amd import checkpoint as ck
    blocker = tmp_path / "storage"
    blocker.write_text("a file where the directory should be")
    with caplog.at_level(logging.ERROR, logger="hippomm_amd.checkpoint"):
        assert ck.save_checkpoint(blocker, "v", K.recipe_memories()) is None
    assert any("Error saving checkpoint" in r.getMessage() for r in caplog.records)


def test_bad_route_names_are_refused():
    from hippomm_amd import checkpoint as ck
    with pytest.raises(ValueError, match="matrices"):
        ck.checkpoint_bytes("v", [], 0.0, matrices="gpu")
    with pytest.raises(ValueError, match="features"):
        ck.load_checkpoint("nowhere.json", features="gpu")
