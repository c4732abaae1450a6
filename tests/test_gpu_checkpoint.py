"""GPU: the base64 kernels against Python, their memory contract in the guarded arena (tests/arena.py), the waveform text the
checkpoint depends on, and whole checkpoint files on the device route against the reference's file
(tests/golden/checkpoint_golden.json) and against the format as tests/checkpoint_cases.py states it."""
import base64
import json

import numpy as np
import pytest
import torch

import arena as A
import checkpoint_cases as K

pytestmark = pytest.mark.gpu

POISON = 0xA5
TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8}
CODE_OF = {np.dtype(np.float32): K.DTYPE_F32, np.dtype(np.float64): K.DTYPE_F64, np.dtype(np.uint8): K.DTYPE_U8}


def _lib():
    from hippomm_amd import _lib as L
    return L.load(), L, L.require_gpu()


def encode_dev(t: torch.Tensor) -> bytes:
    """A contiguous CUDA tensor through hmm_base64_encode_device; also checks that nothing behind the encoded length is written."""
    lib, L, dev = _lib()
    code = {torch.float32: K.DTYPE_F32, torch.float64: K.DTYPE_F64, torch.uint8: K.DTYPE_U8}[t.dtype]
    n = lib.hmm_base64_encoded_length(t.numel() * (1 if code == K.DTYPE_U8 else 8))
    out = torch.full((n + 256,), POISON, dtype=torch.uint8, device=dev)
    before = t.clone()
    L.check(lib.hmm_base64_encode_device(t.data_ptr() if t.numel() else None, code, t.numel(), out.data_ptr(), n, L.stream_ptr()),
            "hmm_base64_encode_device")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == POISON).all()
    assert torch.equal(t.view(torch.uint8), before.view(torch.uint8))
    return got[:n].tobytes()


def decode_dev(text: bytes, code: int, cap=None):
    """-> (report words, the whole poisoned output buffer as bytes)"""
    lib, L, dev = _lib()
    elem = {K.DTYPE_F32: 4, K.DTYPE_F64: 8, K.DTYPE_U8: 1}[code]
    quads = len(text) // 4
    room = (quads * 3 if code == K.DTYPE_U8 else quads * 3 // 8) if cap is None else cap
    t = torch.from_numpy(np.frombuffer(text + b"\0", np.uint8).copy()).to(dev)           # the byte behind the text is not part of it
    out = torch.full(((room + 8) * elem,), POISON, dtype=torch.uint8, device=dev)
    report = torch.full((K.REPORT_WORDS,), -1, dtype=torch.int64, device=dev)
    L.check(lib.hmm_base64_decode_device(t.data_ptr(), len(text), code, out.data_ptr(), room, report.data_ptr(), L.stream_ptr()),
            "hmm_base64_decode_device")
    torch.cuda.synchronize()
    assert t[:len(text)].cpu().numpy().tobytes() == text
    return report.cpu().numpy().view(np.uint64), out.cpu().numpy()


# ---- encode ----
def test_encode_kernel_writes_pythons_bytes_for_every_byte_length():
    dev = _lib()[2]
    for n in sorted(set(K.byte_lengths()) | set(range(10))):
        a = K.sample(np.uint8, n)
        assert encode_dev(torch.from_numpy(a).to(dev)) == base64.b64encode(a.tobytes()), n


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_encode_kernel_writes_the_reference_expression_for_floats(dtype):
    dev = _lib()[2]
    for n in K.value_counts():
        a = K.sample(dtype, n)
        assert encode_dev(torch.from_numpy(a).to(dev)) == base64.b64encode(np.array(a.tolist()).tobytes()), n
    for shape in ((2, 1024), (30, 1024)):
        a = K.sample(dtype, shape[0] * shape[1]).reshape(shape)
        assert encode_dev(torch.from_numpy(a).to(dev)) == base64.b64encode(np.array(a.tolist()).tobytes()), shape
    big = torch.from_numpy(K.sample(dtype, 9 * 1024).reshape(9, 1024)).to(dev)
    rows = big[3:8]                                                   # a row slice of a larger tensor: read where it lies
    assert rows.data_ptr() != big.data_ptr() and rows.is_contiguous()
    assert encode_dev(rows) == base64.b64encode(np.array(rows.cpu().numpy().tolist()).tobytes())
    special = K.special_floats() if dtype == np.float32 else K.special_doubles()
    with np.errstate(all="ignore"):
        want = special.astype(np.float64)
    assert encode_dev(torch.from_numpy(special).to(dev)) == base64.b64encode(want.tobytes())


def test_features_base64_takes_arrays_tensors_and_anything_else():
    from hippomm_amd import checkpoint as ck
    dev = _lib()[2]
    a = K.sample(np.float32, 5 * 1024).reshape(5, 1024)
    want = base64.b64encode(np.array(a.tolist()).tobytes())
    stats = {}
    assert ck.features_base64(a, stats=stats) == want and stats["route"] == "device"
    assert ck.features_base64(torch.from_numpy(a).to(dev), stats=stats) == want and stats["route"] == "device"
    assert ck.features_base64(torch.from_numpy(a).to(dev).t().contiguous().t(), stats=stats) == want            # not contiguous
    assert ck.features_base64(a.astype(np.float64)[1:3], stats=stats) == base64.b64encode(a[1:3].astype(np.float64).tobytes())
    assert ck.features_base64(a[0].tolist(), stats=stats) == base64.b64encode(np.array(a[0].tolist()).tobytes()) and stats["route"] == "host"
    assert ck.features_base64(np.arange(6, dtype=np.int32), stats=stats) == base64.b64encode(np.arange(6).tobytes()) and stats["route"] == "host"


# ---- decode ----
def test_decode_kernel_round_trips_bytes():
    for n in sorted(set(K.byte_lengths())):
        a = K.sample(np.uint8, n)
        report, out = decode_dev(base64.b64encode(a.tobytes()), K.DTYPE_U8)
        assert list(report[:4]) == [K.OK, 0, 0, n], n
        assert out[:n].tobytes() == a.tobytes() and (out[n:] == POISON).all(), n


def test_decode_kernel_round_trips_floats_and_counts_inexact_narrowing():
    for n in K.value_counts() + [2 * 1024, 30 * 1024]:
        f32 = K.sample(np.float32, n)
        text = K.python_base64(f32)
        report, out = decode_dev(text, K.DTYPE_F64)
        assert list(report[:4]) == [K.OK, 0, 0, n], n
        assert (out[:8 * n].view(np.uint64) == f32.astype(np.float64).view(np.uint64)).all() and (out[8 * n:] == POISON).all(), n
        report, out = decode_dev(text, K.DTYPE_F32)
        assert list(report[:4]) == [K.OK, 0, 0, n], n
        assert (out[:4 * n].view(np.uint32) == f32.view(np.uint32)).all() and (out[4 * n:] == POISON).all(), n
        f64 = K.sample(np.float64, n)
        f64[::2] = f32[::2]
        report, out = decode_dev(K.python_base64(f64), K.DTYPE_F32)
        assert list(report[:4]) == [K.OK, 0, n // 2, n], n
        assert (out[:4 * n].view(np.float32) == f64.astype(np.float32)).all(), n
    d = K.special_doubles()
    report, out = decode_dev(K.python_base64(d), K.DTYPE_F64)
    assert (out[:8 * d.size].view(np.uint64) == d.view(np.uint64)).all()
    report, out = decode_dev(K.python_base64(d), K.DTYPE_F32)
    with np.errstate(all="ignore"):
        f = d.astype(np.float32)
        inexact = int((f.astype(np.float64).view(np.uint64) != d.view(np.uint64)).sum())
    assert report[2] == inexact
    ok = ~np.isnan(d)
    assert (out[:4 * d.size].view(np.uint32)[ok] == f.view(np.uint32)[ok]).all()


@pytest.mark.parametrize("code", [K.DTYPE_U8, K.DTYPE_F64, K.DTYPE_F32], ids=["u8", "f64", "f32"])
def test_decode_kernel_refuses_what_the_strict_rules_refuse_and_writes_nothing(code):
    cases = K.refusals()
    long = base64.b64encode(K.sample(np.uint8, 3 * K.BYTES_PER_GROUP).tobytes())          # the offence in another workgroup than the end
    at = len(long) // 2 + 1
    cases += [("bad character far from the end", long[:at] + b"\n" + long[at + 1:], K.BAD_CHAR, at),
              ("two offences in two workgroups", long[:at] + b"=" + long[at + 1:-1] + b"*", K.BAD_PADDING, at)]
    for name, text, status, offset in cases:
        report, out = decode_dev(text, code, cap=len(text))
        assert (int(report[0]), int(report[1])) == (status, offset), name
        assert report[2] == 0 and report[3] == 0, name
        assert (out == POISON).all(), name
    report, out = decode_dev(base64.b64encode(bytes(range(20))), K.DTYPE_F64, cap=8)
    assert (int(report[0]), int(report[1])) == (K.PARTIAL_VALUE, 24) and (out == POISON).all()
    report, out = decode_dev(base64.b64encode(bytes(range(30))), K.DTYPE_U8, cap=28)
    assert (int(report[0]), int(report[1])) == (K.CAPACITY, 36) and (out == POISON).all()


# ---- the memory contract ----
CONTRACT = [(np.uint8, 0), (np.uint8, 1), (np.uint8, K.BYTES_PER_GROUP + 25), (np.float32, K.BYTES_PER_GROUP // 8 + 1),
            (np.float64, K.BYTES_PER_GROUP // 8 + 2), (np.float32, 2 * 1024)]


@pytest.mark.parametrize("case", CONTRACT, ids=lambda c: f"{np.dtype(c[0]).name}-{c[1]}")
def test_encode_owns_its_text_and_nothing_else(case):
    dtype, n = case
    lib, L, dev = _lib()
    a = K.sample(dtype, n)
    want = base64.b64encode(a.tobytes() if dtype == np.uint8 else a.astype(np.float64).tobytes())
    assert lib.hmm_base64_encoded_length(a.size * (1 if dtype == np.uint8 else 8)) == len(want)
    for pattern in ("ones", "big"):
        ar = A.GuardedArena(A.needed_bytes([a.nbytes, len(want)]), dev, A.PATTERNS[pattern])
        src = ar.put(torch.from_numpy(a), "source", align=16)
        out = ar.carve(len(want), "text", align=16)                  # exactly the encoded length
        assert lib.hmm_base64_encode_device(ar.address(src), CODE_OF[np.dtype(dtype)], n, ar.address(out), len(want), L.stream_ptr()) == 0
        torch.cuda.synchronize()
        ar.check_guards()
        assert src.cpu().numpy().tobytes() == a.tobytes(), pattern
        assert out.cpu().numpy().tobytes() == want, pattern


@pytest.mark.parametrize("case", CONTRACT, ids=lambda c: f"{np.dtype(c[0]).name}-{c[1]}")
def test_decode_owns_its_values_and_the_report_and_nothing_else(case):
    dtype, n = case
    lib, L, dev = _lib()
    a = K.sample(dtype, n)
    text = K.python_base64(a)
    for pattern in ("ones", "big"):
        ar = A.GuardedArena(A.needed_bytes([len(text), a.nbytes, 8 * K.REPORT_WORDS]), dev, A.PATTERNS[pattern])
        src = ar.put(torch.from_numpy(np.frombuffer(text, np.uint8).copy()), "text", align=16)
        out = ar.carve(a.nbytes, "values", align=16)                 # exactly n values
        report = ar.carve(8 * K.REPORT_WORDS, "report", align=8)
        assert lib.hmm_base64_decode_device(ar.address(src), len(text), CODE_OF[np.dtype(dtype)], ar.address(out), n, ar.address(report),
                                            L.stream_ptr()) == 0, L.load().hmm_last_error()
        torch.cuda.synchronize()
        ar.check_guards()
        assert src.cpu().numpy().tobytes() == text, pattern
        assert list(report.cpu().numpy().view(np.uint64)[:4]) == [K.OK, 0, 0, n], pattern
        assert out.cpu().numpy().tobytes() == a.tobytes(), pattern


def test_a_refused_text_leaves_the_values_poisoned_in_the_arena():
    lib, L, dev = _lib()
    text = bytearray(K.python_base64(K.sample(np.float32, 1024)))
    text[4097] = ord(" ")
    for pattern in ("ones", "big"):
        ar = A.GuardedArena(A.needed_bytes([len(text), 4 * 1024, 8 * K.REPORT_WORDS]), dev, A.PATTERNS[pattern])
        src = ar.put(torch.from_numpy(np.frombuffer(bytes(text), np.uint8).copy()), "text", align=16)
        out = ar.carve(4 * 1024, "values", align=16)
        report = ar.carve(8 * K.REPORT_WORDS, "report", align=8)
        assert lib.hmm_base64_decode_device(ar.address(src), len(text), K.DTYPE_F32, ar.address(out), 1024, ar.address(report), L.stream_ptr()) == 0
        torch.cuda.synchronize()
        ar.check_guards()
        assert ar.is_pattern(out), pattern
        assert list(report.cpu().numpy().view(np.uint64)[:4]) == [K.BAD_CHAR, 4097, 0, 0], pattern


# ---- the waveform's text ----
def _waveform_text(a: np.ndarray) -> bytes:
    return json.dumps(a.tolist(), indent=2).replace("\n", "\n" + " " * 8).encode("ascii")


@pytest.mark.parametrize("shape,dtype", [((1, 1), np.float64), ((2, 1), np.float64), ((1023, 1), np.float64), ((1024, 1), np.float64),
                                         ((1025, 1), np.float64), ((262145, 1), np.float64), ((7, 2), np.float64), ((1025, 1), np.float32)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name)
def test_waveform_text_at_the_checkpoints_indentation(shape, dtype):
    """These may pass on the matrix writer as it stood before the checkpoint route existed: they pin the shape that route depends
    on -- one value per row, the closing bracket at 8 spaces, 262145 rows crossing HMM_JSON_VALUES_PER_SCAN_ROUND."""
    from hippomm_amd import event_store
    a = np.random.default_rng(shape[0]).uniform(-1, 1, size=shape).astype(dtype)
    a.reshape(-1)[:4] = np.array([1e-5, -0.0, 0.0, 1.0], dtype)[:a.size]
    assert event_store.matrix_json_bytes(a, close_indent=8) == _waveform_text(a)


# ---- whole files ----
def _device_text(memories, timestamp, **kw):
    from hippomm_amd import checkpoint as ck
    stats = {}
    text = ck.checkpoint_bytes(K.RECIPE["video_id"], memories, timestamp, matrices="device", stats=stats, **kw)
    return text, stats


def test_the_device_route_writes_the_reference_file(tmp_path):
    from hippomm_amd import checkpoint as ck
    g, text = K.golden()
    got, stats = _device_text(K.recipe_memories(), g["timestamp"])
    assert got == text
    assert stats == {"features_device": 4, "features_host": 0, "waveform_resident": 0, "waveform_upload": 2, "waveform_host": 0}
    clock = iter([77.5, g["timestamp"]])
    path = ck.save_checkpoint(tmp_path, K.RECIPE["video_id"], K.recipe_memories(), matrices="device", now=lambda: next(clock))
    assert path.endswith("_77.json") and open(path, "rb").read() == text


def test_the_device_route_on_other_shapes_of_memory():
    dev = _lib()[2]
    vision_only, audio_only, no_waveform, tensors, mono = K.recipe_memories() + K.recipe_memories() + K.recipe_memories()[:1]
    del vision_only.features["audio"]
    vision_only.modalities = ["vision"]
    del audio_only.features["vision"]
    audio_only.segment_info.frames = audio_only.segment_info.frame_times = None
    no_waveform.segment_info.audio_data = None
    tensors.features = {k: torch.from_numpy(v).to(dev) for k, v in tensors.features.items()}
    tensors.segment_info.audio_data = torch.from_numpy(tensors.segment_info.audio_data.astype(np.float32)).to(dev)
    mono.segment_info.audio_data = mono.segment_info.audio_data[:, 0].copy()              # 1-D: json's own text
    mono.features["listed"] = mono.features["audio"][0, :8].tolist()                      # not an array: the host expression
    memories = [vision_only, audio_only, no_waveform, tensors, mono]
    got, stats = _device_text(memories, 12.5)
    assert got == K.expected_text(K.RECIPE["video_id"], memories, 12.5)
    assert stats == {"features_device": 8, "features_host": 1, "waveform_resident": 0, "waveform_upload": 3, "waveform_host": 0}
    from hippomm_amd import checkpoint as ck
    assert got == ck.checkpoint_bytes(K.RECIPE["video_id"], memories, 12.5, matrices="host")


def test_a_token_in_the_memories_own_strings_sends_the_file_through_the_host(monkeypatch):
    from hippomm_amd import checkpoint as ck
    g, text = K.golden()

    class Salt:
        hex = "feedbeef"
    monkeypatch.setattr(ck.uuid, "uuid4", lambda: Salt)
    memories = K.recipe_memories()
    memories[1].transcription[0]["text"] = "@@hmm_ckpt_0_0_feedbeef@@"
    got, _ = _device_text(memories, 3.0)
    assert got == K.expected_text(K.RECIPE["video_id"], memories, 3.0)


def test_the_resident_track_writes_the_same_file_without_an_upload():
    from hippomm_amd.audio_track import AudioTrack
    g, text = K.golden()
    track = K.recipe_track()
    spans = [tuple(s) for s in K.RECIPE["spans"]]
    got, stats = _device_text(K.recipe_memories(), g["timestamp"], audio_track=AudioTrack(track, 16000), audio_spans=spans)
    assert got == text and (stats["waveform_resident"], stats["waveform_upload"], stats["waveform_host"]) == (2, 0, 0)
    got, stats = _device_text(K.recipe_memories(), g["timestamp"], audio_track=AudioTrack(track[:, 0].copy(), 16000), audio_spans=[spans[0], None])
    assert got == text and (stats["waveform_resident"], stats["waveform_upload"]) == (1, 1)
    stereo = AudioTrack(np.concatenate([track, track], axis=1), 16000)                    # a mixed-down track is not the memory's array
    got, stats = _device_text(K.recipe_memories(), g["timestamp"], audio_track=stereo, audio_spans=spans)
    assert got == text and (stats["waveform_resident"], stats["waveform_upload"]) == (0, 2)
    narrow = AudioTrack(track.astype(np.float32), 16000)                                  # another dtype than the memory's array
    got, stats = _device_text(K.recipe_memories(), g["timestamp"], audio_track=narrow, audio_spans=spans)
    assert got == text and (stats["waveform_resident"], stats["waveform_upload"]) == (0, 2)


def test_the_loader_returns_device_tensors_with_the_saved_bits(tmp_path):
    from hippomm_amd import checkpoint as ck
    saved = K.recipe_memories()
    odd = np.random.default_rng(4).standard_normal(1000).astype(np.float32)
    wide = np.random.default_rng(5).standard_normal((1, 1024))
    saved[1].features.update(odd=odd, wide=wide)
    path = ck.save_checkpoint(tmp_path, "v", saved, matrices="device")
    got = ck.load_checkpoint(path, features="device")
    for m, want in zip(got, saved):
        assert m.segment_info.audio_data is None
        for k in ("vision", "audio"):
            f = m.features[k]
            assert isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == want.features[k].shape
            assert (f.cpu().numpy().view(np.uint32) == want.features[k].view(np.uint32)).all()
    assert got[1].features["odd"].dtype == np.float64 and (got[1].features["odd"] == odd.astype(np.float64)).all()
    assert got[1].features["wide"].dtype == np.float64 and (got[1].features["wide"].view(np.uint64) == wide.view(np.uint64)).all()
