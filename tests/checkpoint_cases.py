"""Checkpoint cases shared by tests/test_cpu_checkpoint.py, tests/test_gpu_checkpoint.py and the fixture's generator
(tests/golden/make_checkpoint_golden.py): the recipe of tests/golden/checkpoint_golden.json, the file format stated in this
project's own words, a Python model of the strict base64 rules, and the sizes at which the codec is compared with Python."""
from __future__ import annotations

import base64
import json
import types
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "checkpoint_golden.json"

RECIPE = {"seed": 20261020, "video_id": "video_0007", "frames": [2, 3], "track_samples": 96, "spans": [[8, 48], [60, 84]],
          "planted": {"9": 1e-5, "10": -0.0, "11": 0.0, "12": 1.0, "61": -1.0, "62": 5e-324},
          "transcriptions": ["café au lait — 你好", "plain"], "times": [[0.0, 2.5], [2.5, 4.0]]}

# per-thread and per-workgroup units of the kernels (include/hippomm_hip.h)
BYTES_PER_THREAD, BYTES_PER_GROUP = 24, 24 * 256
DTYPE_F32, DTYPE_F64, DTYPE_U8 = 0, 1, 2
OK, BAD_LENGTH, BAD_CHAR, BAD_PADDING, NONCANONICAL, PARTIAL_VALUE, CAPACITY = range(7)
REPORT_WORDS = 5


def recipe_track(recipe=RECIPE) -> np.ndarray:
    rng = np.random.default_rng(recipe["seed"])
    track = rng.uniform(-1.0, 1.0, size=(recipe["track_samples"], 1))
    for at, v in recipe["planted"].items():
        track[int(at), 0] = v
    return track


def recipe_memories(recipe=RECIPE, memory=None, segment=None, track=None):
    """The recipe's memories.  memory / segment: constructors taking the reference's field names as keywords (default: plain
    namespaces).  Features are fp32; the waveforms are float64 (n, 1) slices of one track."""
    memory = memory or (lambda **k: types.SimpleNamespace(**k))
    segment = segment or (lambda **k: types.SimpleNamespace(**k))
    rng = np.random.default_rng(recipe["seed"] + 1)
    track = recipe_track(recipe) if track is None else track
    out = []
    for i, nf in enumerate(recipe["frames"]):
        t0, t1 = recipe["times"][i]
        a, b = recipe["spans"][i]
        frames = [f"frames/{recipe['video_id']}/{i:02d}_{j:03d}.jpg" for j in range(nf)]
        out.append(memory(
            features={"vision": rng.standard_normal((nf, 1024)).astype(np.float32), "audio": rng.standard_normal((1, 1024)).astype(np.float32)},
            content={"frames": frames, "audio": {"path": f"seg_{i}.wav", "data": np.array([0.5, -0.25 * (i + 1)])}},
            timestamp=1700000000.25 + i, source_time=t0, modalities=["vision", "audio"],
            segment_info=segment(start_time=t0, end_time=t1, frames=frames, audio_data=track[a:b].copy(),
                                 frame_times=[t0 + 0.5 * j for j in range(nf)]),
            transcription=[{"start": t0, "end": t1, "text": recipe["transcriptions"][i]}]))
    return out


def _get(obj, key):
    return obj[key] if isinstance(obj, dict) else getattr(obj, key)


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def block_base64(a) -> str:
    """A feature block in the file: its values as float64 in row-major order, little endian, base64 with '=' padding."""
    return base64.b64encode(host(a).astype(np.float64).tobytes()).decode("ascii")


def expected_text(video_id, memories, timestamp) -> bytes:
    """The checkpoint format in this project's words: per memory the keys features, content, timestamp, source_time, modalities,
    segment_info, transcription; features as base64 strings; content['audio']['data'] and segment_info['audio_data'] (present only
    when there is a waveform, after start_time, end_time, frames, frame_times) as nested lists; the whole as JSON indented by 2."""
    mems = []
    for m in memories:
        content = {k: (dict(v, data=host(v["data"]).tolist()) if k == "audio" and isinstance(v, dict) and "data" in v else v)
                   for k, v in _get(m, "content").items()}
        s = _get(m, "segment_info")
        seg = {k: _get(s, k) for k in ("start_time", "end_time", "frames", "frame_times")}
        if _get(s, "audio_data") is not None:
            seg["audio_data"] = host(_get(s, "audio_data")).tolist()
        mems.append({"features": {k: block_base64(v) for k, v in _get(m, "features").items()}, "content": content,
                     "timestamp": _get(m, "timestamp"), "source_time": _get(m, "source_time"), "modalities": _get(m, "modalities"),
                     "segment_info": seg, "transcription": _get(m, "transcription")})
    return json.dumps({"video_id": video_id, "memories": mems, "timestamp": timestamp}, indent=2).encode("ascii")


def golden():
    g = json.loads(GOLDEN.read_text())
    return g, g["text"].encode("ascii")


# ---- the codec against Python ----
def special_doubles() -> np.ndarray:
    bits = [0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF,
            0x7FF8000000000000, 0xFFF8000000000001, 0x7FFC0000DEADBEEF, 0x7FEFFFFFFFFFFFFF, 0x3FB999999999999A]
    return np.array(bits, dtype=np.uint64).view(np.float64)


def special_floats() -> np.ndarray:
    bits = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FC00000, 0xFFC00001, 0x7FE0BEEF, 0x7F7FFFFF, 0x3DCCCCCD]
    return np.array(bits, dtype=np.uint32).view(np.float32)           # every NaN here is quiet


def boundary_counts(unit_values: int, group_values: int):
    return sorted({n for u in (unit_values, group_values) for n in (u - 1, u, u + 1)})


def byte_lengths():
    return list(range(0, 51)) + boundary_counts(BYTES_PER_THREAD, BYTES_PER_GROUP)


def value_counts():
    return list(range(1, 8)) + boundary_counts(BYTES_PER_THREAD // 8, BYTES_PER_GROUP // 8)


def sample(dtype, n: int, seed: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed + n)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=n, dtype=np.uint8)
    return rng.standard_normal(n).astype(dtype)


def python_base64(a: np.ndarray) -> bytes:
    """What the file holds for `a`: bytes as they are, floats as float64."""
    return base64.b64encode(a.tobytes() if a.dtype == np.uint8 else a.astype(np.float64).tobytes())


ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def strict_verdict(text: bytes):
    """(status, offset) of the strict decoder for `text` as bytes: the lowest offending offset and why (include/hippomm_hip.h)."""
    n = len(text)
    if n % 4:
        return BAD_LENGTH, n - n % 4
    for i, c in enumerate(text):
        v = ALPHABET.find(bytes([c]))
        if c == ord("="):
            if i < n - 2 or i % 4 < 2 or (i == n - 2 and text[n - 1] != ord("=")):
                return BAD_PADDING, i
        elif v < 0:
            return BAD_CHAR, i
        elif i == n - 3 and text[n - 2:] == b"==" and v & 15:
            return NONCANONICAL, i
        elif i == n - 2 and text[n - 1] == ord("=") and v & 3:
            return NONCANONICAL, i
    return OK, 0


def refusals():
    """(name, text, status, offset): one text per strictness rule, built from a valid 40-character text."""
    good = base64.b64encode(bytes(range(30)))                         # 40 characters, no padding
    two = base64.b64encode(bytes(range(28)))                          # ends "xx=="
    one = base64.b64encode(bytes(range(29)))                          # ends "xxx="
    assert two.endswith(b"==") and one.endswith(b"=") and not one.endswith(b"==")
    cases = [("bad character", good[:17] + b"*" + good[18:], BAD_CHAR, 17),
             ("bad character in the first place", b"\xff" + good[1:], BAD_CHAR, 0),
             ("embedded newline", good[:20] + b"\n" + good[20:] + b"\n\n\n", BAD_CHAR, 20),
             ("trailing newline", good + b"\n", BAD_LENGTH, 40),
             ("bad length", good[:-1], BAD_LENGTH, 36),
             ("padding in the middle", good[:8] + b"QQ==" + good[8:], BAD_PADDING, 10),
             ("padding, then a character", two[:-1] + b"A", BAD_PADDING, len(two) - 2),
             ("three paddings", two[:-3] + b"===", BAD_PADDING, len(two) - 3),
             ("only padding", b"====", BAD_PADDING, 0),
             ("non-canonical before two paddings", two[:-3] + b"R==", NONCANONICAL, len(two) - 3),
             ("non-canonical before one padding", one[:-2] + b"F=", NONCANONICAL, len(one) - 2),
             ("two offences, the lower wins", good[:5] + b" " + good[6:30] + b"=" + good[31:], BAD_CHAR, 5)]
    for name, text, status, offset in cases:
        assert strict_verdict(text) == (status, offset), (name, strict_verdict(text))
    return cases
