"""Shared inputs and references of tests/test_cpu_event_json_device.py and the GPU tests of the device JSON writer.

The reference is Python itself: ``json.dumps`` of a float is ``float.__repr__`` (``NaN`` / ``Infinity`` / ``-Infinity`` for the
non-finite ones), and the text of a matrix is ``json.dumps(m.tolist(), indent=2)`` with `close_indent` spaces in front of every
line but the first -- what ``json.dumps(indent=2)`` writes for that list nested that deep."""
from __future__ import annotations

import functools
import json
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def header_constant(name: str) -> int:
    text = (ROOT / "include" / "hippomm_hip.h").read_text()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1))


VALUES_PER_GROUP = header_constant("HMM_JSON_VALUES_PER_GROUP")
SCAN_SUMS_PER_ROUND = header_constant("HMM_JSON_SCAN_SUMS_PER_ROUND")
VALUES_PER_SCAN_ROUND = VALUES_PER_GROUP * SCAN_SUMS_PER_ROUND
REPR_BYTES = header_constant("HMM_JSON_REPR_BYTES")

# the longest texts: 24 characters as a double; a widened fp32 has two exponent digits at most, hence 23
LONGEST_F64 = -1.2345678901234567e-308
LONGEST_F32 = float(np.float32(-1.2345679e-38))
assert len(repr(LONGEST_F64)) == 24 and len(repr(LONGEST_F32)) == 23

ODD_VALUES = [
    1e16, 9999999999999998.0, 0.0001, 1e-05,                                   # both notation switches
    5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 2.0 ** 53, 0.1, 0.3, 1 / 3,
    1.0, 100.0, 1e22, 1e100, 1.5e-300, -1e-100, -0.0, 0.0, float("nan"), float("inf"), -float("inf"),
    LONGEST_F64, 123456.789, 2.0 ** -1074 * 3,
]


def python_reprs(values) -> list:
    """``json.dumps`` of each double, as bytes."""
    spell = {"nan": b"NaN", "inf": b"Infinity", "-inf": b"-Infinity"}
    return [spell.get(s) or s.encode("ascii") for s in map(repr, np.asarray(values, np.float64).tolist())]


def core_reprs(values) -> list:
    """``hmm_json_float_repr`` (the device's printer, run on the host) of each double."""
    from hippomm_amd import _lib
    v = np.ascontiguousarray(values, np.float64).reshape(-1)
    chars = np.zeros(v.size * REPR_BYTES, np.uint8)
    lengths = np.full(v.size, -1, np.int32)
    assert _lib.load().hmm_json_float_repr(v.ctypes.data, v.size, chars.ctypes.data, lengths.ctypes.data) == 0
    assert lengths.min(initial=1) >= 1 and lengths.max(initial=1) <= REPR_BYTES
    raw = chars.tobytes()
    return [raw[REPR_BYTES * i: REPR_BYTES * i + n] for i, n in enumerate(lengths.tolist())]


def host_writer_reprs(values) -> list:
    """The same doubles through ``hmm_json_write_matrix_f64`` (the second oracle): one row, its value lines cut out."""
    from hippomm_amd import event_store as es
    v = np.ascontiguousarray(values, np.float64).reshape(1, -1)
    lines = es._matrix_bytes_host(v, 0).split(b"\n")
    assert lines[0] == b"[" and lines[1] == b"  [" and lines[-2] == b"  ]" and lines[-1] == b"]"
    return [line.strip().rstrip(b",") for line in lines[2:-2]]


def every_exponent(rng, randoms: int = 40) -> np.ndarray:
    """Every binary exponent of a double, subnormals (0) through the largest finite (2046), each with the smallest and the largest
    mantissa and `randoms` random ones: walks every entry of both power-of-five tables."""
    bits = []
    for e in range(0, 2047):
        mantissas = [0, 2 ** 52 - 1] + [int(x) for x in rng.integers(0, 2 ** 52, randoms)]
        bits += [(e << 52) | m for m in mantissas if e or m]
    return np.array(bits, np.uint64).view(np.float64)


def powers_of_ten() -> np.ndarray:
    out = []
    for k in range(-323, 309):
        x = float(f"1e{k}")
        out += [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]
    return np.array(out, np.float64)


def matrix_text(m: np.ndarray, close_indent: int) -> bytes:
    """``json.dumps(m.tolist(), indent=2)`` nested so that its closing bracket sits at `close_indent` spaces."""
    return _matrix_text_at_zero(m.dtype.str, m.shape, m.tobytes()).replace(b"\n", b"\n" + b" " * close_indent)


@functools.lru_cache(maxsize=64)
def _matrix_text_at_zero(dtype, shape, raw) -> bytes:
    return json.dumps(np.frombuffer(raw, dtype).reshape(shape).tolist(), indent=2).encode("ascii")


def alternating(shape, dtype) -> np.ndarray:
    """Neighbours alternate between the shortest text (0.0) and the longest, so that every offset depends on the scan."""
    n = shape[0] * shape[1]
    flat = np.zeros(n, dtype)
    flat[1::2] = LONGEST_F64 if dtype == np.float64 else LONGEST_F32
    if n > 2:
        flat[n // 2] = 0.5                                          # and the rhythm breaks once: a constant offset error would show
    return flat.reshape(shape)


def odd_at_group_edges(dtype) -> np.ndarray:
    """Random values with every ODD_VALUES entry at the first and at the last position of a workgroup's range; fp64 as one long
    row, fp32 (where the odd values are rounded, some to inf or 0) in rows of 7, which no workgroup boundary respects."""
    groups = len(ODD_VALUES)
    n = groups * VALUES_PER_GROUP
    n += 7 - n % 7
    flat = np.random.default_rng(17).standard_normal(n)
    for g, x in enumerate(ODD_VALUES):
        flat[g * VALUES_PER_GROUP] = x
        flat[(groups - 1 - g) * VALUES_PER_GROUP + VALUES_PER_GROUP - 1] = x
    flat[-1] = ODD_VALUES[0]
    with np.errstate(over="ignore", under="ignore"):
        return flat.astype(dtype).reshape((1, n) if dtype == np.float64 else (n // 7, 7))
