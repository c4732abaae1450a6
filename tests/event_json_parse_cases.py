"""Shared corpus and references of tests/test_cpu_event_json_parse.py and the GPU tests of the device JSON parser.

The reference is Python itself: a number token of a JSON file becomes ``float(token)`` (``json.loads`` calls exactly that for a
literal with a '.' or an exponent, and ``np.array`` widens its ints the same way), and an fp32 feature is
``np.float32(float(token))``.  Which tokens the parser may FLAG instead of converting is a rule, stated here with Python integers
(``expected_flag``), not whatever the parser happens to do."""
from __future__ import annotations

import json
import math
import re
from fractions import Fraction

import numpy as np

import event_json_cases as jc

ROOT = jc.ROOT
TOKEN_MAX = jc.header_constant("HMM_JSON_TOKEN_MAX")
GROUP_BYTES = jc.header_constant("HMM_JSON_PARSE_GROUP_BYTES")
SCAN_GROUPS_PER_ROUND = jc.header_constant("HMM_JSON_PARSE_SCAN_GROUPS_PER_ROUND")
OK, COUNT, BAD_BYTE, BAD_TOKEN = (jc.header_constant(f"HMM_JSON_PARSE_{n}") for n in ("OK", "COUNT", "BAD_BYTE", "BAD_TOKEN"))
UNDECIDED, RANGE, TOO_LONG, BAD = (jc.header_constant(f"HMM_JSON_FLAG_{n}") for n in ("UNDECIDED", "RANGE", "TOO_LONG", "BAD_TOKEN"))
NO_OFFSET = 2 ** 64 - 1

NUMBER = re.compile(rb"(-?)(0|[1-9][0-9]*)(?:\.([0-9]+))?(?:[eE]([+-]?[0-9]+))?")
INTEGER = re.compile(rb"-?[0-9]+")
PLAIN = [b"0", b"-0", b"-0.0", b"0.0", b"-0e0", b"0e5", b"-0E-5", b"1E5", b"1e+05", b"1e-05", b"1", b"-1", b"10", b"123456789",
         b"9007199254740993", b"9223372036854775807", b"9999999999999999999", b"1000000000000000000", b"-9223372036854775808",
         b"0.1", b"0.5e0", b"2.5E-3", b"NaN", b"Infinity", b"-Infinity", b"0.000", b"100.0", b"1.0e0", b"5e-324", b"4.9e-324",
         b"2.4703282292062328e-324", b"2.4703282292062327e-324", b"1.7976931348623157e308", b"1.7976931348623158e308",
         b"2.2250738585072014e-308", b"2.2250738585072011e-308", b"0e99999", b"1e00005", b"1e-0", b"0.0e-9999"]
BAD_TOKENS = [b"+1", b".5", b"1.", b"1e", b"--1", b"Inf", b"nan", b"01", b"-", b"1e+", b"1.e5", b"-NaN", b"Infinit", b"Infinityy", b"NaNN",
              b"1-2", b"1.2.3", b"1e5e5", b"e5", b"-.5", b"00", b"-01.5", b"1E", b"infinity", b"0x10", b"1e5.0", b"-Inf", b"tNaN"]


def core_parse(tokens):
    """``hmm_json_float_parse`` (the device's parser, run on the host) on every token -> (fp64 bits, fp32 bits, flags)."""
    from hippomm_amd import _lib
    lengths = np.fromiter(map(len, tokens), np.int64, len(tokens))
    ends = np.cumsum(lengths + 1) - 1                              # one space between two tokens
    spans = np.stack([ends - lengths, ends], axis=1).astype(np.uint64)
    text = b" ".join(tokens)
    f64, f32, flags = np.full(len(tokens), 7, np.uint64), np.full(len(tokens), 7, np.uint32), np.full(len(tokens), -1, np.int32)
    assert _lib.load().hmm_json_float_parse(text, spans.ctypes.data, len(tokens), f64.ctypes.data, f32.ctypes.data, flags.ctypes.data) == 0
    return f64, f32, flags


def python_bits(tokens):
    """``float(token)`` and ``np.float32(float(token))`` as bits.  A literal without '.' or exponent is an int to ``json.loads``
    and widened from that: the same value, except that "-0" is 0 and has no sign."""
    d = np.array([float(t) if INTEGER.fullmatch(t) is None else float(int(t)) for t in tokens], np.float64)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return d.view(np.uint64), d.astype(np.float32).view(np.uint32)


def _rounds_out_of_range(w: int, q: int) -> bool:
    """Does w x 10^q (w > 0), correctly rounded, leave the finite non-zero doubles?  Integer division of Python ints is correctly
    rounded (ties to even) over the whole range, subnormals included, and raises instead of returning infinity."""
    return _rounded(w, q) in (0.0, float("inf"))


def _rounded(w: int, q: int) -> float:
    try:
        return w * 10 ** q / 1 if q >= 0 else w / 10 ** -q
    except OverflowError:
        return float("inf")


def expected_flag(token: bytes) -> int:
    """The rule of event_json_parse_core.h, from the characters alone."""
    if len(token) > TOKEN_MAX:
        return TOO_LONG
    if token in (b"NaN", b"Infinity", b"-Infinity"):
        return 0
    m = NUMBER.fullmatch(token)
    if m is None:
        return BAD
    _, whole, frac, exp = m.groups()
    frac = frac or b""
    e = int(exp) if exp else 0
    if abs(e) > 9999:
        return RANGE
    digits = (whole + frac).lstrip(b"0")                            # significant digits: from the first non-zero one
    if not digits:
        return 0
    nd, q = len(digits), e - len(frac)
    if nd <= 19:
        if -300 < q + nd < 300:                                     # 10^(q + nd - 1) <= value < 10^(q + nd): well inside the range
            return 0
        return RANGE if _rounds_out_of_range(int(digits), q) else 0
    w, q = int(digits[:19]), q + nd - 19
    a, b = _rounded(w, q), _rounded(w + 1, q)
    if a != b:
        return UNDECIDED
    return RANGE if a in (0.0, float("inf")) else 0


def f32_origin(rng, n: int):
    """``repr(float(np.float32(x)))`` -- what an event file holds -- for n random fp32 bit patterns and every fp32 binary exponent
    at its smallest and largest mantissa, both signs."""
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    edges = np.array([(s << 31) | (e << 23) | m for s in (0, 1) for e in range(256) for m in (0, 2 ** 23 - 1)], np.uint32)
    with np.errstate(invalid="ignore"):                             # signalling NaNs among the patterns
        return jc.python_reprs(np.concatenate([bits, edges]).view(np.float32).astype(np.float64))


def doubles(rng):
    named = [5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1.7976931348623157e308, 2.0 ** -1022, 2.0 ** -1074 * 3]
    return jc.python_reprs(np.concatenate([jc.every_exponent(rng), np.array(named + [-x for x in named])]))


def powers_of_ten():
    return [b"1e%d" % k for k in range(-330, 311)]


def _midpoint(x: float) -> Fraction:
    """The exact midpoint between the positive double x and the next one up."""
    return (Fraction(x) + Fraction(float(np.nextafter(x, np.inf)))) / 2


def _nineteen_digits(v: Fraction):
    """floor(v x 10^k) with k such that it has exactly 19 digits -> (that integer, k)."""
    k = 18 - math.floor(math.log10(v.numerator) - math.log10(v.denominator))       # an estimate, put right below
    while True:
        n = math.floor(v * Fraction(10) ** k)
        if n >= 10 ** 19:
            k -= 1
        elif n < 10 ** 18:
            k += 1
        else:
            return n, k


def beside_halfway(rng, n: int):
    """19-digit literals just below and just above the exact midpoint between a random double and its neighbour."""
    bits = (rng.integers(1, 2046, n, dtype=np.uint64) << np.uint64(52)) | rng.integers(0, 2 ** 52, n, dtype=np.uint64)
    out = []
    for x in bits.view(np.float64).tolist():
        lo, k = _nineteen_digits(_midpoint(x))
        out += [b"%de%d" % (v, -k) for v in (lo - 1, lo, lo + 1) if 10 ** 18 <= v < 10 ** 19]
    return out


def _written_out(v: Fraction) -> bytes:
    """A dyadic rational as a plain decimal literal, every digit."""
    places = v.denominator.bit_length() - 1                         # denominator 2^places: that many digits behind the point
    n = v.numerator * 5 ** places
    s = str(n).rjust(places + 1, "0")
    return (s[:len(s) - places] + ("." + s[len(s) - places:] if places else "")).encode()


def long_literals(rng, n: int):
    """Exact midpoints between neighbouring doubles written out in full -- integers of 20 to 30 digits, fractions of up to a
    hundred -- and the full expansions of doubles themselves, which have more than 19 digits and are decidable."""
    out = []
    for lo_e, hi_e in ((64, 100), (-12, 3), (-45, -12), (-200, -60)):
        for e in rng.integers(lo_e, hi_e, n).tolist():
            x = float(np.ldexp(1.0 + rng.random(), e))
            out += [_written_out(_midpoint(x)), _written_out(Fraction(x)), b"-" + _written_out(_midpoint(x))]
    out += [b"9007199254740993", b"9007199254740992.5", b"9007199254740993.0000000000000000001", b"1" + b"0" * 30, b"1." + b"0" * 40,
            b"0." + b"0" * 30 + b"1", b"1" + b"0" * 400, b"1" + b"0" * 30 + b"e-40", b"1." + b"0" * 70 + b"e5", b"17976931348623158" + b"0" * 292,
            b"0." + b"0" * 323 + b"24703282292062327", b"12345678901234567890123e-400", b"98765432109876543210e300"]
    return out


def f32_double_rounding(rng, n: int):
    """19-digit literals within 10^-18 relative (below 2^-59) of an fp32 midpoint whose own expansion is longer: the double nearest
    to either is the midpoint itself, so (float)(double) goes to the even fp32 on both sides, where direct rounding would part."""
    out = []
    for e, m in zip(rng.integers(-100, 100, n).tolist(), rng.integers(0, 2 ** 23, n).tolist()):
        mid = Fraction(2 * (2 ** 23 + m) + 1) * Fraction(2) ** (e - 24)
        lo, k = _nineteen_digits(mid)
        if Fraction(lo, 1) * Fraction(10) ** -k != mid:
            out += [b"%de%d" % (lo, -k), b"%de%d" % (lo + 1, -k)]
    return out


# ---- texts of matrices, for the GPU tests ----
def find_span(lib, raw: bytes, min_values: int = 1):
    """The first matrix ``hmm_json_find_matrices`` reports in raw -> (begin, end, rows, cols)."""
    import ctypes as C
    out = (C.c_size_t * 4)()
    n = C.c_int(0)
    assert lib.hmm_json_find_matrices(raw, len(raw), min_values, C.cast(out, C.c_void_p), 1, C.byref(n)) == 0 and n.value >= 1
    return tuple(out)


def host_f32(lib, raw: bytes, span):
    """``hmm_json_parse_matrix_f32`` on the span, or None when it declines."""
    a = np.full((span[2], span[3]), 7, np.float32)
    return a if lib.hmm_json_parse_matrix_f32(raw, span[0], span[1], span[2], span[3], a.ctypes.data) == 0 else None


def json_f64(raw: bytes, span) -> np.ndarray:
    return np.array(json.loads(raw[span[0]:span[1]]), np.float64)


def text_of(tokens, cols: int, style: str = "indent") -> bytes:
    """The tokens as a matrix with `cols` columns: "indent" as json.dumps(indent=2) lays it out at close_indent 4, "compact" as
    json.dumps does, "crlf" with \\r\\n line ends and tabs."""
    rows = [tokens[i:i + cols] for i in range(0, len(tokens), cols)]
    if style == "indent":
        return b"[\n" + b",\n".join(b"      [\n" + b",\n".join(b"        " + t for t in r) + b"\n      ]" for r in rows) + b"\n    ]"
    if style == "compact":
        return b"[" + b", ".join(b"[" + b", ".join(r) + b"]" for r in rows) + b"]"
    return b"[\r\n" + b",\r\n".join(b"\t[\r\n" + b",\r\n".join(b"\t\t" + t for t in r) + b"\r\n\t]" for r in rows) + b"\r\n]"
