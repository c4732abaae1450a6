"""Shared corpora of tests/test_cpu_event_json_find.py and the GPU tests of the device span finder (csrc/event_json_find.hip).

The oracle is the host finder itself, ``hmm_json_find_matrices`` (csrc/event_json.cpp): every text here is a byte string the
finder must answer exactly as the host does -- list, count and order -- whether it is an event file, malformed JSON or noise.
A case is ``(name, text, min_values)``.  ``DECLINE`` names the only cases on which the block finder may answer DECLINED."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

import event_json_cases as jc

ROOT = jc.ROOT
GROUP = jc.header_constant("HMM_JSON_PARSE_GROUP_BYTES")
TOKEN_MAX = jc.header_constant("HMM_JSON_TOKEN_MAX")
MAX_SPAN = jc.header_constant("HMM_JSON_PARSE_MAX_SPAN_BYTES")
MAX_CANDIDATES = jc.header_constant("HMM_JSON_FIND_MAX_CANDIDATES")
FIND_OK, FIND_DECLINED = jc.header_constant("HMM_JSON_FIND_OK"), jc.header_constant("HMM_JSON_FIND_DECLINED")
NO_OFFSET = 2 ** 64 - 1
CAP = 64                                      # entries the helpers bring; no corpus text has more matrices


class Span(C.Structure):
    _fields_ = [("begin", C.c_size_t), ("end", C.c_size_t), ("rows", C.c_size_t), ("cols", C.c_size_t)]


def _as_list(spans, n):
    return [(int(s.begin), int(s.end), int(s.rows), int(s.cols)) for s in spans[:n]]


def host_find(raw: bytes, min_values: int = 1, cap: int = CAP):
    """``hmm_json_find_matrices`` -> (the list, n_found)."""
    from hippomm_amd import _lib
    spans, n = (Span * max(cap, 1))(), C.c_int(-1)
    assert _lib.load().hmm_json_find_matrices(raw, len(raw), min_values, C.cast(spans, C.c_void_p), cap, C.byref(n)) == 0
    return _as_list(spans, min(n.value, cap)), n.value


def blocks_find(raw: bytes, min_values: int = 1, cap: int = CAP):
    """``hmm_json_find_matrices_blocks`` -> (the list, the report as a dict)."""
    from hippomm_amd import _lib
    spans, report = (Span * max(cap, 1))(), (C.c_uint64 * 4)(7, 7, 7, 7)
    assert _lib.load().hmm_json_find_matrices_blocks(raw, len(raw), min_values, C.cast(spans, C.c_void_p), cap, C.cast(report, C.c_void_p)) == 0
    rep = dict(n_found=int(report[0]), n_candidates=int(report[1]), status=int(report[2]), first_declined=int(report[3]))
    return _as_list(spans, min(rep["n_found"], cap)), rep


# ---- event texts from the project's writers ----
def _matrix(rng, rows, cols, odd=False):
    m = rng.standard_normal((rows, cols)).astype(np.float32).astype(np.float64)
    if odd:
        m.reshape(-1)[[0, m.size // 2, m.size - 1]] = [float("nan"), float("inf"), float("-inf")]
    return m.tolist()


def _events():
    rng = np.random.default_rng(11)
    base = dict(event_id="e-1", frames=["f0.jpg", "f1.jpg"], frame_times=[0.0, 0.5], frame_captions=["a [[1,2]] b", 'q"uote'],
                audio_times=[[0.0, 1.0], [1.0, 2.5]], audio_transcription="so [ it ] goes")
    new = lambda feats: dict(base, features=feats, feature_times={k: [0.25 * i for i in range(len(v))] for k, v in feats.items()})  # noqa: E731
    old = lambda feats: dict(base, features={k: dict(features=v, times=[0.5 * i for i in range(len(v))]) for k, v in feats.items()})  # noqa: E731
    one = dict(vision=_matrix(rng, 3, 4))
    two = dict(vision=_matrix(rng, 3, 4), audio=_matrix(rng, 2, 6, odd=True))
    four = dict(vision=_matrix(rng, 5, 3), audio=_matrix(rng, 1, 12), text=_matrix(rng, 12, 1), depth=_matrix(rng, 4, 4, odd=True))
    small = dict(vision=_matrix(rng, 3, 4), tiny=_matrix(rng, 2, 2), flat=[1.0, 2.5, -3.0], cube=np.arange(24.0).reshape(2, 3, 4).tolist())
    return [("new-1", new(one)), ("new-2", new(two)), ("new-4", new(four)), ("old-1", old(one)), ("old-2", old(two)), ("old-4", old(four)),
            ("new-small-1d-3d", new(small)), ("old-small-1d-3d", old(small))]


def event_texts():
    cases = []
    for name, event in _events():
        for style, kw in (("none", dict(indent=None)), ("2", dict(indent=2)), ("4", dict(indent=4)), ("compact", dict(separators=(",", ":")))):
            raw = json.dumps(event, **kw).encode("ascii")
            for mv in (1, 12, 13):                             # 3 x 4 sits at min_values, 2 x 2 below it
                cases.append((f"event-{name}-{style}-min{mv}", raw, mv))
    return cases


# ---- strings ----
def strings():
    m = b"[[1,2],[3,4]]"
    texts = [b'{"a":"' + m + b'","b":' + m + b"}", b'"\\"' + m + b'"' + m, b'"x\\"",' + m, b'\\' + m, b'\\"' + m + b'"' + m,
             b'{"k":"v\\\\",' + b'"m":' + m + b"}", m + b'"' + m, m + b'"abc\\', b'"' + m, m + b"\\", b'[["1"]]' + m, b'[[1,"2"]]', b'[[1],"[2]"]',
             b'[ "[" [1]]', b'["[",[1]]' + m, b'[[1]"]"' + m]
    for k in range(1, 6):
        texts.append(b'"a' + b"\\" * k + b'"' + m + b'"' + m)
        texts.append(b"\\" * k + b'"' + m + b'"' + m)
    return [(f"string-{i}", t, 1) for i, t in enumerate(texts)]


# ---- single-byte edits of a small event ----
EDIT_BYTES = b'[],"\\ \n01-.eNx'


def edits():
    head, matrix, tail = b'{"s":"a]","m": ', b"[[1,-2.5e1], [NaN,40]]", b',"t":[7,8]}'
    event = head + matrix + tail
    lo, hi = len(head) - 3, len(head) + len(matrix) + 3
    cases = [("edit-none", event, 1)]
    for at in range(lo, hi):
        cases.append((f"edit-del-{at}", event[:at] + event[at + 1:], 1))
        for b in EDIT_BYTES:
            cases.append((f"edit-ins-{at}-{b}", event[:at] + bytes([b]) + event[at:], 1))
            cases.append((f"edit-rep-{at}-{b}", event[:at] + bytes([b]) + event[at + 1:], 1))
    return cases


# ---- shapes of failure ----
def failures():
    good = b"[[9,8],[7,6]]"
    texts = [b"[[1],[2,3],[4,5]]", b"[[1,2],[3],[4,5]]", b"[[1,2],[3,4],[5]]", b"[[1,2],[3,4],[5,6,7]]", b"[[2,1,3],[1,2],[1]]", b"[[]]", b"[[1,],[2]]",
             b"[[1] [2]]", b"[[01]]", b"[[1.]]", b"[[-NaN]]", b"[[1],[2]]]", b"[[[1]]", b"[[[1]]]", b"[[1,[2]]]", b"[[1],2]", b"[[1],[2],]", b"[,[1]]",
             b"[[1]],[[2]]", b"[[1 2]]", b"[[1],,[2]]", b"[[+1]]", b"[[.5]]", b"[[1e]]", b"[[Infinity,-Infinity,NaN]]", b"[[Infinityy]]", b"[[1]x]", b"[[1]",
             b"[[1],[2]", b"[[", b"[ [", b"]]", b"[[1\\]]", b"[[1e5,1E-5,0.0,-0]]", b"[[[[[1]]]]]", b"[[1],[[2]]]", b"[[[1],[2]],[[3],[4]]]"]
    cases = [(f"fail-{i}", t + b"," + good, 1) for i, t in enumerate(texts)] + [(f"fail-alone-{i}", t, 1) for i, t in enumerate(texts)]
    for rows, cols in ((3, 5), (5, 3), (1, 15), (15, 1), (4, 4)):
        t = json.dumps(np.arange(rows * cols).reshape(rows, cols).tolist()).encode()
        cases += [(f"min-{rows}x{cols}-{mv}", t, mv) for mv in (rows * cols - 1, rows * cols, rows * cols + 1)]
    return cases


# ---- group boundaries ----
def _across(body: bytes, k: int, d: int, pad: bytes = b" ") -> bytes:
    """`body` behind padding so that its byte k is the text's byte GROUP + d."""
    return pad * (GROUP + d - k) + body


def boundaries():
    cases = []
    items = [("quote", b'{"s":"a[[1]]b","m":[[1.5,2],[3,4]]}', lambda b: b.index(b'"a')),
             ("quote-close", b'{"s":"a[[1]]b","m":[[1.5,2],[3,4]]}', lambda b: b.index(b'b"') + 1),
             ("backslash-quote", b'{"s":"a\\"[[1]]","m":[[1.5,2],[3,4]]}', lambda b: b.index(b'\\"') + 1),
             ("cand", b'{"m":[ [1.5,2],[3,4]],"n":[[5]]}', lambda b: b.index(b"[ [") + 1),
             ("cand-tight", b'{"m":[[1.5,2],[3,4]],"n":[[5]]}', lambda b: b.index(b"[[") + 1),
             ("closer", b'{"m":[[1.5,2],[3,4]],"n":[[5]]}', lambda b: b.index(b"]]") + 1),
             ("closer-wide", b'{"m":[[1.5,2],[3,4] ],"n":[[5]]}', lambda b: b.index(b"] ]") + 1),
             ("token", b'{"m":[[1.5,2],[-12345.678e-3,4]]}', lambda b: b.index(b"345")),
             ("comma", b'{"m":[[1.5,2],[3,4]]}', lambda b: b.index(b"],[") + 1),
             ("bad-token", b'{"m":[[1.5,2],[12x45,4]]}', lambda b: b.index(b"x"))]
    for name, body, where in items:
        for d in (-1, 0, 1):
            cases.append((f"edge-{name}{d:+d}", _across(body, where(body), d), 1))
            cases.append((f"edge-{name}{d:+d}-in-string", b'"' + _across(body, where(body), d - 1), 1))
    wide = b" \n\t\r" * (GROUP // 2 + 33)                      # longer than two groups
    cases += [("ws-run-inside", b'{"m":[[1,2],' + wide + b"[3,4]]}", 1), ("ws-run-candidate", b'{"m":[' + wide + b"[1,2],[3,4]]}", 1),
              ("ws-run-closer", b'{"m":[[1,2],[3,4]' + wide + b"]}", 1), ("ws-run-comma", b"[[1,2]" + wide + b"," + wide + b"[3,4]]", 1),
              ("ws-run-ragged", b"[[1,2]," + wide + b"[3]]", 1), ("ws-run-string", b'"' + wide + b'[[1]]"' + wide + b"[[2]]", 1)]
    big = np.random.default_rng(5).standard_normal((64, 1024)).astype(np.float32).astype(np.float64)
    raw = json.dumps(dict(features=dict(vision=big.tolist()), n=[[1, 2], [3, 4]]), separators=(",", ":")).encode()
    assert len(raw) > 257 * GROUP
    cases += [("matrix-over-256-groups", raw, 1024), ("matrix-over-256-groups-ragged", raw.replace(b"],[", b",1],[", 1), 1024)]
    cases += [("one-byte-[", b"[", 1), ("one-byte-1", b"1", 1), ("one-byte-quote", b'"', 1), ("two-bytes", b"[[", 1)]
    m = b"[[1,2],[3,4]]"
    for n in (GROUP - 1, GROUP, GROUP + 1):
        cases += [(f"len-{n}-head", m + b" " * (n - len(m)), 1), (f"len-{n}-tail", b" " * (n - len(m)) + m, 1),
                  (f"len-{n}-cut", (b" " * (n - len(m) + 1) + m)[:n], 1)]
    return cases


# ---- the decline cases, and only these ----
def _number(n: int) -> bytes:
    return b"1" * (n - 4) + b".5e3"


DECLINE = {"long-65-inside", "long-200-inside", "long-65-inside-edge"}


def long_tokens():
    inside = lambda n: b'{"m":[[1,' + _number(n) + b"],[2,3]]}"            # noqa: E731
    outside = lambda n: b'{"v":[1,' + _number(n) + b'],"m":[[1,2],[2,3]]}'   # noqa: E731
    return [("long-65-inside", inside(TOKEN_MAX + 1), 1), ("long-200-inside", inside(200), 1), ("long-64-inside", inside(TOKEN_MAX), 1),
            ("long-65-outside", outside(TOKEN_MAX + 1), 1), ("long-200-outside", outside(200), 1),
            ("long-65-inside-edge", _across(inside(TOKEN_MAX + 1), 20, 0), 1), ("long-64-inside-edge", _across(inside(TOKEN_MAX), 20, 0), 1),
            ("long-65-inside-too-small", inside(TOKEN_MAX + 1), 5), ("long-65-garbage-inside", b"[[1," + b"1" * 40 + b"x" + b"1" * 40 + b"]]", 1),
            ("long-65-inside-broken", b"[[1," + _number(TOKEN_MAX + 1) + b",],[2]]", 1)]


def all_cases():
    return event_texts() + strings() + edits() + failures() + boundaries() + long_tokens()


# ---- seeded random texts ----
PIECES = [b"[", b"]", b",", b'"', b"\\", b" ", b"\n", b"0", b"1", b"-", b".", b"e", b"N", b"x", b"[[", b"]]", b"],[", b"[[1,2],[3,4]]", b"[[1],[2]]",
          b"[1,2]", b"1.5", b"NaN", b"-Infinity", b'"a"', b'\\"', b"[[1,2]", b",[3,4]]", b"\t", b"\r", b"]]]", b"[[[", b"12", b"1e5"]


def random_short(seed: int, n: int):
    """n texts of 1 to 12 pieces -> (text, min_values)."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 13, n)
    picks = rng.integers(0, len(PIECES), int(lengths.sum())).tolist()
    mins = rng.integers(1, 5, n).tolist()
    out, at = [], 0
    for k, mv in zip(lengths.tolist(), mins):
        out.append((b"".join(PIECES[i] for i in picks[at:at + k]), mv))
        at += k
    return out


def _random_matrix(rng) -> bytes:
    rows, cols = int(rng.integers(1, 7)), int(rng.integers(1, 9))
    m = np.round(rng.standard_normal((rows, cols)) * 100, int(rng.integers(0, 6))).tolist()
    if rng.random() < 0.2:                                         # ragged
        m[int(rng.integers(0, rows))].append(1.0)
    style = int(rng.integers(0, 4))
    return json.dumps(m, **[dict(indent=None), dict(indent=2), dict(indent=1), dict(separators=(",", ":"))][style]).encode()


def random_long(seed: int, n: int):
    """n texts of 8 to 20 KiB put together from matrices, strings and noise -> (text, min_values)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        want, parts, size = int(rng.integers(8 * 1024, 20 * 1024 + 1)), [], 0
        while size < want:
            kind = rng.random()
            if kind < 0.55:
                p = _random_matrix(rng)
            elif kind < 0.7:
                p = b'"' + b"".join(PIECES[i] for i in rng.integers(0, len(PIECES), int(rng.integers(0, 8))).tolist()).replace(b'"', b'\\"') + b'"'
                if p.endswith(b'\\"'):
                    p = p[:-2] + b'"'
            elif kind < 0.8:
                p = b" " * int(rng.integers(1, 200))
            else:
                p = b"".join(PIECES[i] for i in rng.integers(0, len(PIECES), int(rng.integers(1, 6))).tolist())
            parts.append(p)
            parts.append([b",", b", ", b":", b"\n", b""][int(rng.integers(0, 5))])
            size += len(p) + len(parts[-1])
        out.append((b"".join(parts)[:want], int(rng.integers(1, 9))))
    return out
