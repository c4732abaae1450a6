"""GPU: the memory contract of hmm_json_parse_matrix_device in the guarded arena (tests/arena.py).  The text, the output, the
report, the flagged list and the workspace are carved at exactly their size, at odd alignments, under the three poison patterns:
every guard still holds its pattern afterwards, the text is unchanged, `out` holds exactly rows x cols defined values -- the same
under all three patterns (a byte read outside the span or a workspace word read before it is written would differ between two of
them) --, the flagged list is untouched behind min(n_flagged, cap) and the workspace behind its stated size.  The same for a
token count that is not rows x cols, where nothing behind the tokens that exist is written -- and the call can be captured into a
graph whose replay reads new text."""
import numpy as np
import pytest
import torch

import arena as A
import event_json_parse_cases as pc

pytestmark = pytest.mark.gpu

G = pc.GROUP_BYTES
CAP = 3


def _text(n_values, cols, style, flagged=()):
    toks = pc.f32_origin(np.random.default_rng(21), n_values)[:n_values]
    for at, lit in flagged:
        toks[at] = lit
    return toks, pc.text_of(toks, cols, style)


def _midpoints():
    return [pc._written_out(pc._midpoint(x)) for x in (2.0 ** 70 * 1.2345, 2.0 ** 80 * 1.75001, 0.0123456789, 2.0 ** 66 * 1.1)]


# (values, cols, style, flagged literals at these ordinals, lead bytes in front of the span, fp64)
CASES = [(15, 5, "indent", 0, 1, False), (1, 1, "compact", 0, 0, True), (7 * 64, 7, "compact", 2, 5, False),
         (3 * 257, 257, "indent", 4, 3, True), (33 * 11, 11, "crlf", 3, 2, False)]


def _setup(pattern, raw, span, f64, extra_ws=256):
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    begin, end, rows, cols = span
    elem = 8 if f64 else 4
    ws_bytes = lib.hmm_json_parse_matrix_device_workspace_bytes(end - begin)
    ar = A.GuardedArena(A.needed_bytes([len(raw), rows * cols * elem, 32, 32 * CAP, ws_bytes + extra_ws]), dev, A.PATTERNS[pattern])
    v = dict(text=ar.put(torch.frombuffer(bytearray(raw), dtype=torch.uint8), "text", align=1), out=ar.carve(rows * cols * elem, "out", align=elem),
             report=ar.carve(32, "report", align=8), flagged=ar.carve(32 * CAP, "flagged", align=8),
             ws=ar.carve(ws_bytes + extra_ws, "workspace", align=8))
    return ar, v, ws_bytes


def _call(ar, v, span, f64, ws_bytes):
    from hippomm_amd import _lib
    begin, end, rows, cols = span
    return _lib.load().hmm_json_parse_matrix_device(ar.address(v["text"]), begin, end, rows, cols, 1 if f64 else 0, ar.address(v["out"]),
                                                    ar.address(v["report"]), ar.address(v["flagged"]), CAP, ar.address(v["ws"]), ws_bytes,
                                                    _lib.stream_ptr())


def _report(v):
    w = v["report"].cpu().numpy().view(np.uint64)
    return dict(n_tokens=int(w[0]), n_flagged=int(w[1]), first_bad=int(w[2]), status=int(w[3]))


def _flagged(v, n):
    return sorted(tuple(e) for e in v["flagged"].cpu().numpy().view(np.uint64)[:4 * n].reshape(-1, 4).tolist())


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}v-{c[2]}-{c[3]}flagged-lead{c[4]}-{'f64' if c[5] else 'f32'}")
def test_guards_hold_inputs_stay_and_the_result_does_not_depend_on_the_poison(case):
    from hippomm_amd import _lib
    n_values, cols, style, n_flag, lead, f64 = case
    ordinals = [(i + 1) * n_values // (n_flag + 1) for i in range(n_flag)]
    toks, body = _text(n_values, cols, style, list(zip(ordinals, _midpoints())))
    raw = b"9876543210"[:lead] + body + b"1,2]"                       # numbers on both sides of the span, were they read
    span = (lead, lead + len(body), n_values // cols, cols)
    if f64:
        want = pc.json_f64(raw, span).view(np.uint64).reshape(-1).copy()
    else:
        want = pc.host_f32(_lib.load(), raw, span).view(np.uint32).reshape(-1).copy()
    want[ordinals] = 0                                             # flagged slots are written as zero
    want_entries = sorted((k, raw.index(toks[k]), raw.index(toks[k]) + len(toks[k]), pc.UNDECIDED) for k in ordinals)
    for pattern in A.PATTERNS:
        ar, v, ws_bytes = _setup(pattern, raw, span, f64)
        for attempt in range(2):                                       # the second call finds a re-poisoned workspace, output and report
            assert _call(ar, v, span, f64, ws_bytes) == 0
            torch.cuda.synchronize()
            ar.check_guards()
            assert v["text"].cpu().numpy().tobytes() == raw, pattern
            assert _report(v) == dict(n_tokens=n_values, n_flagged=n_flag, first_bad=pc.NO_OFFSET, status=pc.OK), (pattern, attempt)
            got = v["out"].cpu().numpy().view(np.uint64 if f64 else np.uint32)
            assert (got == want).all(), (pattern, attempt, np.nonzero(got != want)[0][:5])
            listed = min(n_flag, CAP)
            assert set(_flagged(v, listed)) <= set(want_entries) and len(set(_flagged(v, listed))) == listed, (pattern, attempt)
            assert ar.is_pattern(v["flagged"], start=32 * listed), (pattern, attempt)      # nothing behind the entries that exist
            assert ar.is_pattern(v["ws"], start=ws_bytes), (pattern, attempt)              # nor behind the stated workspace
            for key in ("ws", "out", "report", "flagged"):
                ar.repoison(v[key])


@pytest.mark.parametrize("delta", [-1, 1], ids=["a-row-fewer", "a-row-more"])
def test_a_token_count_that_is_not_rows_x_cols_writes_nothing_behind_the_matrix_or_the_tokens(delta):
    from hippomm_amd import _lib
    rows, cols = 40, 9                                             # 360 values, more than two groups of text
    toks, body = _text(rows * cols, cols, "indent")
    assert len(body) > 2 * G
    raw = b"77" + body
    stated = rows + delta
    span = (2, 2 + len(body), stated, cols)
    full = pc.host_f32(_lib.load(), raw, (2, 2 + len(body), rows, cols)).view(np.uint32).reshape(-1)
    results = []
    for pattern in A.PATTERNS:
        ar, v, ws_bytes = _setup(pattern, raw, span, False)
        assert _call(ar, v, span, False, ws_bytes) == 0
        torch.cuda.synchronize()
        ar.check_guards()                                          # the carve of `out` ends at stated x cols values
        assert _report(v) == dict(n_tokens=rows * cols, n_flagged=0, first_bad=pc.NO_OFFSET, status=pc.COUNT), pattern
        written = min(rows, stated) * cols
        got = v["out"].cpu().numpy().view(np.uint32)
        assert (got[:written] == full[:written]).all(), pattern
        assert ar.is_pattern(v["out"], start=4 * written) and ar.is_pattern(v["flagged"]) and ar.is_pattern(v["ws"], start=ws_bytes), pattern
        assert v["text"].cpu().numpy().tobytes() == raw
        results.append(got[:written].copy())
    assert all((r == results[0]).all() for r in results)


def test_the_call_is_graph_capturable_and_a_replay_reads_new_text():
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    toks, first = _text(7 * 64, 7, "compact")
    second = pc.text_of(toks[::-1], 7, "compact")                    # the same bytes in another order: same length, other values
    assert len(second) == len(first) > 2 * G
    span = (0, len(first), 64, 7)
    text = torch.frombuffer(bytearray(first), dtype=torch.uint8).to(dev)
    out = torch.zeros(64 * 7, dtype=torch.int32, device=dev)
    report = torch.zeros(4 + 4 * CAP, dtype=torch.int64, device=dev)
    ws_bytes = lib.hmm_json_parse_matrix_device_workspace_bytes(len(first))
    ws = torch.zeros(ws_bytes // 8, dtype=torch.int64, device=dev)

    def call():
        assert lib.hmm_json_parse_matrix_device(text.data_ptr(), 0, len(first), 64, 7, 0, out.data_ptr(), report.data_ptr(), report.data_ptr() + 32,
                                                CAP, ws.data_ptr(), ws_bytes, _lib.stream_ptr()) == 0

    def bits(raw):
        torch.cuda.synchronize()
        assert report[:4].tolist() == [64 * 7, 0, -1, pc.OK]
        return out.cpu().numpy().view(np.uint32).tobytes() == pc.host_f32(lib, raw, span).tobytes()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    assert bits(first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    out.zero_()
    report.zero_()
    graph.replay()
    assert bits(first)
    text.copy_(torch.frombuffer(bytearray(second), dtype=torch.uint8))   # new text of the same length, same graph
    graph.replay()
    assert bits(second)


def test_bad_arguments_are_refused_with_nothing_written():
    from hippomm_amd import _lib
    toks, body = _text(15, 5, "indent")
    span = (0, len(body), 3, 5)
    ar, v, ws_bytes = _setup("ones", body, span, False)
    lib = _lib.load()
    args = lambda **c: [c.get("text", ar.address(v["text"])), c.get("begin", 0), len(body), 3, 5, c.get("dtype", 0), ar.address(v["out"]),  # noqa: E731
                        ar.address(v["report"]), ar.address(v["flagged"]), c.get("cap", CAP), ar.address(v["ws"]), c.get("ws_bytes", ws_bytes),
                        _lib.stream_ptr()]
    assert lib.hmm_json_parse_matrix_device(*args(ws_bytes=ws_bytes - 1)) == -1 and b"json_parse_matrix_device" in lib.hmm_last_error()
    assert lib.hmm_json_parse_matrix_device(*args(begin=len(body))) == -1
    assert lib.hmm_json_parse_matrix_device(*args(dtype=2)) == -1
    assert lib.hmm_json_parse_matrix_device(*args(cap=-1)) == -1
    torch.cuda.synchronize()
    for key in ("out", "report", "flagged", "ws"):
        assert ar.is_pattern(v[key]), key
    ar.check_guards()
