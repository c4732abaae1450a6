"""GPU: the memory contract of hmm_json_find_matrices_device in the guarded arena (tests/arena.py).  The text, the output, the
report and the workspace are carved at exactly their size, the text at odd alignments, under the three poison patterns: every
guard still holds its pattern afterwards, the text is unchanged, the list and the report are the host finder's -- the same under
all three patterns (a byte read outside the text or a workspace word read before it is written would differ between two of them)
--, `out` keeps its poison from min(n_found, cap) entries on and the workspace behind its stated size.  Bytes that would change the
answer -- a `[[` and a `"` -- placed just outside each end of the text change nothing."""
import numpy as np
import pytest
import torch

import arena as A
import event_json_find_cases as fc

pytestmark = pytest.mark.gpu

G = fc.GROUP


def _texts():
    cases = {name: (raw, mv) for name, raw, mv in fc.event_texts() + fc.boundaries() + fc.long_tokens() + fc.failures()}
    names = ["event-new-small-1d-3d-2-min1", "event-old-4-compact-min12", "edge-cand+0", "edge-closer-1", "ws-run-candidate", "len-4096-tail",
             "len-4097-cut", "long-65-inside", "fail-alone-29", "one-byte-["]
    return [(n,) + cases[n] for n in names]


def _setup(pattern, raw, cap, lead=0, before=b"", after=b"", extra_ws=512):
    """The text carved `lead` bytes (plus len(before)) behind a 256-byte boundary, `before` and `after` beside it in the same carve."""
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    ws_bytes = lib.hmm_json_find_matrices_device_workspace_bytes(len(raw))
    whole = before + raw + after
    ar = A.GuardedArena(A.needed_bytes([len(whole) + 256, 32 * cap, 32, ws_bytes + extra_ws]), dev, A.PATTERNS[pattern])
    v = dict(text=ar.put(torch.frombuffer(bytearray(whole), dtype=torch.uint8), "text", align=lead if lead else 256),
             out=ar.carve(32 * cap, "out", align=8), report=ar.carve(32, "report", align=8), ws=ar.carve(ws_bytes + extra_ws, "workspace", align=8))
    return ar, v, ws_bytes, whole


def _call(ar, v, raw, min_values, cap, ws_bytes, skip=0):
    from hippomm_amd import _lib
    return _lib.load().hmm_json_find_matrices_device(ar.address(v["text"]) + skip, len(raw), min_values, ar.address(v["out"]) if cap else None, cap,
                                                     ar.address(v["report"]), ar.address(v["ws"]), ws_bytes, _lib.stream_ptr())


def _report(v):
    w = v["report"].cpu().numpy().view(np.uint64)
    return dict(n_found=int(w[0]), n_candidates=int(w[1]), status=int(w[2]), first_declined=int(w[3]))


def _listed(v, n):
    return [tuple(int(x) for x in e) for e in v["out"].cpu().numpy().view(np.uint64)[:4 * n].reshape(-1, 4)]


@pytest.mark.parametrize("case", _texts(), ids=lambda c: c[0])
def test_guards_hold_the_text_stays_and_the_result_does_not_depend_on_the_poison(case):
    name, raw, min_values = case
    want, n = fc.host_find(raw, min_values)
    twin = fc.blocks_find(raw, min_values)[1]
    cap = 3
    reports = []
    for pattern, lead in zip(A.PATTERNS, (1, 2, 16)):
        ar, v, ws_bytes, whole = _setup(pattern, raw, cap, lead=lead)
        for attempt in range(2):                                       # the second call finds a re-poisoned workspace, output and report
            assert _call(ar, v, raw, min_values, cap, ws_bytes) == 0
            torch.cuda.synchronize()
            ar.check_guards()
            assert v["text"].cpu().numpy().tobytes() == whole, pattern
            rep = _report(v)
            assert rep == twin, (pattern, attempt, rep, twin)
            listed = min(rep["n_found"], cap)
            if name in fc.DECLINE:
                assert rep["status"] == fc.FIND_DECLINED and listed == 0
            else:
                assert rep["status"] == fc.FIND_OK and rep["n_found"] == n and _listed(v, listed) == want[:cap], (pattern, attempt)
            assert ar.is_pattern(v["out"], start=32 * listed), (pattern, attempt)         # nothing behind the entries that exist
            assert ar.is_pattern(v["ws"], start=ws_bytes), (pattern, attempt)              # nor behind the stated workspace
            for key in ("ws", "out", "report"):
                ar.repoison(v[key])
        reports.append(rep)
    assert all(r == reports[0] for r in reports)


@pytest.mark.parametrize("cap", [0, 1, 2, 5])
def test_entries_behind_min_n_found_cap_keep_their_poison(cap):
    raw = b'{"a":[[1,2]],"b":[[3],[4]],"c": [[5]]}'
    want, n = fc.host_find(raw, 1)
    assert n == 3
    for pattern in A.PATTERNS:
        ar, v, ws_bytes, _ = _setup(pattern, raw, max(cap, 1))
        assert _call(ar, v, raw, 1, cap, ws_bytes) == 0
        torch.cuda.synchronize()
        ar.check_guards()
        listed = min(n, cap)
        assert _report(v) == dict(n_found=3, n_candidates=3, status=fc.FIND_OK, first_declined=fc.NO_OFFSET)
        assert _listed(v, listed) == want[:listed] and ar.is_pattern(v["out"], start=32 * listed), (pattern, cap)


@pytest.mark.parametrize("length", [1, 15, 16, 17, G - 1, G, G + 1, 2 * G + 5])
def test_bytes_beside_the_text_are_never_read(length):
    """A `[[` in front would make the text's own `[[1,2]]` rows of a larger matrix or a candidate of its first bracket, a quote in
    front would put the whole text inside a string, and either behind the end would change the last candidate: none is read."""
    body = b"[1,2],[3,4]],[[5,6]] "
    raw = (b"[" + body * (length // len(body) + 1))[:length]
    want, n = fc.host_find(raw, 1, cap=512)
    results = []
    for before, after in ((b"", b""), (b'"[[', b'[["'), (b"[ [", b"]]]"), (b'\\"[', b'1]]'), (b"[[1],", b",[2]]")):
        for lead in (1, 2, 16):
            ar, v, ws_bytes, _ = _setup("zeros", raw, 512, lead=lead, before=before, after=after)
            assert _call(ar, v, raw, 1, 512, ws_bytes, skip=len(before)) == 0
            torch.cuda.synchronize()
            ar.check_guards()
            rep = _report(v)
            assert rep["status"] == fc.FIND_OK and rep["n_found"] == n and _listed(v, n) == want, (before, after, lead, rep)
            results.append(rep)
    assert all(r == results[0] for r in results)


def test_the_call_is_graph_capturable_and_a_replay_reads_new_text():
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    first = b'{"m":[[1,2],[3,4]],"s":"[[5]]","n":[[6]]}' + b" " * (2 * G)
    second = b'{"m":[[1,2],[3,4,5]],"s":"[[5]]" ,"n":[[6]]}'
    second += b" " * (len(first) - len(second))
    text = torch.frombuffer(bytearray(first), dtype=torch.uint8).to(dev)
    out = torch.zeros(4 + 4 * 4, dtype=torch.int64, device=dev)
    ws_bytes = lib.hmm_json_find_matrices_device_workspace_bytes(len(first))
    ws = torch.zeros(ws_bytes // 8, dtype=torch.int64, device=dev)

    def call():
        assert lib.hmm_json_find_matrices_device(text.data_ptr(), len(first), 1, out.data_ptr() + 32, 4, out.data_ptr(), ws.data_ptr(), ws_bytes,
                                                 _lib.stream_ptr()) == 0

    def agrees(raw):
        torch.cuda.synchronize()
        want, n = fc.host_find(raw, 1)
        w = out.cpu().numpy().view(np.uint64)
        return int(w[0]) == n and int(w[2]) == fc.FIND_OK and [tuple(int(x) for x in e) for e in w[4:4 + 4 * n].reshape(-1, 4)] == want

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    assert agrees(first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    out.zero_()
    graph.replay()
    assert agrees(first)
    text.copy_(torch.frombuffer(bytearray(second), dtype=torch.uint8))   # new text of the same length, same graph
    out.zero_()
    graph.replay()
    assert agrees(second) and fc.host_find(second, 1)[1] == 1


def test_bad_arguments_are_refused_with_nothing_written():
    from hippomm_amd import _lib
    raw = b'{"m":[[1,2],[3,4]]}'
    ar, v, ws_bytes, _ = _setup("ones", raw, 2)
    lib = _lib.load()
    good = [ar.address(v["text"]), len(raw), 1, ar.address(v["out"]), 2, ar.address(v["report"]), ar.address(v["ws"]), ws_bytes, _lib.stream_ptr()]

    def call(at, value):
        a = list(good)
        a[at] = value
        return lib.hmm_json_find_matrices_device(*a)
    assert call(7, ws_bytes - 1) == -1 and b"json_find_matrices_device" in lib.hmm_last_error()
    assert call(1, 0) == -1 and call(4, -1) == -1 and call(3, None) == -1 and call(6, good[6] + 4) == -1 and call(5, None) == -1
    torch.cuda.synchronize()
    for key in ("out", "report", "ws"):
        assert ar.is_pattern(v[key]), key
    ar.check_guards()
