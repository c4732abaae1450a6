"""GPU: the memory contract of hmm_json_write_matrix_device in the guarded arena (tests/arena.py).  The matrix, the text buffer
(its full bound), the length word and the workspace are carved at exactly their size under the three poison patterns: every guard
still holds its pattern afterwards, the matrix is bit-identical, the text is json.dumps' under all three (a value read behind the
matrix or a workspace word read before it is written would differ between two of them), nothing behind the text's last byte and
nothing of the workspace behind its stated size is written -- and the call can be captured into a graph and runs on two streams
at once."""
import numpy as np
import pytest
import torch

import arena as A
import event_json_cases as jc

pytestmark = pytest.mark.gpu

G = jc.VALUES_PER_GROUP
# (shape, dtype, close_indent, byte offset of the text inside its carve: the kernel stores whole dwords only where the address allows)
CASES = [((3, 5), np.float32, 4, 0), ((1, 1), np.float64, 0, 1), ((2, G // 2 + 3), np.float32, 7, 3), ((33, 257), np.float64, 4, 2),
         ((1, 2 * G + 1), np.float32, 32, 1)]
SLACK = 64                                                          # bytes of the carve in front of the text: text_offset < SLACK


def _setup(pattern, m, close_indent, extra_ws=0):
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    cap = lib.hmm_json_matrix_text_bound(m.shape[0], m.shape[1], close_indent)
    ws_bytes = lib.hmm_json_write_matrix_device_workspace_bytes(m.shape[0], m.shape[1])
    ar = A.GuardedArena(A.needed_bytes([m.nbytes, SLACK + cap, 8, ws_bytes + extra_ws]), dev, A.PATTERNS[pattern])
    v = dict(m=ar.put(torch.from_numpy(m), "matrix", align=16), out=ar.carve(SLACK + cap, "text"), written=ar.carve(8, "written", align=8),
             ws=ar.carve(ws_bytes + extra_ws, "workspace", align=8))
    return ar, v, cap, ws_bytes


def _call(ar, v, m, close_indent, cap, ws_bytes, text_offset=0, stream=None):
    from hippomm_amd import _lib
    return _lib.load().hmm_json_write_matrix_device(ar.address(v["m"]), 1 if m.dtype == np.float64 else 0, m.shape[0], m.shape[1], close_indent,
                                                    ar.address(v["out"]) + text_offset, cap, ar.address(v["written"]), ar.address(v["ws"]),
                                                    ws_bytes, stream if stream is not None else _lib.stream_ptr())


def _written(v) -> int:
    return int(v["written"].cpu().numpy().view(np.uint64)[0])


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}-indent{c[2]}-at{c[3]}")
def test_guards_hold_inputs_stay_and_the_text_does_not_depend_on_the_poison(case):
    shape, dtype, close_indent, text_offset = case
    m = jc.alternating(shape, dtype)
    m.reshape(-1)[::7] = np.random.default_rng(6).standard_normal(m.reshape(-1)[::7].size).astype(dtype)
    want = jc.matrix_text(m, close_indent)
    for pattern in A.PATTERNS:
        ar, v, cap, ws_bytes = _setup(pattern, m, close_indent, extra_ws=256)
        for attempt in range(2):                                       # the second call finds a re-poisoned workspace and output
            assert _call(ar, v, m, close_indent, cap, ws_bytes, text_offset) == 0
            torch.cuda.synchronize()
            ar.check_guards()
            assert torch.equal(v["m"].cpu(), torch.from_numpy(m).reshape(-1).view(torch.uint8)), pattern
            assert _written(v) == len(want), (pattern, attempt)
            assert v["out"][text_offset:text_offset + len(want)].cpu().numpy().tobytes() == want, (pattern, attempt)
            expected = ar._expected(ar._carve_of(v["out"]).start, ar._carve_of(v["out"]).start + text_offset)
            assert torch.equal(v["out"][:text_offset], expected), (pattern, attempt)                 # nothing in front of the text
            assert ar.is_pattern(v["out"], start=text_offset + len(want)), (pattern, attempt)        # nothing behind *written
            assert ar.is_pattern(v["ws"], start=ws_bytes), (pattern, attempt)                        # nor behind the stated workspace
            for key in ("ws", "out", "written"):
                ar.repoison(v[key])


def test_bad_arguments_are_refused_with_nothing_written():
    from hippomm_amd import _lib
    m = jc.alternating((3, 5), np.float32)
    ar, v, cap, ws_bytes = _setup("ones", m, 4)
    assert _call(ar, v, m, 4, cap - 1, ws_bytes) == -1 and b"json_write_matrix_device" in _lib.load().hmm_last_error()
    assert _call(ar, v, m, 4, cap, ws_bytes - 1) == -1
    assert _call(ar, v, m, 33, cap, ws_bytes) == -1
    torch.cuda.synchronize()
    for key in ("out", "written", "ws"):
        assert ar.is_pattern(v[key]), key
    ar.check_guards()


def test_the_call_is_graph_capturable_and_a_replay_reads_new_values():
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    shape, close_indent = (3, G // 2 + 1), 4
    first, second = jc.alternating(shape, np.float32), np.random.default_rng(8).standard_normal(shape).astype(np.float32)
    m = torch.from_numpy(first).to(dev)
    cap = lib.hmm_json_matrix_text_bound(shape[0], shape[1], close_indent)
    ws_bytes = lib.hmm_json_write_matrix_device_workspace_bytes(*shape)
    out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    ws = torch.zeros(ws_bytes // 8, dtype=torch.int64, device=dev)
    written = torch.zeros(1, dtype=torch.int64, device=dev)

    def call():
        assert lib.hmm_json_write_matrix_device(m.data_ptr(), 0, shape[0], shape[1], close_indent, out.data_ptr(), cap, written.data_ptr(),
                                                ws.data_ptr(), ws_bytes, _lib.stream_ptr()) == 0

    def text():
        torch.cuda.synchronize()
        return out[:int(written.item())].cpu().numpy().tobytes()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    assert text() == jc.matrix_text(first, close_indent)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    out.zero_()
    written.zero_()
    graph.replay()
    assert text() == jc.matrix_text(first, close_indent)
    m.copy_(torch.from_numpy(second))                                # new values of the same shape, same graph
    graph.replay()
    assert text() == jc.matrix_text(second, close_indent)


def test_two_calls_on_two_streams_do_not_disturb_each_other():
    from hippomm_amd import _lib
    lib, dev = _lib.load(), _lib.require_gpu()
    rng = np.random.default_rng(9)
    jobs = []
    for shape, dtype in (((64, 257), np.float32), ((31, 1024), np.float64)):
        a = rng.standard_normal(shape).astype(dtype)
        cap = lib.hmm_json_matrix_text_bound(shape[0], shape[1], 4)
        ws_bytes = lib.hmm_json_write_matrix_device_workspace_bytes(*shape)
        jobs.append(dict(a=a, m=torch.from_numpy(a).to(dev), cap=cap, ws_bytes=ws_bytes, out=torch.zeros(cap, dtype=torch.uint8, device=dev),
                         ws=torch.zeros(ws_bytes // 8, dtype=torch.int64, device=dev), written=torch.zeros(1, dtype=torch.int64, device=dev),
                         stream=torch.cuda.Stream()))
    torch.cuda.synchronize()
    for _ in range(3):                                               # interleaved: each stream has work queued while the other runs
        for j in jobs:
            with torch.cuda.stream(j["stream"]):
                assert lib.hmm_json_write_matrix_device(j["m"].data_ptr(), 1 if j["a"].dtype == np.float64 else 0, j["a"].shape[0],
                                                        j["a"].shape[1], 4, j["out"].data_ptr(), j["cap"], j["written"].data_ptr(),
                                                        j["ws"].data_ptr(), j["ws_bytes"], j["stream"].cuda_stream) == 0
    torch.cuda.synchronize()
    for j in jobs:
        n = int(j["written"].item())
        assert j["out"][:n].cpu().numpy().tobytes() == jc.matrix_text(j["a"], 4)
