"""GPU: the memory contract of hmm_jpeg_encode in the guarded arena (tests/arena.py).  Frames, tables, output slots, status and
workspace are carved at exactly their size under the three poison patterns: every guard still holds its pattern afterwards, the
inputs are bit-identical, the files are Pillow's under all three (a pixel read behind a frame, a header byte read behind the
tables or a word of the bitstream left unzeroed would differ between two of them), nothing behind a file's last byte is
written, and a second call on a re-poisoned workspace gives the same bytes: no read depends on what an earlier call left there."""
import numpy as np
import pytest
import torch

import arena as A
import jpeg_encode_cases as ec

pytestmark = pytest.mark.gpu

CASES = ["noise_17x15_q75_420", "noise_31x33_q95_420_s1", "noise_216x200_q75_420", "noise_9x7_q75_grey", "noise_24x8_q75_422",
         "noise_40x24_q75_420_bgr"]


def _setup(pattern, cases, n_slots, stride=None):
    from hippomm_amd import _lib, jpeg
    dev = _lib.require_gpu()
    c = cases[0]
    h, w = c.frame.shape[:2]
    g = jpeg.encode_geometry(h, w, 1 if c.grey else 3, c.subsampling)
    head, qt = jpeg.encode_header(g, c.quality)
    tables = np.concatenate([qt.reshape(-1).view(np.uint8), np.frombuffer(head, dtype=np.uint8)])
    frames = np.concatenate([(x.frame[None, :, :, None] if x.grey else x.frame[None]) for x in cases])
    stride = stride or jpeg.encode_bound(g)
    n = len(cases)
    ws_bytes = jpeg.encode_workspace_bytes(g, n)
    ar = A.GuardedArena(A.needed_bytes([frames.nbytes, tables.nbytes, n_slots * stride, n * 8, ws_bytes]), dev, A.PATTERNS[pattern])
    v = dict(frames=ar.put(torch.from_numpy(frames), "frames"), tables=ar.put(torch.from_numpy(tables), "tables", align=16),
             out=ar.carve(n_slots * stride, "out"), status=ar.carve(n * 8, "status", align=16), ws=ar.carve(ws_bytes, "workspace", align=16))
    return ar, v, g, frames, tables, stride


def _call(ar, v, g, c, n, stride, header_bytes):
    from hippomm_amd import _lib, jpeg
    ga = jpeg._geom_array(g)
    st = _lib.load().hmm_jpeg_encode(ar.address(v["frames"]), n, ga.ctypes.data, g[2], jpeg.CHANNEL_ORDER[c.channel_order],
                                     ar.address(v["tables"]), ar.address(v["tables"]) + 256, header_bytes, ar.address(v["out"]), stride,
                                     ar.address(v["status"]), ar.address(v["ws"]), v["ws"].numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("name", CASES)
def test_guards_hold_inputs_stay_and_files_do_not_depend_on_the_poison(name):
    from hippomm_amd import jpeg
    c = next(x for x in ec.cases() if x.name == name)
    want = ec.expected(c)
    for pattern, word in A.PATTERNS.items():
        ar, v, g, frames, tables, stride = _setup(pattern, [c], 1)
        for attempt in range(2):                                       # the second call finds a re-poisoned workspace and output
            assert _call(ar, v, g, c, 1, stride, tables.nbytes - 256) == 0
            ar.check_guards()
            assert torch.equal(v["frames"].cpu(), torch.from_numpy(frames).reshape(-1)), pattern
            assert torch.equal(v["tables"].cpu(), torch.from_numpy(tables)), pattern
            assert v["status"].cpu().numpy().view(np.int32).tolist() == [jpeg.ENCODED, len(want)], (pattern, attempt)
            assert v["out"][:len(want)].cpu().numpy().tobytes() == want, (pattern, attempt)
            assert ar.is_pattern(v["out"], start=len(want)), (pattern, attempt)
            for key in ("ws", "out", "status"):
                ar.repoison(v[key])


def test_a_batch_with_an_overflowing_slot_stays_inside_its_carves():
    from hippomm_amd import jpeg
    batch = ec.batches()[1]
    want = [ec.expected(c) for c in batch]
    sizes = sorted(len(w) for w in want)
    stride = sizes[1] + 1                                              # odd on purpose: slots need no alignment
    for pattern in A.PATTERNS:
        ar, v, g, frames, tables, stride = _setup(pattern, batch, len(batch), stride)
        assert _call(ar, v, g, batch[0], len(batch), stride, tables.nbytes - 256) == 0
        ar.check_guards()
        status = v["status"].cpu().numpy().view(np.int32).reshape(-1, 2)
        for i, w in enumerate(want):
            if len(w) > stride:
                assert status[i].tolist() == [jpeg.ENCODE_OVERFLOW, len(w)]
            else:
                assert status[i].tolist() == [jpeg.ENCODED, len(w)]
                slot = v["out"][i * stride:(i + 1) * stride].cpu().numpy()
                assert slot[:len(w)].tobytes() == w, (pattern, i)
                expected_tail = ar._expected(ar._carve_of(v["out"]).start + i * stride + len(w), ar._carve_of(v["out"]).start + (i + 1) * stride)
                assert torch.equal(v["out"][i * stride + len(w):(i + 1) * stride], expected_tail), (pattern, i)


def test_bad_arguments_are_refused_with_nothing_written():
    from hippomm_amd import _lib
    c = next(x for x in ec.cases() if x.name == CASES[0])
    ar, v, g, frames, tables, stride = _setup("ones", [c], 1)
    assert _call(ar, v, g, c, 1, stride, tables.nbytes - 256 - 1) == -1 and b"jpeg_encode" in _lib.load().hmm_last_error()
    assert _call(ar, v, (g[0], g[1], 3, 1, 2, 0), c, 1, stride, tables.nbytes - 256) == -1
    for key in ("out", "status", "ws"):
        assert ar.is_pattern(v[key]), key
    ar.check_guards()
