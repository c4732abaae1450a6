"""GPU: the memory contract of hmm_jpeg_encoded_pixels in the guarded arena (tests/arena.py).  Three 17 x 15 frames at 4:2:0 are
encoded inside the arena; the encoder's workspace, the tables, the output and the pixel workspace are carved at exactly their
size under the three poison patterns.  After the call on an interior window every guard still holds its pattern, the encoder's
workspace and the tables are byte-identical to what they were, and the pixels are the same under all three patterns -- a block
read beside the encoder's coefficients, a table entry read behind the tables or a sample plane read before it was written would
differ between two of them -- and they are Pillow's."""
import numpy as np
import pytest
import torch

import arena as A
import jpeg_encode_cases as ec
import jpeg_resident_cases as rc

pytestmark = pytest.mark.gpu

N = 3
WINDOW = (3, 1, 11, 13)                                              # interior, odd start: the chroma halo on every side is read
KINDS = ("noise", "ramp", "checker")


def _cases():
    return [ec._case(kind, 17, 15, 75, "4:2:0") for kind in KINDS]


def _run(pattern):
    from hippomm_amd import _lib, jpeg
    dev = _lib.require_gpu()
    lib = _lib.load()
    cases = _cases()
    g = jpeg.encode_geometry(15, 17, 3, "4:2:0")
    ga = jpeg._geom_array(g)
    head, qt = jpeg.encode_header(g, 75)
    tables = np.concatenate([qt.reshape(-1).view(np.uint8), np.frombuffer(head, dtype=np.uint8)])
    frames = np.stack([c.frame for c in cases])
    stride = jpeg.encode_bound(g)
    enc_bytes = jpeg.encode_workspace_bytes(g, N)
    x0, y0, w, h = WINDOW
    out_bytes = N * h * w * 3
    ws_bytes = lib.hmm_jpeg_encoded_pixels_workspace_bytes(ga.ctypes.data, N, x0, y0, w, h)
    assert ws_bytes > 0
    ar = A.GuardedArena(A.needed_bytes([frames.nbytes, tables.nbytes, 256, N * stride, N * 8, enc_bytes, out_bytes, ws_bytes]), dev,
                        A.PATTERNS[pattern])
    v = dict(frames=ar.put(torch.from_numpy(frames), "frames"), tables=ar.put(torch.from_numpy(tables), "tables", align=16),
             qtables=ar.put(torch.from_numpy(tables[:256].copy()), "qtables", align=16),       # exactly the two tables, poison behind
             files=ar.carve(N * stride, "files"), status=ar.carve(N * 8, "status", align=16),
             enc=ar.carve(enc_bytes, "encode workspace", align=16), out=ar.carve(out_bytes, "rgb", align=16),
             ws=ar.carve(ws_bytes, "workspace", align=16))
    st = lib.hmm_jpeg_encode(ar.address(v["frames"]), N, ga.ctypes.data, 3, jpeg.CHANNEL_ORDER["RGB"], ar.address(v["tables"]),
                             ar.address(v["tables"]) + 256, tables.nbytes - 256, ar.address(v["files"]), stride, ar.address(v["status"]),
                             ar.address(v["enc"]), enc_bytes, _lib.stream_ptr())
    assert st == 0
    torch.cuda.synchronize()
    status = v["status"].cpu().numpy().view(np.int32).reshape(N, 2)
    for i, c in enumerate(cases):                                    # the blocks in the workspace are those of Pillow's files
        assert status[i].tolist() == [jpeg.ENCODED, len(ec.expected(c))]
    enc_before, q_before = v["enc"].clone(), v["qtables"].clone()
    results = []
    for attempt in range(2):                                         # the second call finds a re-poisoned workspace and output
        st = lib.hmm_jpeg_encoded_pixels(ar.address(v["enc"]), N, ga.ctypes.data, ar.address(v["qtables"]), x0, y0, w, h,
                                         ar.address(v["out"]), ar.address(v["ws"]), ws_bytes, _lib.stream_ptr())
        assert st == 0, lib.hmm_last_error()
        torch.cuda.synchronize()
        ar.check_guards()
        assert torch.equal(v["enc"], enc_before) and torch.equal(v["qtables"], q_before), (pattern, attempt)
        assert torch.equal(v["frames"].cpu(), torch.from_numpy(frames).reshape(-1))
        results.append(v["out"].cpu().numpy().reshape(N, h, w, 3).copy())
        ar.repoison(v["out"])
        ar.repoison(v["ws"])
    assert np.array_equal(results[0], results[1]), pattern
    return ar, v, results[0], (lib, ga, ws_bytes)


def test_guards_hold_inputs_stay_and_pixels_do_not_depend_on_the_poison():
    outs = {}
    for pattern in A.PATTERNS:
        outs[pattern] = _run(pattern)[2]
    first = outs["ones"]
    for pattern, got in outs.items():
        assert np.array_equal(got, first), pattern
    for i, c in enumerate(_cases()):
        assert np.array_equal(first[i], rc.cut(rc.pillow_decoded(c), WINDOW)), c.name


def test_bad_arguments_are_refused_with_nothing_written():
    ar, v, _, (lib, ga, ws_bytes) = _run("big")
    from hippomm_amd import _lib
    x0, y0, w, h = WINDOW
    args = lambda **kw: (ar.address(v["enc"]), N, ga.ctypes.data, ar.address(v["qtables"]), kw.get("x0", x0), y0, w, h,
                         ar.address(v["out"]), ar.address(v["ws"]), kw.get("ws", ws_bytes), _lib.stream_ptr())
    assert lib.hmm_jpeg_encoded_pixels(*args(x0=7)) == -1 and b"jpeg_encoded_pixels" in lib.hmm_last_error()    # 7 + 11 > 17
    assert lib.hmm_jpeg_encoded_pixels(*args(ws=ws_bytes - 1)) == -2
    torch.cuda.synchronize()
    assert ar.is_pattern(v["out"]) and ar.is_pattern(v["ws"])        # _run left both re-poisoned
    ar.check_guards()
