"""GPU: the device entropy pass (hmm_jpeg_decode_coefs_device) writes the coefficient slots of the host pass
(hmm_jpeg_decode_coefs), byte for byte: on a corpus every frame of which the device must decode ITSELF (a fallback cannot hide a
failure), in batches, on the seeded damage sweep (status parity, and slot parity where decoded), and inside the guarded,
poisoned arena of the memory-contract tests."""
import numpy as np
import pytest
import torch

import arena as A
import jpeg_entropy_corpus as jc
from hippomm_amd import _lib, jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def device_pass(files, geometry, window):
    """files of one geometry -> (status (n, 2) int32, slots (n, slot_bytes) u8), both numpy; every file must pass the prepare pass."""
    prepared = [jc.prepare(d, geometry) for d in files]
    assert all(st == jpeg.DECODED for st, _ in prepared)
    stride = max(s.nbytes for _, s in prepared)
    bits = np.zeros((len(files), stride), dtype=np.uint8)
    for k, (_, s) in enumerate(prepared):
        bits[k, :s.nbytes] = s
    sb = jpeg.slot_bytes(geometry, window)
    slots = torch.full((len(files), sb), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((len(files), 2), -7, dtype=torch.int32, device=DEV)
    jpeg.decode_coefs_device(torch.from_numpy(bits).to(DEV), geometry, window, slots, status)
    torch.cuda.synchronize()
    return status.cpu().numpy(), slots.cpu().numpy()


@pytest.mark.parametrize("name", [name for name, _ in jc.corpus()])
def test_slots_equal_the_host_pass_and_no_frame_is_left_to_the_host(name):
    data = dict(jc.corpus())[name]
    g = jpeg.parse(data)
    for window in jc.windows(g):
        st, want = jc.host_slot(data, g, window)
        assert st == jpeg.DECODED
        status, got = device_pass([data], g, window)
        print(name, window, "status", status[0, 0], "rounds", status[0, 1])
        assert status[0, 0] == jpeg.DECODED, (name, window)
        np.testing.assert_array_equal(got[0], want, err_msg=f"{name} {window}")
        if name.startswith("noise_q95"):
            assert status[0, 1] >= 2, status                              # the fixed point, not only the first guess


def test_batch_of_different_lengths_in_two_orders_equals_single_calls():
    from test_cpu_jpeg import encode, frame
    files = [encode(frame(72, 40, seed=s), quality=q, subsampling=2, optimize=opt)
             for s, q, opt in ((1, 30, False), (2, 95, True), (3, 75, False), (4, 100, False), (5, 5, True))]
    assert len({len(f) for f in files}) == 5
    g = jpeg.parse(files[0])
    window = (3, 5, 60, 30)
    single = [device_pass([f], g, window) for f in files]
    for order in ((0, 1, 2, 3, 4), (3, 0, 4, 2, 1)):
        status, slots = device_pass([files[k] for k in order], g, window)
        for row, k in enumerate(order):
            assert status[row, 0] == jpeg.DECODED
            assert tuple(status[row]) == tuple(single[k][0][0])
            np.testing.assert_array_equal(slots[row], single[k][1][0])
            np.testing.assert_array_equal(slots[row], jc.host_slot(files[k], g, window)[1])


def test_more_frames_than_one_launch_takes():
    """40 frames: the call runs them in chunks of 32 through one workspace."""
    data = [d for n, d in jc.corpus() if n in ("noise_q95_256x144", "noise_q95_256x144_opt")]
    g = jpeg.parse(data[0])
    window = (0, 0, g[0], g[1])
    status, slots = device_pass([data[k % 2] for k in range(40)], g, window)
    want = [jc.host_slot(d, g, window)[1] for d in data]
    assert (status[:, 0] == jpeg.DECODED).all()
    for k in range(40):
        np.testing.assert_array_equal(slots[k], want[k % 2])


def test_damage_sweep_has_the_host_status_and_the_host_slots():
    """Parity on files that were not written to fault: every case of the CPU sweep that the prepare pass takes, thinned to at
    most 200; the device status is the host's, and where it is DECODED the slot is the host's."""
    taken = [(g, d) for g, d in jc.damage_sweep() if jc.prepare(d, g)[0] == jpeg.DECODED]
    taken = taken[::len(taken) // 200 + 1]
    assert 100 < len(taken) <= 200
    decoded = 0
    for g in sorted({g for g, _ in taken}):
        files = [d for gg, d in taken if gg == g]
        window = (0, 0, g[0], g[1])
        status, slots = device_pass(files, g, window)
        for k, d in enumerate(files):
            st, want = jc.host_slot(d, g, window)
            assert status[k, 0] == st, (g, k)
            if st == jpeg.DECODED:
                decoded += 1
                np.testing.assert_array_equal(slots[k], want)
    assert 0 < decoded < len(taken)


def _arena_run(pattern, files, g, window, first=None):
    """One call inside the arena -> (status, slots) as numpy.  first: (files, geometry, window) of a call that uses the same
    workspace before."""
    lib = _lib.load()
    prepared = [jc.prepare(d, g)[1] for d in files]
    stride = max(s.nbytes for s in prepared)
    bits = np.zeros((len(files), stride), dtype=np.uint8)
    for k, s in enumerate(prepared):
        bits[k, :s.nbytes] = s
    sb = jpeg.slot_bytes(g, window)
    ga = jpeg._geom_array(g)
    ws_bytes = lib.hmm_jpeg_entropy_workspace_bytes(ga.ctypes.data, len(files), stride)
    sizes = [bits.nbytes, sb * len(files), 8 * len(files), ws_bytes]
    if first is not None:
        f_files, f_g, f_window = first
        f_prepared = [jc.prepare(d, f_g)[1] for d in f_files]
        f_stride = max(s.nbytes for s in f_prepared)
        f_bits = np.zeros((len(f_files), f_stride), dtype=np.uint8)
        for k, s in enumerate(f_prepared):
            f_bits[k, :s.nbytes] = s
        f_sb = jpeg.slot_bytes(f_g, f_window)
        f_ga = jpeg._geom_array(f_g)
        f_ws = lib.hmm_jpeg_entropy_workspace_bytes(f_ga.ctypes.data, len(f_files), f_stride)
        sizes += [f_bits.nbytes, f_sb * len(f_files), 8 * len(f_files), f_ws]
    ar = A.GuardedArena(A.needed_bytes(sizes), DEV, A.PATTERNS[pattern])
    ws = ar.carve(ws_bytes if first is None else max(ws_bytes, f_ws), "workspace", align=16)
    if first is not None:
        fb = ar.put(torch.from_numpy(f_bits), "first bitslots")
        fs = ar.carve(f_sb * len(f_files), "first slots")
        fst = ar.carve(8 * len(f_files), "first status")
        _lib.check(lib.hmm_jpeg_decode_coefs_device(ar.address(fb), len(f_files), f_stride, f_ga.ctypes.data, *f_window, ar.address(fs),
                                                    f_sb, ar.address(fst), ar.address(ws), f_ws, _lib.stream_ptr()), "first call")
    b = ar.put(torch.from_numpy(bits), "bitslots")
    slots = ar.carve(sb * len(files), "slots")
    status = ar.carve(8 * len(files), "status")
    _lib.check(lib.hmm_jpeg_decode_coefs_device(ar.address(b), len(files), stride, ga.ctypes.data, *window, ar.address(slots), sb,
                                                ar.address(status), ar.address(ws), ws_bytes, _lib.stream_ptr()), "call")
    torch.cuda.synchronize()
    ar.check_guards()                                                       # nothing past slot_bytes, the status words, the workspace
    return status.cpu().numpy().view(np.int32).reshape(-1, 2), slots.cpu().numpy().reshape(len(files), sb)


@pytest.mark.parametrize("case", ["small", "multi"])
def test_memory_contract_in_the_guarded_arena(case):
    corpus = dict(jc.corpus())
    files = [corpus["420_16x16"]] if case == "small" else [corpus["noise_q95_256x144"], corpus["noise_q95_256x144_opt"]]
    g = jpeg.parse(files[0])
    window = (0, 0, g[0], g[1]) if case == "small" else (g[0] // 2, g[1] // 2, g[0] - g[0] // 2, g[1] - g[1] // 2)
    want = [jc.host_slot(d, g, window)[1] for d in files]
    other = ([corpus["444_40x24"]], jpeg.parse(corpus["444_40x24"]), (0, 0, 40, 24))
    runs = [_arena_run(p, files, g, window) for p in A.PATTERNS]
    runs.append(_arena_run("ones", files, g, window, first=other))          # after another geometry used the workspace
    for status, slots in runs:
        assert (status[:, 0] == jpeg.DECODED).all()
        np.testing.assert_array_equal(status, runs[0][0])
        for k in range(len(files)):
            np.testing.assert_array_equal(slots[k], want[k])
