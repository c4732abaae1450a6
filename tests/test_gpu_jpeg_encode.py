"""GPU: hippomm_amd.encode_jpeg writes Pillow's file, byte for byte, for every case of tests/jpeg_encode_cases.py -- from numpy
arrays and from CUDA tensors, alone and in batches, at every position of a batch; lengths are exact, nothing behind a file's
last byte is written, a frame whose slot is too small is reported, leaves its neighbours alone and is answered by Pillow;
decode_jpeg reads the files back to Pillow's pixels; save_frame / save_frames write the same bytes; and the quantised blocks
the first kernel leaves in the workspace are the ones the project's host entropy pass reads out of Pillow's file."""
import numpy as np
import pytest
import torch

import jpeg_encode_cases as ec

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    from hippomm_amd import _lib
    return _lib.require_gpu()


def _geometry(case):
    from hippomm_amd import jpeg
    h, w = case.frame.shape[:2]
    return jpeg.encode_geometry(h, w, 1 if case.grey else 3, case.subsampling)


def _as4(frame):
    return frame[None, :, :, None] if frame.ndim == 2 else frame[None]


def _encode_into_filled_slots(cases, dev, stride=None, spare_slots=1):
    """The C call on frames of one geometry with every output byte pre-filled -> (out (n + spare, stride) u8, status (n, 2)) on the host."""
    from hippomm_amd import jpeg
    g = _geometry(cases[0])
    n = len(cases)
    stride = stride or (jpeg.encode_bound(g) + 15) // 16 * 16
    frames = torch.from_numpy(np.concatenate([_as4(c.frame) for c in cases])).to(dev)
    out = torch.full((n + spare_slots, stride), FILL, dtype=torch.uint8, device=dev)
    status = torch.full((n + 1, 2), -7, dtype=torch.int32, device=dev)
    jpeg.encode_device(frames, g, cases[0].quality, cases[0].channel_order, out[:n], status[:n])
    torch.cuda.synchronize()
    assert status[n].tolist() == [-7, -7]
    return out.cpu().numpy(), status[:n].cpu().numpy()


def test_every_case_equals_pillow_from_numpy_and_from_cuda_tensors(dev):
    import hippomm_amd
    for c in ec.cases():
        want = ec.expected(c)
        for source in (c.frame, torch.from_numpy(c.frame).to(dev)):
            stats = {}
            got = hippomm_amd.encode_jpeg(source, c.quality, c.subsampling, c.channel_order, stats=stats)
            assert len(got) == 1 and got[0] == want, (c.name, type(source).__name__, len(got[0]), len(want))
            assert stats == {"device": 1, "host": 0, "overflow": 0}, (c.name, stats)      # the kernels answered, not the fallback


def test_lengths_are_exact_and_no_byte_behind_a_file_is_written(dev):
    from hippomm_amd import jpeg
    for c in ec.cases():
        want = ec.expected(c)
        out, status = _encode_into_filled_slots([c], dev)
        assert status[0].tolist() == [jpeg.ENCODED, len(want)], (c.name, status)
        assert out[0, :len(want)].tobytes() == want, c.name
        assert (out[0, len(want):] == FILL).all() and (out[1] == FILL).all(), c.name


@pytest.mark.parametrize("batch", ec.batches(), ids=["n1", "n3"])
def test_batches_of_different_lengths(dev, batch):
    import hippomm_amd
    from hippomm_amd import jpeg
    want = [ec.expected(c) for c in batch]
    out, status = _encode_into_filled_slots(batch, dev)
    for i, w in enumerate(want):
        assert status[i].tolist() == [jpeg.ENCODED, len(w)] and out[i, :len(w)].tobytes() == w and (out[i, len(w):] == FILL).all()
    stats = {}
    frames = np.stack([c.frame for c in batch])
    assert hippomm_amd.encode_jpeg(frames, batch[0].quality, batch[0].subsampling, stats=stats) == want
    assert hippomm_amd.encode_jpeg(torch.from_numpy(frames).to(dev), batch[0].quality, batch[0].subsampling) == want
    assert stats == {"device": len(batch), "host": 0, "overflow": 0}


def test_a_slot_that_is_too_small_overflows_alone_and_pillow_answers(dev):
    import hippomm_amd
    from hippomm_amd import jpeg
    batch = ec.batches()[1]
    want = [ec.expected(c) for c in batch]
    sizes = sorted(len(w) for w in want)
    stride = (sizes[1] + 15) // 16 * 16                                  # the longest file does not fit, the two others do
    assert sizes[1] <= stride < sizes[2]
    out, status = _encode_into_filled_slots(batch, dev, stride=stride, spare_slots=2)
    for i, w in enumerate(want):
        if len(w) > stride:
            assert status[i].tolist() == [jpeg.ENCODE_OVERFLOW, len(w)]             # the length it would have had
        else:
            assert status[i].tolist() == [jpeg.ENCODED, len(w)] and out[i, :len(w)].tobytes() == w
            assert (out[i, len(w):] == FILL).all()                                  # also when the slot before it overflowed
    assert (out[len(batch):] == FILL).all()
    stats = {}
    frames = np.stack([c.frame for c in batch])
    assert hippomm_amd.encode_jpeg(frames, batch[0].quality, batch[0].subsampling, stats=stats, _slot_bytes=stride) == want
    assert stats == {"device": 2, "host": 1, "overflow": 1}
    before = jpeg.encode_stats()
    hippomm_amd.encode_jpeg(frames[:1], batch[0].quality, batch[0].subsampling, _slot_bytes=16)
    after = jpeg.encode_stats()
    assert after["overflow"] == before["overflow"] + 1 and after["host"] == before["host"] + 1


def test_a_frame_does_not_depend_on_its_position_or_on_the_batch_size(dev):
    import hippomm_amd
    frames = [ec.content(kind, 40, 24, 3, seed=3) for kind in ("noise", "ramp", "checker", "impulse", "blocks")]
    want = [ec.pillow_bytes(f, 95, "4:2:0") for f in frames]
    for n in (1, 2, 5):
        for shift in range(5):
            order = [(shift + k) % 5 for k in range(n)]
            got = hippomm_amd.encode_jpeg(np.stack([frames[i] for i in order]), 95, "4:2:0")
            assert got == [want[i] for i in order], (n, order)


def test_a_list_of_frames_of_different_sizes_and_kinds_keeps_its_order(dev):
    import hippomm_amd
    cases = [c for c in ec.cases() if c.quality == 75 and c.subsampling == "4:2:0" and c.channel_order == "RGB"][:12]
    colour = next(c for c in cases if not c.grey and c.frame.shape[0] > 1)
    pair = np.stack([colour.frame, colour.frame[::-1]])                   # an (n, h, w, 3) array inside the list
    frames = [c.frame if k % 2 else torch.from_numpy(c.frame).to(dev) for k, c in enumerate(cases)] + [cases[0].frame, pair, cases[2].frame]
    stats = {}
    got = hippomm_amd.encode_jpeg(frames, 75, "4:2:0", stats=stats)
    assert got == [ec.expected(c) for c in cases] + [ec.expected(cases[0]), ec.expected(colour),
                                                     ec.pillow_bytes(pair[1], 75, "4:2:0"), ec.expected(cases[2])]
    assert stats == {"device": len(got), "host": 0, "overflow": 0}


def test_decode_of_encode_equals_pillows_decode_of_pillows_encode(dev):
    import hippomm_amd
    from hippomm_amd import jpeg
    for name in ("noise_128x96_q100_444", "noise_216x200_q75_420", "ramp_40x24_q95_422", "noise_17x15_q75_grey", "noise_31x33_q95_420_s1"):
        c = next(x for x in ec.cases() if x.name == name)
        files = hippomm_amd.encode_jpeg(c.frame, c.quality, c.subsampling, c.channel_order)
        pixels = hippomm_amd.decode_jpeg(files)[0].cpu().numpy()
        assert np.array_equal(pixels, jpeg._pillow_rgb(ec.expected(c))), name


def test_save_frame_and_save_frames_write_the_bytes_of_the_call(dev, tmp_path):
    import hippomm_amd
    from hippomm_amd import frame_extraction as seg
    frames = [ec.content(kind, 40, 24, 3, seed=4) for kind in ("noise", "ramp", "impulse")]
    want = hippomm_amd.encode_jpeg(frames, 95, "4:2:0", "BGR")
    assert want == [ec.pillow_bytes(f, 95, "4:2:0", "BGR") for f in frames]
    assert seg.save_frame(frames[0], tmp_path / "a" / "one.jpg") is True
    assert (tmp_path / "a" / "one.jpg").read_bytes() == want[0]
    assert seg.save_frame(torch.from_numpy(frames[1]).to(dev), tmp_path / "a" / "resident.jpg") is True
    assert (tmp_path / "a" / "resident.jpg").read_bytes() == want[1]
    paths = [tmp_path / "b" / f"{k}.jpg" for k in range(3)]
    assert seg.save_frames(frames, paths) == [True, True, True]
    assert [p.read_bytes() for p in paths] == want
    assert seg.save_frames(np.stack(frames), [tmp_path / "c" / f"{k}.jpg" for k in range(3)]) == [True, True, True]
    assert [(tmp_path / "c" / f"{k}.jpg").read_bytes() for k in range(3)] == want


@pytest.mark.parametrize("name", ["noise_16x16_q75_420", "noise_128x96_q100_444", "noise_17x15_q75_grey"])
def test_the_quantised_blocks_are_the_ones_the_host_entropy_pass_reads_from_pillows_file(dev, name):
    """hmm_jpeg_encode leaves the quantised blocks at the start of its workspace (zigzag order, scan order: include/hippomm_hip.h);
    jpeg.decode_coefs of Pillow's file gives the same blocks per component in natural order.  Frames whose sides are whole MCUs,
    or grey: every scan block is a block of the file's component grids."""
    from hippomm_amd import jpeg
    c = next(x for x in ec.cases() if x.name == name)
    g = _geometry(c)
    w, h, comps, hs, vs, _ = g
    data = ec.expected(c)
    slot = np.zeros(jpeg.slot_bytes(g, (0, 0, w, h)), dtype=np.uint8)
    assert jpeg.parse(data)[:5] == g[:5] and jpeg.decode_coefs(data, g, (0, 0, w, h), slot) == jpeg.DECODED
    file_blocks = slot[512:].view(np.int16).reshape(-1, 64)
    frames = torch.from_numpy(_as4(c.frame)).to(dev)
    ws = torch.zeros(jpeg.encode_workspace_bytes(g, 1), dtype=torch.uint8, device=dev)
    out = torch.empty(1, jpeg.encode_bound(g) + 16, dtype=torch.uint8, device=dev)
    jpeg.encode_device(frames, g, c.quality, c.channel_order, out, torch.empty(1, 2, dtype=torch.int32, device=dev), ws)
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    per_mcu = 1 if comps == 1 else hs * vs + 2
    blocks = mcux * mcuy * per_mcu
    kernel = ws[:blocks * 128].cpu().numpy().view(np.int16).reshape(blocks, 64)
    natural = np.empty_like(kernel)
    natural[:, ec.ZIGZAG] = kernel
    luma = mcux * hs * mcuy * vs
    for b in range(blocks):
        mcu, k = divmod(b, per_mcu)
        my, mx = divmod(mcu, mcux)
        if comps == 1 or k < hs * vs:
            at = (my * vs + k // hs) * (mcux * hs) + mx * hs + k % hs
        else:
            at = luma + (k - hs * vs) * mcux * mcuy + my * mcux + mx
        assert np.array_equal(natural[b], file_blocks[at]), (name, b)
