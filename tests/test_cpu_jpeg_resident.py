"""CPU: what keeping the decoded pixels of saved frames on the device rests on, pinned against Pillow without a GPU.  The block
lookup of hmm_jpeg_encoded_pixels, restated in numpy (tests/jpeg_resident_cases.py) on the two models the JPEG tests already have
-- the encoder's scan-order blocks and the decoder's pixel half -- gives Pillow's decode of Pillow's file for every case of the
encoder's table, on the full window and on an interior one; every mutant of an index rule is rejected by a named case; the blocks
stay far below the decoder's refusal bound; the two exports refuse bad arguments by name; save_frames keeps save_frame's return
rules with the caches given; and the two caches keep their books (keys, eviction, stale keys) on CPU tensors."""
import ctypes
import logging
import os
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import jpeg_encode_cases as ec
import jpeg_resident_cases as rc
from hippomm_amd import build, jpeg

ROOT = Path(__file__).resolve().parent.parent
NEW = ["hmm_jpeg_encoded_pixels_workspace_bytes", "hmm_jpeg_encoded_pixels"]
HMM_OK, HMM_E_INVALID, HMM_E_WORKSPACE = 0, -1, -2
ONE, FAR = 1 << 20, 1 << 40                                      # aligned non-null dummies: nothing is dereferenced before the checks
COLUMN_BOUND = 5800                                              # jpeg_host.cpp, kColumnBound


def test_reindexed_blocks_reconstruct_to_pillows_pixels_on_full_and_interior_windows():
    pairs = 0
    for c in ec.cases():
        h, w = c.frame.shape[:2]
        want = rc.pillow_decoded(c)
        assert want.shape == (h, w, 3)
        for window in ((0, 0, w, h), rc.interior_window(w, h)):
            if window is None:
                continue
            assert np.array_equal(rc.pixels_from_scan(c, window), rc.cut(want, window)), (c.name, window)
            pairs += 1
    assert pairs > 150


REJECTED_BY = {
    "luma_transposed": "noise_17x15_q75_420",
    "chroma_offset_dropped": "noise_16x16_q75_444",
    "zigzag_kept": "noise_8x8_q75_444",
    "chroma_table0": "noise_40x24_q75_420",
}


@pytest.mark.parametrize("mutant", rc.MUTANTS)
def test_every_mutant_of_an_index_rule_is_rejected_by_a_named_case(mutant):
    case = next(c for c in ec.cases() if c.name == REJECTED_BY[mutant])
    h, w = case.frame.shape[:2]
    assert np.array_equal(rc.pixels_from_scan(case, (0, 0, w, h)), rc.pillow_decoded(case))
    assert not np.array_equal(rc.pixels_from_scan(case, (0, 0, w, h), mutant=mutant), rc.pillow_decoded(case))


def test_every_mutant_of_the_issue_is_listed():
    assert set(REJECTED_BY) == set(rc.MUTANTS) and len(rc.MUTANTS) == 4


def test_the_largest_column_sum_of_the_table_stays_below_the_decoders_bound():
    """No frame from 8-bit input can be refused (include/hippomm_hip.h); the table holds the largest AC coefficients such input
    gives (`extreme`) and the coarsest tables (quality 1)."""
    names = {c.name for c in ec.cases()}
    assert "extreme_16x16_q100_444" in names and any("_q1_" in n for n in names)
    sums = {c.name: rc.max_column_sum(c) for c in ec.cases()}
    worst = max(sums, key=sums.get)
    print("largest column sum", sums[worst], "in", worst)
    assert sums[worst] < COLUMN_BOUND, (worst, sums[worst])


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(build.build()))
    for name in NEW:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _lib._SIGNATURES, name
    assert _lib.load().hmm_abi_version() == 7


def test_workspace_query_and_argument_errors_are_reported_without_a_gpu():
    from hippomm_amd import _lib
    build.build()
    lib = _lib.load()
    query, call, name = lib.hmm_jpeg_encoded_pixels_workspace_bytes, lib.hmm_jpeg_encoded_pixels, b"jpeg_encoded_pixels"
    g = jpeg._geom_array((40, 24, 3, 2, 2, 0))
    gp = g.ctypes.data
    # the u8 planes of the stored rectangles: luma 5 x 3 blocks, chroma 3 x 2 each, 64 bytes a block, 3 frames
    assert query(gp, 3, 0, 0, 40, 24) == 3 * (15 + 6 + 6) * 64 + (-3 * 27 * 64) % 256
    assert query(gp, 3, 0, 0, 40, 24) == lib.hmm_jpeg_workspace_bytes(gp, 3, 0, 0, 40, 24)
    assert query(gp, 1, 9, 9, 1, 1) == 256                       # one luma block and one of each chroma: 192 bytes, rounded up
    assert query(gp, 0, 0, 0, 40, 24) == 0 and query(None, 1, 0, 0, 40, 24) == 0 and query(gp, 1, 0, 0, 41, 24) == 0
    assert query(jpeg._geom_array((40, 24, 3, 1, 2)).ctypes.data, 1, 0, 0, 40, 24) == 0      # a sampling the encoder does not take
    ws = query(gp, 3, 1, 1, 38, 22)

    def refused(*args, say, code=HMM_E_INVALID):
        assert call(*args) == code, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg

    #    encode_workspace, n, geometry, qtables, x0, y0, w, h, rgb_out, workspace, workspace_bytes, stream
    ptrs = (ONE, 2 * ONE, FAR, 2 * FAR)                                      # encode workspace, qtables, rgb out, workspace
    for missing in range(4):
        p = [None if i == missing else v for i, v in enumerate(ptrs)]
        refused(p[0], 3, gp, p[1], 1, 1, 38, 22, p[2], p[3], ws, None, say=b"null pointer")
    enc, q, out, wk = ptrs
    refused(enc, 3, None, q, 1, 1, 38, 22, out, wk, ws, None, say=b"null pointer")
    refused(enc, -1, gp, q, 1, 1, 38, 22, out, wk, ws, None, say=b"negative")
    for bad in ((0, 24, 3, 2, 2), (40, 70000, 3, 2, 2), (40, 24, 2, 1, 1), (40, 24, 3, 1, 2), (65535, 65535, 3, 1, 1)):
        refused(enc, 3, jpeg._geom_array(bad).ctypes.data, q, 0, 0, 1, 1, out, wk, ws, None, say=b"bad geometry")
    for window in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (33, 0, 8, 8), (0, 17, 8, 8), (0, 0, 41, 24)):
        refused(enc, 3, gp, q, *window, out, wk, ws, None, say=b"bad window")
    refused(enc + 8, 3, gp, q, 1, 1, 38, 22, out, wk, ws, None, say=b"aligned")
    refused(enc, 3, gp, q + 1, 1, 1, 38, 22, out, wk, ws, None, say=b"aligned")
    refused(enc, 3, gp, q, 1, 1, 38, 22, out + 2, wk, ws, None, say=b"aligned")
    refused(enc, 3, gp, q, 1, 1, 38, 22, out, wk + 8, ws, None, say=b"aligned")
    refused(enc, 3, gp, q, 1, 1, 38, 22, out, wk, ws - 1, None, say=b"workspace", code=HMM_E_WORKSPACE)
    assert call(enc, 0, gp, q, 1, 1, 38, 22, out, wk, 0, None) == HMM_OK      # no frames: no launch (there is no GPU here)


# ---- save_frames with the caches, the encoder stubbed by Pillow ---------------------------------------------------------------
def _cpu_gray_into(frames, order, gray, minmax):
    """hmm_gray_u8 on CPU tensors: OpenCV's 8-bit rule on RGB (order 0) frames."""
    assert order == 0
    f = frames.to(torch.int32)
    g = ((4899 * f[..., 0] + 9617 * f[..., 1] + 1868 * f[..., 2] + 8192) >> 14).to(torch.uint8)
    gray.copy_(g)
    minmax[:, 0] = g.reshape(len(g), -1).min(dim=1).values.to(torch.int32)
    minmax[:, 1] = g.reshape(len(g), -1).max(dim=1).values.to(torch.int32)


def _pillow_stub(calls):
    from hippomm_amd import segmentation as seg

    def stub(frames, return_decoded=False, window=None):
        frames = list(frames) if isinstance(frames, list) else [frames]
        calls.append((len(frames), return_decoded, window))
        files = [jpeg.pillow_encode(f, seg.SAVE_QUALITY, seg.SAVE_SUBSAMPLING, "BGR") for f in frames]
        if not return_decoded:
            return files
        decoded = [torch.from_numpy(np.array(jpeg._pillow_rgb(data))) for data in files]
        if window is not None:
            x0, y0, w, h = window
            decoded = [d[y0:y0 + h, x0:x0 + w] for d in decoded]
        return files, decoded
    return stub


@pytest.fixture
def on_cpu(monkeypatch):
    """The two kernels the caches launch, replaced by CPU stand-ins: the bookkeeping is what these tests are about."""
    from hippomm_amd import preprocess as pp, ssim
    monkeypatch.setattr(ssim, "gray_into", _cpu_gray_into)
    seen = []

    def preprocess_into(frames, out, full_hw=None):
        seen.append((tuple(frames.shape), full_hw))
        out.copy_(frames.float().mean(dim=(1, 2, 3))[:, None, None, None].expand_as(out))
        return out
    monkeypatch.setattr(pp, "_preprocess_into", preprocess_into)
    return seen


def test_save_frames_with_the_caches_keeps_the_return_rules_and_puts_only_what_it_wrote(tmp_path, monkeypatch, caplog, on_cpu):
    from hippomm_amd import frame_extraction as seg, preprocess as pp    # the module that looks _encode_bgr up, and its logger
    calls = []
    monkeypatch.setattr(seg, "_encode_bgr", _pillow_stub(calls))
    frames = [ec.content(k, 40, 24, 3) for k in ("noise", "ramp", "mid")] + [None]
    paths = [tmp_path / "batch" / f"{k}.jpg" for k in range(4)]
    paths[1].parent.mkdir()
    paths[1].write_bytes(b"kept")
    cache, tower = seg.FrameCache(), pp.TowerInputCache()
    with caplog.at_level(logging.ERROR, logger=seg.__name__):
        assert seg.save_frames(frames, paths, cache=cache, tower_inputs=tower) == [True, True, True, False]
    assert calls == [(2, True, None)]                                        # one encode call for the two new files, whole frames
    assert sum("Invalid frame data" in r.message for r in caplog.records) == 1
    assert paths[1].read_bytes() == b"kept" and paths[0].read_bytes() == ec.pillow_bytes(frames[0], 95, "4:2:0", "BGR")
    assert cache.lookup(str(paths[0])) is not None and cache.lookup(str(paths[2])) is not None
    assert cache.lookup(str(paths[1])) is None and tower.get(str(paths[1])) is None       # that file was not ours
    assert cache.decodes == 0 and len(tower) == 2
    slab, slot = cache.lookup(str(paths[0]))
    rgb = jpeg._pillow_rgb(paths[0].read_bytes()).astype(np.int32)           # the gray rule ran on RGB order, as load runs it
    want = ((4899 * rgb[..., 0] + 9617 * rgb[..., 1] + 1868 * rgb[..., 2] + 8192) >> 14).astype(np.uint8)
    assert np.array_equal(slab.gray[slot].numpy(), want)
    assert slab.minmax[slot].tolist() == [int(want.min()), int(want.max())]
    x0, y0, ww, wh = pp.needed_window(24, 40)                                # the tower got the window of the whole frame
    assert on_cpu == [((2, wh, ww, 3), (24, 40))]

    # only the tower asks: the encoder is asked for the needed window alone
    calls.clear()
    on_cpu.clear()
    only = pp.TowerInputCache()
    path = tmp_path / "single" / "frame.jpg"
    assert seg.save_frame(frames[0], path, tower_inputs=only) is True
    assert calls == [(1, True, (x0, y0, ww, wh))] and on_cpu == [((1, wh, ww, 3), (24, 40))] and only.get(path) is not None
    assert seg.save_frame(frames[1], path, cache=cache, tower_inputs=only) is True and len(calls) == 1    # exists: untouched
    with caplog.at_level(logging.ERROR, logger=seg.__name__):
        assert seg.save_frame(None, tmp_path / "none.jpg", cache=cache) is False
        blocker = tmp_path / "file_not_folder"
        blocker.write_bytes(b"x")
        assert seg.save_frame(frames[0], blocker / "frame.jpg", cache=cache) is False
        monkeypatch.setattr(seg, "_encode_bgr", lambda frames, **kw: (_ for _ in ()).throw(RuntimeError("encoder down")))
        assert seg.save_frame(frames[0], tmp_path / "error.jpg", cache=cache) is False
        assert seg.save_frames(frames[:1], [tmp_path / "error2.jpg"], tower_inputs=only) == [False]
    assert any("encoder down" in r.message for r in caplog.records)
    assert not (tmp_path / "none.jpg").exists() and not (tmp_path / "error.jpg").exists()
    with pytest.raises(ValueError):
        seg.save_frames(frames, paths[:2], cache=cache)

    # a failure while a cache is filled is logged; the file is there, so the answer stays True
    monkeypatch.setattr(seg, "_encode_bgr", _pillow_stub(calls))
    monkeypatch.setattr(cache, "put", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("cache down")))
    with caplog.at_level(logging.ERROR, logger=seg.__name__):
        assert seg.save_frames(frames[:1], [tmp_path / "late.jpg"], cache=cache) == [True]
    assert any("cache down" in r.message for r in caplog.records)


def _write(path, payload: bytes, mtime_ns=None):
    path.write_bytes(payload)
    if mtime_ns is not None:
        os.utime(path, ns=(mtime_ns, mtime_ns))


def test_frame_cache_put_keys_eviction_and_stale_keys(tmp_path, on_cpu):
    from hippomm_amd import segmentation as seg
    h, w = 8, 16
    cache = seg.FrameCache(cache_bytes=4 * h * w)                             # four slots of this size
    rng = np.random.default_rng(3)
    paths = [tmp_path / f"{k}.jpg" for k in range(6)]
    frames = torch.from_numpy(rng.integers(0, 256, (6, h, w, 3), dtype=np.uint8))
    for p in paths:
        _write(p, b"file " + p.name.encode())
    cache.put(str(paths[0]), frames[0])
    assert cache.lookup(str(paths[0])) is not None and cache.lookup(paths[0]) is not None      # str and Path are one key
    slab, slot = cache.lookup(str(paths[0]))
    assert (slab.h, slab.w, slab.capacity) == (h, w, 4) and cache.decodes == 0
    cache.put([str(p) for p in paths[1:4]], frames[1:4])                      # full now; 0 is the least recently used ...
    assert all(cache.lookup(str(p)) is not None for p in paths[:4])
    cache.lookup(str(paths[0]))                                               # ... until it is looked up
    cache.put(str(paths[4]), frames[4])
    assert cache.lookup(str(paths[1])) is None and cache.lookup(str(paths[0])) is not None     # 1 left, 0 stayed
    cache.put(str(paths[4]), frames[5])                                       # the same file again: one slot, the new pixels
    assert sum(len(s.slots) for s in cache.slabs.values()) == 4
    slab, slot = cache.lookup(str(paths[4]))
    gray = torch.empty(1, h, w, dtype=torch.uint8)
    _cpu_gray_into(frames[5:6], 0, gray, torch.empty(1, 2, dtype=torch.int32))
    assert torch.equal(slab.gray[slot], gray[0])
    # a file rewritten since (another size, or only another mtime) is a miss
    _write(paths[0], b"file 0.jpg, longer now")
    assert cache.lookup(str(paths[0])) is None
    st = os.stat(paths[2])
    _write(paths[2], b"file 2.jpg", st.st_mtime_ns + 1_000_000_000)
    assert os.stat(paths[2]).st_size == st.st_size and cache.lookup(str(paths[2])) is None
    assert cache.lookup(str(tmp_path / "missing.jpg")) is None
    with pytest.raises(OSError):
        cache.put(str(tmp_path / "missing.jpg"), frames[0])                   # only files that exist have a key
    with pytest.raises(ValueError):
        cache.put(str(paths[3]), frames[0].float())
    # more frames in one call than the budget holds: every one of them is kept
    cache.put([str(p) for p in paths], frames)
    assert all(cache.lookup(str(p)) is not None for p in paths)


def test_tower_input_cache_keys_lru_by_bytes_and_stale_keys(tmp_path, on_cpu):
    from hippomm_amd import preprocess as pp
    assert pp.TOWER_INPUT_BYTES == 3 * 224 * 224 * 4 and pp.TowerInputCache().cache_bytes == 4 << 30
    cache = pp.TowerInputCache(cache_bytes=3 * pp.TOWER_INPUT_BYTES)
    paths = [tmp_path / f"{k}.jpg" for k in range(5)]
    for p in paths:
        _write(p, b"file " + p.name.encode())
    rows = torch.arange(5, dtype=torch.float32)[:, None, None, None].expand(5, 3, 224, 224)
    for k in range(3):
        cache.put(str(paths[k]), rows[k])
    assert len(cache) == 3 and cache.bytes == 3 * pp.TOWER_INPUT_BYTES
    assert torch.equal(cache.get(paths[0]), rows[0])                          # str and Path are one key; 0 is the most recent now
    cache.put(str(paths[3]), rows[3])
    assert cache.get(str(paths[1])) is None and cache.get(str(paths[0])) is not None and len(cache) == 3
    assert cache.bytes == 3 * pp.TOWER_INPUT_BYTES
    cache.put(str(paths[3]), rows[4])                                         # the same file again: one entry, the new row
    assert len(cache) == 3 and torch.equal(cache.get(str(paths[3])), rows[4])
    _write(paths[0], b"file 0.jpg rewritten")
    assert cache.get(str(paths[0])) is None                                   # stale: a miss
    cache.put(str(paths[0]), rows[1])                                         # put again under the new key: the stale entry leaves
    assert len(cache) == 3 and torch.equal(cache.get(str(paths[0])), rows[1])
    assert cache.get(str(tmp_path / "missing.jpg")) is None
    hits, misses = cache.hits, cache.misses
    cache.get(str(paths[0]))
    cache.get(str(tmp_path / "missing.jpg"))
    assert (cache.hits, cache.misses) == (hits + 1, misses + 1)
    with pytest.raises(ValueError):
        cache.put(str(paths[0]), torch.zeros(3, 8, 8))
    # put_frames: one preprocess launch for the batch, one entry per path
    big = pp.TowerInputCache()
    big.put_frames([str(p) for p in paths[:2]], torch.full((2, 9, 11, 3), 7, dtype=torch.uint8), (24, 40))
    assert on_cpu[-1] == ((2, 9, 11, 3), (24, 40)) and len(big) == 2 and float(big.get(str(paths[1]))[0, 0, 0]) == 7.0
    with pytest.raises(ValueError):
        big.put_frames([str(paths[0])], torch.zeros(2, 9, 11, 3, dtype=torch.uint8))


def test_forward_ranges_never_leave_a_lone_frame():
    from hippomm_amd.encoder import _forward_ranges
    assert _forward_ranges(1, 256) == [(0, 1)] and _forward_ranges(5, 256) == [(0, 5)] and _forward_ranges(0, 256) == []
    assert _forward_ranges(257, 256) == [(0, 255), (255, 257)] and _forward_ranges(512, 256) == [(0, 256), (256, 512)]
    for n in range(2, 40):
        for step in (1, 2, 3, 4, 7):
            ranges = _forward_ranges(n, step)
            assert ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            assert all(2 <= hi - lo <= max(step, 3) for lo, hi in ranges), (n, step, ranges)
