"""CPU: everything the GPU JPEG encoder rests on, pinned against Pillow without a GPU.  The kernels' per-thread functions
(hippomm_amd/csrc/jpeg_encode_core.h), run thread by thread by the stand-alone program tools/jpeg_encode_model.cpp under
AddressSanitizer and UBSan, give Pillow's file byte for byte on every case of tests/jpeg_encode_cases.py; so does the numpy stage
model; hmm_jpeg_encode_header gives Pillow's header.  A census taken from the model proves the table contains the entropy coder's
edge cases, every mutant of the stage model is rejected by a named case, the C ABI refuses bad arguments by name, and
save_frame's return rules hold with the encoder stubbed by Pillow.  The program is built here from source with the host compiler
of hipcc; nothing of it is loaded into this interpreter."""
import ctypes
import logging
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import jpeg_encode_cases as ec
from hippomm_amd import build, jpeg

ROOT = Path(__file__).resolve().parent.parent
NEW = ["hmm_jpeg_encode_header", "hmm_jpeg_encode_workspace_bytes", "hmm_jpeg_encode_bound", "hmm_jpeg_encode"]
HMM_OK, HMM_E_INVALID, HMM_E_WORKSPACE = 0, -1, -2
ONE, FAR = 1 << 20, 1 << 40                                      # aligned non-null dummies: nothing is dereferenced before the checks


def _geometry(case):
    h, w = case.frame.shape[:2]
    return jpeg.encode_geometry(h, w, 1 if case.grey else 3, case.subsampling)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    build.build()
    exe = tmp_path_factory.mktemp("encode_model") / "jpeg_encode_model"
    cmd = [build._hipcc(), "-O1", "-g", "-std=c++17", "-x", "hip", f"--offload-arch={build.ARCH}", "-I", str(ROOT / "include"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           str(ROOT / "tools" / "jpeg_encode_model.cpp"), str(build.CSRC / "jpeg_encode_host.cpp"), "-fsanitize=address,undefined",
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def _run(model, folder, cases, strides=None):
    """-> per case: (the file the program wrote or None, its report line as a dict of ints)."""
    lines = []
    for k, c in enumerate(cases):
        (folder / f"{k}.raw").write_bytes(np.ascontiguousarray(c.frame).tobytes())
        w, h, comps, hs, vs, _ = _geometry(c)
        stride = strides[k] if strides else 0
        lines.append(f"{folder}/{k}.raw {folder}/{k}.jpg {w} {h} {comps} {int(c.channel_order == 'BGR')} {hs} {vs} {c.quality} {stride}")
    manifest = folder / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(model), str(manifest)], capture_output=True, text=True, timeout=600)
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert r.returncode == 0, report[-4000:]
    out = r.stdout.splitlines()
    assert out[-1] == f"cases={len(cases)}", out[-1]
    results = []
    for k in range(len(cases)):
        path = folder / f"{k}.jpg"
        results.append((path.read_bytes() if path.exists() else None, {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", out[k])}))
    return results


@pytest.fixture(scope="module")
def modelled(model, tmp_path_factory):
    """The model's file and census for every case of the table, computed once."""
    cases = ec.cases() + [c for batch in ec.batches() for c in batch]
    return cases, _run(model, tmp_path_factory.mktemp("encode_cases"), cases)


def test_the_model_writes_pillows_file_for_every_case(modelled):
    cases, results = modelled
    assert len(cases) > 100
    for c, (data, report) in zip(cases, results):
        want = ec.expected(c)
        assert report["status"] == jpeg.ENCODED and report["bytes"] == len(want), (c.name, report)
        assert data == want, c.name
        assert len(want) <= jpeg.encode_bound(_geometry(c)), c.name


def test_the_stage_model_re_encodes_to_the_same_bytes():
    for c in ec.cases():
        assert ec.encode(c.frame, c.quality, c.subsampling, c.channel_order) == ec.expected(c), c.name


def test_the_table_holds_the_sizes_options_and_contents_of_the_issue():
    cases = ec.cases()
    names = {c.name for c in cases}
    for w, h in ec.SIZES:
        for tag in ("444", "422", "420", "grey", "420_bgr"):
            assert f"noise_{w}x{h}_q75_{tag}" in names
    for kind in ec.CONTENTS:
        assert any(n.startswith(kind + "_") for n in names), kind
    assert {c.quality for c in cases} >= set(ec.QUALITIES)
    assert "noise_128x96_q100_444" in names
    w, h = ec.SCAN_TILE_SIZE
    blocks = -(-w // 16) * -(-h // 16) * 6
    assert f"noise_{w}x{h}_q75_420" in names and ec.SCAN_TILE < blocks < 2 * ec.SCAN_TILE
    text = (build.CSRC / "jpeg_encode_core.h").read_text()
    assert re.search(rf"kEncScanTile = {ec.SCAN_TILE};", text)
    assert [len(b) for b in ec.batches()] == [1, 3]
    assert len({len(ec.expected(c)) for c in ec.batches()[1]}) == 3          # different contents, hence different lengths


def test_header_equals_pillows_for_every_geometry_sampling_and_quality():
    combos = {(_geometry(c), c.quality) for c in ec.cases()}
    combos |= {((40, 24, 3, 2, 2, 0), q) for q in range(1, 101)} | {((17, 15, 1, 1, 1, 0), q) for q in range(1, 101)}
    rng = np.random.default_rng(5)
    for (w, h, comps, hs, vs, _), q in sorted(combos):
        frame = rng.integers(0, 256, (h, w, 3) if comps == 3 else (h, w), dtype=np.uint8)
        sub = {v: k for k, v in ec.SAMPLING.items()}[(hs, vs)]
        want = ec.pillow_bytes(frame, q, sub)
        want = want[:ec.header_bytes_of(want)]
        head, qt = jpeg.encode_header((w, h, comps, hs, vs, 0), q)
        assert head == want, (w, h, comps, hs, vs, q)
        assert ec.header(w, h, comps, hs, vs, q) == want
        assert np.array_equal(qt, ec.quant_tables(q))
        assert len(head) == (623 if comps == 3 else 328)


def test_census_the_table_contains_every_edge_of_the_entropy_coder(modelled):
    """Each figure is taken from the model's run of the cases.  All of them can be produced from legal 8-bit input: a DC
    difference of category 11 needs quantiser 1 and neighbouring blocks near -1024 and +1016 (blocks_40x24_q100_444), an AC
    coefficient of category 10 (|v| >= 512) the sign pattern of a basis function at quantiser 1 (extreme_16x16_q100_444)."""
    cases, results = modelled
    by_name = {c.name: r[1] for c, r in zip(cases, results)}
    reports = list(by_name.values())
    assert any(r["zrl"] > 0 for r in reports)                                    # a ZRL
    assert any(r["max_zrl_block"] == 3 for r in reports)                         # three ZRLs in one block
    assert any(r["no_eob"] > 0 for r in reports)                                 # a block whose coefficient 63 is not zero
    cats = 0
    for r in reports:
        cats |= r["dc_cats"]
    assert cats & 1 and cats >> 11 & 1 and cats == 0xFFF                         # DC differences of category 0 .. 11
    assert by_name["blocks_40x24_q100_444"]["dc_cats"] >> 11 & 1
    assert max(r["ac_cat_max"] for r in reports) == 10                           # an AC coefficient of category 10, none above
    assert by_name["extreme_16x16_q100_444"]["ac_cat_max"] == 10
    assert any(r["stuffed"] > 0 for r in reports)                                # a stuffed FF inside the scan
    assert by_name["noise_8x8_q75_444_s11"]["last_ff"] == 1                      # a file whose padded last byte is FF
    assert ec.expected(next(c for c in cases if c.name == "noise_8x8_q75_444_s11")).endswith(b"\xff\x00\xff\xd9")
    assert any(r["straddle"] > 0 for r in reports)                               # a code that straddles a 32-bit word
    assert any(r["blocks"] > ec.SCAN_TILE for r in reports)                      # more blocks than one step of the prefix sum


REJECTED_BY = {
    "no_bias": "noise_17x15_q75_420",
    "no_edge": "ramp_17x15_q95_420",
    "half_up": "noise_31x33_q50_420_s1",
    "dc_shared": "noise_16x16_q75_444",
    "zrl_before_eob": "sparse_24x8_q95_444",
    "pad_zero": "noise_1x1_q75_444",
    "last_unstuffed": "noise_8x8_q75_444_s11",
    "bgr_unswapped": "noise_17x15_q75_420_bgr",
}


@pytest.mark.parametrize("mutant", ec.MUTANTS)
def test_every_mutant_of_the_stage_model_is_rejected_by_a_named_case(mutant):
    case = next(c for c in ec.cases() if c.name == REJECTED_BY[mutant])
    assert ec.encode(case.frame, case.quality, case.subsampling, case.channel_order) == ec.expected(case)
    assert ec.encode(case.frame, case.quality, case.subsampling, case.channel_order, mutant=mutant) != ec.expected(case)


def test_every_mutant_of_the_issue_is_listed():
    assert set(REJECTED_BY) == set(ec.MUTANTS) and len(ec.MUTANTS) == 8


def test_a_slot_that_is_too_small_is_reported_and_nothing_behind_it_is_written(model, tmp_path):
    """The model's output buffer is exactly the slot: a write behind it is the sanitizer's finding."""
    case = next(c for c in ec.cases() if c.name == "noise_31x33_q95_420_s1")
    size = len(ec.expected(case))
    strides = [size, size - 1, 700, 100, 1]
    results = _run(model, tmp_path, [case] * len(strides), strides)
    assert results[0][0] == ec.expected(case) and results[0][1]["status"] == jpeg.ENCODED
    for data, report in results[1:]:
        assert data is None and report["status"] == jpeg.ENCODE_OVERFLOW and report["bytes"] == size


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


def test_bound_and_workspace_queries():
    from hippomm_amd import _lib
    build.build()
    lib = _lib.load()
    g = jpeg._geom_array((1280, 720, 3, 2, 2, 0))
    blocks = 80 * 45 * 6
    assert lib.hmm_jpeg_encode_bound(g.ctypes.data) == 623 + 2 * ((blocks * (22 + 63 * 26) + 7) // 8) + 2
    one = lib.hmm_jpeg_encode_workspace_bytes(g.ctypes.data, 1)
    assert one >= blocks * 128 + (blocks + 1) * 4 + (blocks * 1660 + 7) // 8 and one % 256 == 0
    assert lib.hmm_jpeg_encode_workspace_bytes(g.ctypes.data, 4) >= 4 * (one - 3 * 256)
    assert lib.hmm_jpeg_encode_workspace_bytes(g.ctypes.data, 0) == 0
    assert lib.hmm_jpeg_encode_workspace_bytes(None, 1) == 0 and lib.hmm_jpeg_encode_bound(None) == 0
    for bad in ((0, 8, 3, 2, 2), (8, 65536, 3, 2, 2), (8, 8, 2, 1, 1), (8, 8, 3, 1, 2), (8, 8, 3, 4, 1), (65535, 65535, 3, 1, 1)):
        assert lib.hmm_jpeg_encode_bound(jpeg._geom_array(bad).ctypes.data) == 0, bad
    assert lib.hmm_jpeg_encode_bound(jpeg._geom_array((8, 8, 1, 2, 2)).ctypes.data) == 328 + 2 * 208 + 2    # grey ignores the sampling


def test_argument_errors_are_reported_without_a_gpu():
    from hippomm_amd import _lib
    build.build()
    lib = _lib.load()
    call, name = lib.hmm_jpeg_encode, b"jpeg_encode"
    g = jpeg._geom_array((40, 24, 3, 2, 2, 0))
    gp = g.ctypes.data
    ws = lib.hmm_jpeg_encode_workspace_bytes(gp, 3)

    def refused(*args, say, code=HMM_E_INVALID):
        assert call(*args) == code, args
        msg = lib.hmm_last_error()
        assert name in msg and say in msg, msg

    #    frames, n, geometry, channels, order, qtables, header, header_bytes, out, out_stride, status, workspace, workspace_bytes, stream
    ptrs = (ONE, 2 * ONE, 3 * ONE, FAR, 2 * FAR, 3 * FAR)                     # frames, qtables, header, out, status, workspace
    for missing in range(6):
        p = [None if i == missing else v for i, v in enumerate(ptrs)]
        refused(p[0], 3, gp, 3, 0, p[1], p[2], 623, p[3], 4096, p[4], p[5], ws, None, say=b"null pointer")
    f, q, hd, out, st, wk = ptrs
    refused(f, 3, None, 3, 0, q, hd, 623, out, 4096, st, wk, ws, None, say=b"null pointer")
    refused(f, -1, gp, 3, 0, q, hd, 623, out, 4096, st, wk, ws, None, say=b"negative")
    for bad in ((0, 24, 3, 2, 2), (40, 70000, 3, 2, 2), (40, 24, 2, 1, 1), (40, 24, 3, 1, 2), (65535, 65535, 3, 1, 1)):
        refused(f, 3, jpeg._geom_array(bad).ctypes.data, 3, 0, q, hd, 623, out, 4096, st, wk, ws, None, say=b"bad geometry")
    refused(f, 3, gp, 1, 0, q, hd, 623, out, 4096, st, wk, ws, None, say=b"channels")
    refused(f, 3, gp, 3, 2, q, hd, 623, out, 4096, st, wk, ws, None, say=b"channel order")
    refused(f, 3, gp, 3, 0, q, hd, 328, out, 4096, st, wk, ws, None, say=b"header of 328 bytes")
    refused(f, 3, gp, 3, 0, q, hd, 623, out, 4096, st, wk + 8, ws, None, say=b"aligned")
    refused(f, 3, gp, 3, 0, q, hd, 623, out, 4096, st + 2, wk, ws, None, say=b"aligned")
    refused(f, 3, gp, 3, 0, q + 1, hd, 623, out, 4096, st, wk, ws, None, say=b"aligned")
    refused(f, 3, gp, 3, 0, q, hd, 623, out, 0, st, wk, ws, None, say=b"stride")
    refused(f, 3, gp, 3, 0, q, hd, 623, out, 4096, st, wk, ws - 1, None, say=b"workspace", code=HMM_E_WORKSPACE)
    assert call(f, 0, gp, 3, 0, q, hd, 623, out, 4096, st, wk, 0, None) == HMM_OK      # no frames: no launch (there is no GPU here)

    head = np.zeros(1024, np.uint8)
    qt = np.zeros(128, np.uint16)
    for args, say in (((None, 95, head.ctypes.data, 1024, qt.ctypes.data), b"null pointer"),
                      ((gp, 0, head.ctypes.data, 1024, qt.ctypes.data), b"quality 0"),
                      ((gp, 101, head.ctypes.data, 1024, qt.ctypes.data), b"quality 101"),
                      ((gp, 95, head.ctypes.data, 622, qt.ctypes.data), b"623 needed"),
                      ((jpeg._geom_array((40, 24, 3, 2, 1 + 2)).ctypes.data, 95, head.ctypes.data, 1024, qt.ctypes.data), b"bad geometry")):
        assert lib.hmm_jpeg_encode_header(*args) == HMM_E_INVALID, args
        assert b"jpeg_encode_header" in lib.hmm_last_error() and say in lib.hmm_last_error(), lib.hmm_last_error()


def test_encode_jpeg_refuses_other_dtypes_shapes_and_options_before_it_needs_a_gpu():
    import hippomm_amd
    ok = np.zeros((8, 8, 3), np.uint8)
    for bad in (ok.astype(np.float32), ok.astype(np.int8), [ok.astype(np.uint16)], "frame", None):
        with pytest.raises(TypeError):
            hippomm_amd.encode_jpeg(bad)
    import torch
    with pytest.raises(TypeError):
        hippomm_amd.encode_jpeg(torch.zeros(8, 8, 3, dtype=torch.uint8))        # a CPU tensor: numpy or CUDA only
    for shape in ((8, 8, 4), (8, 8, 1), (2, 8, 8, 2), (8,), (1, 2, 8, 8, 3), (0, 8, 3), (8, 0), (2, 0, 8, 3), (65536, 1), (1, 65536, 3)):
        with pytest.raises(ValueError):
            hippomm_amd.encode_jpeg(np.zeros(shape, np.uint8))
    for kw in (dict(quality=0), dict(quality=101), dict(quality=95.0), dict(subsampling="4:1:1"), dict(subsampling=2),
               dict(channel_order="GBR")):
        with pytest.raises(ValueError):
            hippomm_amd.encode_jpeg(ok, **kw)
    assert hippomm_amd.encode_jpeg([]) == [] and hippomm_amd.encode_jpeg(np.zeros((0, 8, 8, 3), np.uint8)) == []


def test_save_frame_keeps_the_reference_return_rules(tmp_path, monkeypatch, caplog):
    """The encoder stubbed by Pillow (the bytes the device route returns), so the rules are checked without a GPU."""
    from hippomm_amd import frame_extraction as seg             # the module that looks _encode_bgr up, and whose logger it is
    calls = []

    def stub(frames):
        frames = list(frames) if isinstance(frames, list) else [frames]
        calls.append(len(frames))
        return [jpeg.pillow_encode(f, seg.SAVE_QUALITY, seg.SAVE_SUBSAMPLING, "BGR") for f in frames]

    monkeypatch.setattr(seg, "_encode_bgr", stub)
    frame = ec.content("noise", 17, 15, 3)
    path = tmp_path / "t_0001" / "deep" / "frame_000001.jpg"
    assert seg.save_frame(frame, path) is True and calls == [1]                 # the parent directories are created
    assert path.read_bytes() == ec.pillow_bytes(frame, 95, "4:2:0", "BGR")
    path.write_bytes(b"already here")
    assert seg.save_frame(frame, path) is True and path.read_bytes() == b"already here" and calls == [1]   # untouched, no encode
    assert seg.save_frame(frame, str(tmp_path / "as_string.jpg")) is True
    with caplog.at_level(logging.ERROR, logger=seg.__name__):
        assert seg.save_frame(None, tmp_path / "none.jpg") is False
        assert seg.save_frame(np.zeros((0, 8, 3), np.uint8), tmp_path / "empty.jpg") is False
        blocker = tmp_path / "file_not_folder"
        blocker.write_bytes(b"x")
        assert seg.save_frame(frame, blocker / "frame.jpg") is False             # the directory cannot be created: logged, False
        monkeypatch.setattr(seg, "_encode_bgr", lambda frames: (_ for _ in ()).throw(RuntimeError("encoder down")))
        assert seg.save_frame(frame, tmp_path / "error.jpg") is False
    assert not (tmp_path / "none.jpg").exists() and not (tmp_path / "empty.jpg").exists() and not (tmp_path / "error.jpg").exists()
    assert sum("Invalid frame data" in r.message for r in caplog.records) == 2
    assert any("encoder down" in r.message for r in caplog.records)

    monkeypatch.setattr(seg, "_encode_bgr", stub)
    calls.clear()
    frames = [ec.content(k, 17, 15, 3) for k in ("noise", "ramp", "mid")] + [None]
    paths = [tmp_path / "batch" / f"{k}.jpg" for k in range(4)]
    paths[1].parent.mkdir()
    paths[1].write_bytes(b"kept")
    assert seg.save_frames(frames, paths) == [True, True, True, False] and calls == [2]      # one encode call for the two new files
    assert paths[1].read_bytes() == b"kept" and paths[0].read_bytes() == ec.pillow_bytes(frames[0], 95, "4:2:0", "BGR")
    with pytest.raises(ValueError):
        seg.save_frames(frames, paths[:2])
