"""CPU: the host side of the recall frame windows -- cv2.resize's 8-bit INTER_LINEAR tables (segmentation.resize_linear_tables)
against hand-derived values and the index-by-index restatement in tests/resize_oracle.py, the choice between the linear and the
2 x 2 area arithmetic, the dedup walk of a window on hand-made scores, and the C ABI of hmm_resize_linear_u8: declared, exported,
bound, the ABI version unchanged, every argument error a status code with a message on a host without a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import resize_oracle as ro

ROOT = Path(__file__).resolve().parent.parent
HMM_OK, HMM_E_INVALID = 0, -1
NAN = float("nan")


# ---- tables ------------------------------------------------------------------------------------------------------------------
def test_1920_to_320_reads_the_two_middle_pixels_of_every_six_with_equal_weights():
    from hippomm_amd.resize import resize_linear_tables
    ofs, coef = resize_linear_tables(1920, 320)
    assert ofs.dtype == np.int32 and coef.dtype == np.int16 and ofs.shape == (320,) and coef.shape == (320, 2)
    assert ofs.tolist() == [6 * d + 2 for d in range(320)]
    assert (coef == 1024).all()
    ofs, coef = resize_linear_tables(1080, 180)
    assert ofs.tolist() == [6 * d + 2 for d in range(180)] and (coef == 1024).all()


def test_1440_to_320_alternates_quarter_and_three_quarter_weights():
    from hippomm_amd.resize import resize_linear_tables
    ofs, coef = resize_linear_tables(1440, 320)                          # scale 4.5: f = 4.5 d + 1.75
    assert ofs.tolist() == [int(np.floor(4.5 * d + 1.75)) for d in range(320)]
    assert coef[0::2].tolist() == [[512, 1536]] * 160
    assert coef[1::2].tolist() == [[1536, 512]] * 160


def test_identity_takes_every_pixel_whole():
    from hippomm_amd.resize import resize_linear_tables
    ofs, coef = resize_linear_tables(180, 180)
    assert ofs.tolist() == list(range(180))
    assert coef.tolist() == [[2048, 0]] * 180


def test_a_product_ending_in_one_half_rounds_to_even():
    """2049 -> 2048: f = (2 d + 1) / 4096 exactly, so f * 2048 = d + 0.5 and (1 - f) * 2048 = 2047 - d + 0.5; rint goes to the even
    neighbour of each (round-half-up would give (2048, 1) at d = 0)."""
    from hippomm_amd.resize import resize_linear_tables
    ofs, coef = resize_linear_tables(2049, 2048)
    assert ofs[:6].tolist() == [0, 1, 2, 3, 4, 5]
    assert coef[:6].tolist() == [[2048, 0], [2046, 2], [2046, 2], [2044, 4], [2044, 4], [2042, 6]]


@pytest.mark.parametrize("src,dst", [(1920, 320), (1440, 320), (1080, 180), (1280, 320), (720, 180), (323, 320), (181, 180),
                                     (640, 320), (400, 180), (11, 7), (9, 5), (2049, 2048), (7, 7), (1000, 333), (4097, 1031)])
def test_tables_equal_the_index_by_index_restatement(src, dst):
    from hippomm_amd.resize import resize_linear_tables
    ofs, coef = resize_linear_tables(src, dst)
    want_ofs, want_coef = ro.tables(src, dst)
    assert ofs.tolist() == want_ofs.tolist() and coef.tolist() == want_coef.tolist()
    assert ofs.min() >= 0 and ofs.max() <= src - 1
    assert (ofs + 1 < src).all() or src == dst                           # s + 1 leaves the row only at scale 1


def test_tables_are_cached_and_read_only():
    from hippomm_amd.resize import resize_linear_tables
    a, b = resize_linear_tables(720, 180), resize_linear_tables(720, 180)
    assert a[0] is b[0] and a[1] is b[1]
    with pytest.raises(ValueError):
        a[0][0] = 1


# ---- mode --------------------------------------------------------------------------------------------------------------------
def test_mode_is_area_only_when_both_scales_are_two():
    from hippomm_amd.resize import RESIZE_AREA2X, RESIZE_LINEAR, resize_mode
    assert resize_mode((360, 640), (180, 320)) == RESIZE_AREA2X
    assert resize_mode((400, 640), (180, 320)) == RESIZE_LINEAR         # only x is 2
    assert resize_mode((360, 641), (180, 320)) == RESIZE_LINEAR
    assert resize_mode((1080, 1920), (180, 320)) == RESIZE_LINEAR       # an integer scale, but not 2
    assert resize_mode((180, 320), (180, 320)) == RESIZE_LINEAR
    assert resize_mode((14, 12), (7, 6)) == RESIZE_AREA2X
    assert ro.is_area((360, 640), (180, 320)) and not ro.is_area((400, 640), (180, 320))


@pytest.mark.parametrize("src,dst", [((179, 320), (180, 320)), ((180, 319), (180, 320)), ((90, 160), (180, 320)), ((360, 300), (180, 320))])
def test_an_enlargement_on_either_axis_is_refused(src, dst):
    from hippomm_amd.resize import resize_linear_tables, resize_mode
    with pytest.raises(ValueError, match="no larger than the source"):
        resize_mode(src, dst)
    with pytest.raises(ValueError, match="no enlargement"):
        resize_linear_tables(160, 320)


# ---- the walk ----------------------------------------------------------------------------------------------------------------
def _scores(m, entries):
    t = np.full((m, m), 123.0)                                           # a consulted entry that was not set would drop a frame
    for (i, j), v in entries.items():
        t[i, j] = v
    return t


def test_walk_keeps_frame_zero_and_a_window_of_one():
    from hippomm_amd.retrieval import walk_recall_window
    assert walk_recall_window([]) == []
    assert walk_recall_window([[NAN]]) == [0]
    assert walk_recall_window(np.zeros((1, 1))) == [0]


def test_walk_of_two_drops_above_the_cut_only():
    from hippomm_amd.retrieval import walk_recall_window
    assert walk_recall_window(_scores(2, {(0, 1): 0.31})) == [0]
    assert walk_recall_window(_scores(2, {(0, 1): 0.29})) == [0, 1]
    assert walk_recall_window(_scores(2, {(0, 1): 0.3})) == [0, 1]       # the reference drops on > 0.3
    assert walk_recall_window(_scores(2, {(0, 1): NAN})) == [0, 1]       # NaN > 0.3 is False: the frame stays
    assert walk_recall_window(_scores(2, {(0, 1): 0.31}), similarity_cut=0.5) == [0, 1]


def test_a_dropped_frame_does_not_become_the_base():
    from hippomm_amd.retrieval import walk_recall_window
    # 1 is dropped against 0; 2 is then compared with 0 (kept), not with 1: (1, 2) says "drop" and must not be consulted
    assert walk_recall_window(_scores(3, {(0, 1): 0.9, (0, 2): 0.1, (1, 2): 0.9})) == [0, 2]
    # 1 is kept and becomes the base: (0, 2) says "keep" and must not be consulted
    assert walk_recall_window(_scores(3, {(0, 1): 0.1, (1, 2): 0.9, (0, 2): 0.1})) == [0, 1]
    assert walk_recall_window(_scores(3, {(0, 1): NAN, (1, 2): NAN, (0, 2): 0.9})) == [0, 1, 2]
    assert walk_recall_window(_scores(3, {(0, 1): 0.9, (0, 2): 0.9, (1, 2): 0.1})) == [0]


def test_walk_of_eight_follows_the_last_kept_frame():
    from hippomm_amd.retrieval import walk_recall_window
    consulted = {(0, 1): 0.8, (0, 2): 0.7, (0, 3): 0.2, (3, 4): NAN, (4, 5): 0.6, (4, 6): 0.31, (4, 7): 0.0}
    assert walk_recall_window(_scores(8, consulted)) == [0, 3, 4, 7]
    everything_new = {(i, i + 1): 0.0 for i in range(7)}
    assert walk_recall_window(_scores(8, everything_new)) == list(range(8))
    still = {(0, j): 1.0 for j in range(1, 8)}
    assert walk_recall_window(_scores(8, still)) == [0]


def test_the_gpu_tests_inputs_decide_far_from_the_cut():
    """tests/recall_window_cases.py, the composed oracle route: every score the walk consults is NaN or further than 1e-6 from
    0.3 (the GPU's SSIM differs from the oracle's in the last digits only), and the windows exercise what they are named for."""
    import recall_window_cases as rc
    from hippomm_amd.retrieval import walk_recall_window
    want = {w["name"]: w for w in rc.expected()}
    for w in want.values():
        for i, j, s in w["consulted"]:
            assert np.isnan(s) or abs(s - rc.CUT) > rc.MARGIN, (w["name"], i, j, s)
        m = len(w["all_files"])
        table = np.full((m, m), 123.0)
        for i, j, s in w["consulted"]:
            table[i, j] = s
        assert walk_recall_window(table) == w["kept"], w["name"]          # the same walk, consulting the same pairs
    assert want["identical"]["kept"] == [0] and want["noise"]["kept"] == [0, 1, 2] and want["single"]["kept"] == [0]
    assert want["flat_first"]["kept"] == [0, 1] and np.isnan(want["flat_first"]["consulted"][0][2])
    assert want["other_geometry"]["kept"] == [0, 2] and want["mixed_geometries"]["kept"] == [0, 1] and want["empty"]["kept"] == []


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
ONE = 1 << 20                                                            # aligned non-null dummies, far apart
SRC, DST, XO, XC, YO, YC = ONE, 2 * ONE, 3 * ONE, 4 * ONE, 5 * ONE, 6 * ONE


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_is_declared_exported_and_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, build
    import hippomm_amd
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    assert "hmm_resize_linear_u8" in set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    assert hasattr(ctypes.CDLL(str(build.build())), "hmm_resize_linear_u8")
    assert "hmm_resize_linear_u8" in _lib._SIGNATURES
    assert _lib.load().hmm_abi_version() == 7
    assert callable(hippomm_amd.recall_window_frames)


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib()
    call = lib.hmm_resize_linear_u8

    def refused(*args, say):
        assert call(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert b"resize_linear_u8" in msg and say in msg, msg

    #       src, n, src_h, src_w, channels, dst, dst_h, dst_w, xofs, xcoef, yofs, ycoef, mode, stream
    refused(SRC, 1, 360, 640, 3, DST, 180, 320, XO, XC, YO, YC, 2, None, say=b"mode")
    refused(SRC, 1, 360, 640, 3, DST, 180, 320, XO, XC, YO, YC, -1, None, say=b"mode")
    for channels in (0, 2, 4):
        refused(SRC, 1, 360, 640, channels, DST, 180, 320, XO, XC, YO, YC, 0, None, say=b"channels")
    refused(SRC, -1, 360, 640, 3, DST, 180, 320, XO, XC, YO, YC, 0, None, say=b"n=")
    refused(SRC, 65536, 360, 640, 3, DST, 180, 320, XO, XC, YO, YC, 0, None, say=b"n=")
    for dims in ((0, 640, 180, 320), (360, 0, 180, 320), (360, 640, 0, 320), (360, 640, 180, 0), (360, 640, -180, 320),
                 (65536, 640, 180, 320), (360, 65536, 180, 320)):
        refused(SRC, 1, dims[0], dims[1], 3, DST, dims[2], dims[3], XO, XC, YO, YC, 0, None, say=b"bad shape")
    refused(SRC, 1, 65535, 65535, 1, DST, 65535, 65535, XO, XC, YO, YC, 0, None, say=b"too large")
    refused(SRC, 1, 179, 640, 3, DST, 180, 320, XO, XC, YO, YC, 0, None, say=b"enlarges")
    refused(SRC, 1, 360, 319, 3, DST, 180, 320, XO, XC, YO, YC, 0, None, say=b"enlarges")
    refused(SRC, 1, 400, 640, 3, DST, 180, 320, XO, XC, YO, YC, 1, None, say=b"exactly twice")
    refused(SRC, 1, 360, 641, 3, DST, 180, 320, XO, XC, YO, YC, 1, None, say=b"exactly twice")
    refused(None, 1, 360, 640, 3, DST, 180, 320, XO, XC, YO, YC, 0, None, say=b"null pointer")
    refused(SRC, 1, 360, 640, 3, None, 180, 320, XO, XC, YO, YC, 0, None, say=b"null pointer")
    refused(SRC, 1, 360, 640, 3, None, 180, 320, None, None, None, None, 1, None, say=b"null pointer")
    for missing in range(4):
        t = [None if i == missing else v for i, v in enumerate((XO, XC, YO, YC))]
        refused(SRC, 1, 400, 640, 3, DST, 180, 320, *t, 0, None, say=b"null pointer")
    refused(SRC, 1, 400, 640, 3, DST, 180, 320, XO + 2, XC, YO, YC, 0, None, say=b"aligned")
    refused(SRC, 1, 400, 640, 3, DST, 180, 320, XO, XC, YO + 1, YC, 0, None, say=b"aligned")
    refused(SRC, 1, 400, 640, 3, DST, 180, 320, XO, XC + 1, YO, YC, 0, None, say=b"aligned")
    refused(SRC, 1, 400, 640, 3, DST, 180, 320, XO, XC, YO, YC + 1, 0, None, say=b"aligned")


def test_zero_frames_return_ok_without_a_launch():
    """No GPU on this host: a launch would fail, HMM_OK means none was tried."""
    lib = _lib()
    assert lib.hmm_resize_linear_u8(None, 0, 360, 640, 3, None, 180, 320, None, None, None, None, 1, None) == HMM_OK
    assert lib.hmm_resize_linear_u8(None, 0, 400, 640, 1, None, 180, 320, None, None, None, None, 0, None) == HMM_OK
    assert lib.hmm_resize_linear_u8(None, 0, 100, 640, 1, None, 180, 320, None, None, None, None, 0, None) == HMM_E_INVALID


# ---- the Python layer, as far as it goes without a GPU -------------------------------------------------------------------------
def test_recall_window_frames_validates_before_it_needs_a_gpu():
    from hippomm_amd import recall_window_frames
    frame = np.zeros((360, 640, 3), np.uint8)
    with pytest.raises(ValueError, match="at most 8"):
        recall_window_frames([[(float(i), frame) for i in range(9)]])
    with pytest.raises(TypeError, match="uint8"):
        recall_window_frames([[(0.0, frame.astype(np.float32))]])
    with pytest.raises(TypeError, match="BGR"):
        recall_window_frames([[(0.0, frame[..., 0])]])
    with pytest.raises(ValueError, match="no larger than the source"):
        recall_window_frames([[(0.0, frame), (1.0, np.zeros((90, 160, 3), np.uint8))]])
    with pytest.raises(ValueError, match="one path per frame"):
        recall_window_frames([[(0.0, frame), (1.0, frame)]], paths=[["a.jpg"]])
    with pytest.raises(ValueError, match="paths="):
        recall_window_frames([[(0.0, frame)]], cache=object())
    with pytest.raises(ValueError, match="SSIM window"):
        recall_window_frames([[(0.0, frame)]], size=(6, 180))
    got = recall_window_frames([])                                       # nothing to do: no GPU needed
    assert got.kept == [] and got.all_segment_times == [] and got.all_segment_files == [] and got.all_segment_frames is None
    got = recall_window_frames([[], []], paths=[[], []])
    assert got.kept == [[], []] and got.files == [[], []] and got.all_segment_frames == []
