"""CPU: the host model of the frame-extraction loop (tests/extraction_model.py) against the golden made by the unmodified reference
(tests/golden/extraction_golden.json): fed the golden's recorded diffs, and fed 1 - ssim_oracle.ssim(frame, anchor, 255) on the
recipe's frames, it gives every case's kept frames, times, failed_saves and consulted frames; the oracle's diffs are within 1e-9 of
skimage's; the recipes still hash to what the golden was made from, and every case keeps its distance from the threshold."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE / "golden"))
import extraction_model as model  # noqa: E402
import extraction_recipes as X  # noqa: E402
import segmentation_recipes as R  # noqa: E402
import ssim_oracle  # noqa: E402

GOLDEN = json.loads((HERE / "golden" / "extraction_golden.json").read_text())["cases"]


def _check(name, got):
    g = GOLDEN[name]
    assert got.kept == g["kept"]
    assert got.frame_times == g["frame_times"]               # the same Python division, so the same floats
    assert got.failed_saves == g["failed_saves"]
    assert [i for i, _ in got.consulted] == [i for i, _ in g["consulted"]]


def test_the_golden_covers_every_recipe_and_keeps_its_margin():
    assert sorted(GOLDEN) == sorted(X.CASES)
    for name, g in GOLDEN.items():
        assert g["margin"] is None or g["margin"] >= 1e-6, name
        assert (g["margin"] is None) == (not g["consulted"]), name
    assert any(g["failed_saves"] == 2 for g in GOLDEN.values()) and any(g["failed_frames"] == [0] for g in GOLDEN.values())
    assert GOLDEN["drift_48x64_fps60"]["consulted"] != GOLDEN["drift_48x64_fps30"]["consulted"]      # the 1-s rule bites


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_model_on_the_recorded_diffs(name):
    g, c = GOLDEN[name], X.case(name)
    diff = model.recorded_diffs(g["consulted"])
    got = model.walk(c["n"], c["fps"], diff, lambda i: i not in g["failed_frames"], check_interval=c["check_interval"])
    assert not diff.left
    _check(name, got)
    assert [d for _, d in got.consulted] == [d for _, d in g["consulted"]]


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_model_on_the_oracle_ssim(name):
    g, c = GOLDEN[name], X.case(name)
    video = X.gray_frames(name)
    assert R.sha256(video) == g["input_sha256"]
    got = model.walk(c["n"], c["fps"], lambda i, a: 1.0 - ssim_oracle.ssim(video[i], video[a], 255.0),
                     lambda i: i not in g["failed_frames"], check_interval=c["check_interval"])
    _check(name, got)
    if g["consulted"]:
        assert np.abs(np.array([d for _, d in got.consulted]) - np.array([d for _, d in g["consulted"]])).max() <= 1e-9


def test_records_describe_every_frame_looked_at():
    """Before the first save every frame is looked at; afterwards only the check frames; a refused save changes nothing."""
    got = model.walk(200, 30.0, lambda i, a: 0.2, lambda i: i not in (0, 1, 90), check_interval=30)
    assert [r[0] for r in got.records] == [0, 1, 2, 30, 60, 90, 120, 150, 180]
    assert got.kept == [2, 120, 180] and got.failed_saves == 3
    by = {r[0]: r for r in got.records}
    assert by[30][1:5] == (0, 0, 0.0, 0.0)                    # less than a second after frame 2: not compared
    assert by[90][1:5] == (1, 0, 0.2, 0.4)                    # compared, wanted, refused: cumulative_diff stays
    assert by[120][1:5] == (1, 1, 0.2, 0.0)
