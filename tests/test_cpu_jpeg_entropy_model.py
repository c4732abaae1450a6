"""CPU: the device entropy pass's logic (hippomm_amd/csrc/jpeg_entropy_core.h), run thread by thread by the stand-alone model
program tools/jpeg_entropy_model.cpp under AddressSanitizer and UBSan, gives the host entropy pass's status for every file the
prepare pass takes and the host pass's slot bytes where both decode: over the corpus (whole frame and two windows each) and over
the seeded damage sweep of test_cpu_jpeg.py.  The program is built here from source with the host compiler of hipcc; nothing is
loaded into this interpreter."""
import re
import subprocess
from pathlib import Path

import pytest

import jpeg_entropy_corpus as jc
from hippomm_amd import build, jpeg

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("entropy_model") / "jpeg_entropy_model"
    cmd = [build._hipcc(), "-O1", "-g", "-std=c++17", "-x", "hip", f"--offload-arch={build.ARCH}", "-I", str(ROOT / "include"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           str(ROOT / "tools" / "jpeg_entropy_model.cpp"), str(build.CSRC / "jpeg_host.cpp"), "-fsanitize=address,undefined", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def _run(model, tmp_path, cases):
    """cases: (name, bytes, geometry, window) -> the program's report lines by name."""
    lines = []
    for k, (name, data, g, win) in enumerate(cases):
        path = tmp_path / f"{k:04d}_{name}.jpg"
        path.write_bytes(data)
        lines.append(" ".join([str(path)] + [str(int(v)) for v in (*g[:5], *win)]))
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(model), str(manifest)], capture_output=True, text=True, timeout=600)
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert r.returncode == 0, report[-4000:]
    assert "MISMATCH" not in r.stdout
    return r.stdout


def test_model_equals_the_host_pass_on_the_corpus(model, tmp_path):
    cases = []
    for name, data in jc.corpus():
        g = jpeg.parse(data)
        cases += [(name, data, g, win) for win in jc.windows(g)]
    out = _run(model, tmp_path, cases)
    m = re.search(r"cases=(\d+) taken=(\d+) decoded=(\d+) failures=(\d+)", out)
    assert m, out[-2000:]
    n = len(cases)
    assert tuple(map(int, m.groups())) == (n, n, n, 0), out[-2000:]          # every corpus frame is decoded by the model itself
    for name in ("noise_q95_256x144", "noise_q95_256x144_opt", "noise_q95_640x360"):
        rounds = [int(r) for r in re.findall(rf"_{name}\.jpg threads=256 .* rounds=(\d+)", out)]
        assert rounds and min(rounds) >= 2, (name, rounds)                   # the fixed point is exercised, not only the first guess


def test_model_equals_the_host_pass_on_the_damage_sweep(model, tmp_path):
    cases = [("damaged", data, g, (0, 0, g[0], g[1])) for g, data in jc.damage_sweep()]
    out = _run(model, tmp_path, cases)
    m = re.search(r"cases=(\d+) taken=(\d+) decoded=(\d+) failures=(\d+)", out)
    assert m, out[-2000:]
    n_cases, taken, decoded, failures = map(int, m.groups())
    assert n_cases == len(cases) == 800 and failures == 0
    assert taken > 200 and decoded > 0 and decoded < taken                   # the sweep reaches both outcomes
