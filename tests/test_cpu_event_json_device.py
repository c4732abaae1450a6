"""CPU: the float printer of the device JSON writer (csrc/event_json_core.h), run on the host through hmm_json_float_repr, against
Python's own repr -- and against hmm_json_write_matrix_f64, the writer the device's text must equal; the committed power-of-five
tables against their generator; the argument checks of hmm_json_write_matrix_device, which need no GPU."""
import subprocess
import sys

import numpy as np
import pytest

import event_json_cases as jc


def _agree(values, what):
    values = np.ascontiguousarray(values, np.float64).reshape(-1)
    got, want = jc.core_reprs(values), jc.python_reprs(values)
    bad = [(float(values[i]).hex(), got[i], want[i]) for i in range(values.size) if got[i] != want[i]]
    assert not bad, f"{what}: {len(bad)} of {values.size} differ from repr(), e.g. {bad[:3]}"
    second = jc.host_writer_reprs(values)
    assert second == got, f"{what}: differs from hmm_json_write_matrix_f64 at {[i for i in range(values.size) if second[i] != got[i]][:3]}"


def test_tables_are_what_their_generator_prints():
    r = subprocess.run([sys.executable, str(jc.ROOT / "tools" / "gen_event_json_tables.py"), "--check"])
    assert r.returncode == 0, "hippomm_amd/csrc/event_json_tables.h is not the output of tools/gen_event_json_tables.py"


def test_every_binary_exponent():
    _agree(jc.every_exponent(np.random.default_rng(1)), "every exponent")


def test_random_bit_patterns():
    bits = np.random.default_rng(2).integers(0, 2 ** 64, 2_000_000, dtype=np.uint64)
    _agree(bits.view(np.float64), "random 64-bit patterns")


def test_widened_fp32():
    _agree(np.random.default_rng(3).uniform(-1, 1, 1_000_000).astype(np.float32).astype(np.float64), "fp32 in [-1, 1]")


def test_powers_of_ten_and_their_neighbours():
    _agree(jc.powers_of_ten(), "powers of ten")


def test_notation_switches_and_odd_values():
    values = jc.ODD_VALUES + [-x for x in jc.ODD_VALUES] + [1.5e300, 1e-300, 1.234e+100, 9.999999999999999e22, 1e23]
    _agree(values, "odd values")
    spelled = dict(zip([float(v).hex() if v == v else "nan" for v in values], jc.core_reprs(values)))
    assert spelled[float(1e16).hex()] == b"1e+16" and spelled[float(9999999999999998.0).hex()] == b"9999999999999998.0"
    assert spelled[float(0.0001).hex()] == b"0.0001" and spelled[float(1e-05).hex()] == b"1e-05"
    assert spelled["nan"] == b"NaN" and spelled[float("inf").hex()] == b"Infinity" and spelled[float("-inf").hex()] == b"-Infinity"
    assert spelled[float(-0.0).hex()] == b"-0.0" and spelled[float(0.0).hex()] == b"0.0"
    assert spelled[float(5e-324).hex()] == b"5e-324" and spelled[float(1e22).hex()] == b"1e+22"
    assert spelled[float(jc.LONGEST_F64).hex()] == b"-1.2345678901234567e-308"


def test_argument_errors_are_reported_without_a_gpu():
    from hippomm_amd import _lib
    lib = _lib.load()
    bound = lib.hmm_json_matrix_text_bound(3, 5, 4)
    need = lib.hmm_json_write_matrix_device_workspace_bytes(3, 5)
    assert need == 8 and lib.hmm_json_write_matrix_device_workspace_bytes(2, jc.VALUES_PER_GROUP) == 16
    assert lib.hmm_json_write_matrix_device_workspace_bytes(0, 5) == 0 and lib.hmm_json_write_matrix_device_workspace_bytes(5, 0) == 0
    assert lib.hmm_json_write_matrix_device_workspace_bytes(2 ** 31, 2) == 0
    p = 4096                                                      # never dereferenced: every case is refused before a launch
    good = dict(m=p, dtype=0, rows=3, cols=5, indent=4, out=p, cap=bound, written=p, ws=p, ws_bytes=need)

    def call(**change):
        a = dict(good, **change)
        rc = lib.hmm_json_write_matrix_device(a["m"], a["dtype"], a["rows"], a["cols"], a["indent"], a["out"], a["cap"], a["written"],
                                              a["ws"], a["ws_bytes"], None)
        return rc, lib.hmm_last_error()

    for change, word in [(dict(cap=bound - 1), b"buffer"), (dict(ws_bytes=need - 1), b"workspace"), (dict(rows=0), b"at least"),
                         (dict(cols=0), b"at least"), (dict(m=None), b"null"), (dict(out=None), b"null"), (dict(written=None), b"null"),
                         (dict(ws=None), b"null"), (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
                         (dict(rows=2 ** 31, cols=2, cap=2 ** 40), b"at most"), (dict(indent=-1), b"close_indent"),
                         (dict(indent=33, cap=2 ** 20), b"close_indent"), (dict(m=p + 2), b"aligned"), (dict(dtype=1, m=p + 4), b"aligned"),
                         (dict(written=p + 4), b"aligned")]:
        rc, message = call(**change)
        assert rc == -1 and message.startswith(b"json_write_matrix_device") and word in message, (change, rc, message)


def test_python_entry_points_validate_before_any_gpu_work():
    from hippomm_amd import event_store as es
    with pytest.raises(TypeError):
        es.matrix_json_bytes([[1.0, 2.0]])
    with pytest.raises(TypeError):
        es.matrix_json_bytes(np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError):
        es.matrix_json_bytes(np.zeros(4, np.float32))
    with pytest.raises(ValueError):
        es.matrix_json_bytes(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError):
        es.matrix_json_bytes(np.zeros((2, 2), np.float32), close_indent=33)
    with pytest.raises(ValueError):
        es.event_json_bytes({"features": {}}, matrices="gpu")
