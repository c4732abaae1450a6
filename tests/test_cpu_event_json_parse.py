"""CPU: the number parser of the device JSON reader (csrc/event_json_parse_core.h), run on the host through hmm_json_float_parse,
against Python's own float(token) and np.float32(float(token)), bit for bit; which tokens it flags against the rule, stated with
Python integers in event_json_parse_cases.expected_flag; the committed power-of-ten table against its generator; the argument
checks of hmm_json_parse_matrix_device, which need no GPU; and the Python entry points' defaults."""
import json
import subprocess
import sys

import numpy as np
import pytest

import event_json_parse_cases as pc


def _agree(tokens, what, never_flagged=False):
    """Unflagged results are Python's bits; the flags are exactly the rule's; flagged and bad tokens carry no value."""
    f64, f32, flags = pc.core_parse(tokens)
    want_flags = np.array([pc.expected_flag(t) for t in tokens], np.int32)
    wrong = np.nonzero(flags != want_flags)[0]
    assert wrong.size == 0, f"{what}: flags differ from the rule, e.g. {[(tokens[i], int(flags[i]), int(want_flags[i])) for i in wrong[:3]]}"
    if never_flagged:
        assert not flags.any(), f"{what}: {tokens[int(np.nonzero(flags)[0][0])]} is flagged"
    done = flags == 0
    want64, want32 = pc.python_bits([t for t, ok in zip(tokens, done.tolist()) if ok])
    bad = np.nonzero((f64[done] != want64) | (f32[done] != want32))[0]
    kept = [t for t, ok in zip(tokens, done.tolist()) if ok]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(kept)} differ from float(), e.g. "
                           f"{[(kept[i], hex(int(f64[done][i])), hex(int(want64[i])), hex(int(f32[done][i])), hex(int(want32[i]))) for i in bad[:3]]}")
    assert not f64[~done].any() and not f32[~done].any(), f"{what}: a flagged token has a value"
    return flags


def test_table_is_what_its_generator_prints():
    r = subprocess.run([sys.executable, str(pc.ROOT / "tools" / "gen_event_json_parse_tables.py"), "--check"])
    assert r.returncode == 0, "hippomm_amd/csrc/event_json_parse_tables.h is not the output of tools/gen_event_json_parse_tables.py"


def test_fp32_origin_values():
    tokens = pc.f32_origin(np.random.default_rng(1), 2_000_000)
    assert len(tokens) >= 2_000_000 + 4 * 256
    _agree(tokens, "fp32-origin", never_flagged=True)


def test_doubles_over_every_binary_exponent():
    _agree(pc.doubles(np.random.default_rng(2)), "doubles", never_flagged=True)


def test_powers_of_ten_and_the_ends_of_the_range():
    tokens = pc.powers_of_ten()
    flags = _agree(tokens, "powers of ten")
    flagged = {t for t, f in zip(tokens, flags.tolist()) if f}
    assert all(f in (0, pc.RANGE) for f in flags.tolist())
    assert flagged == {b"1e%d" % k for k in list(range(-330, -323)) + [309, 310]}      # float() gives 0.0 and inf there


def test_nineteen_digits_beside_a_halfway_point():
    tokens = pc.beside_halfway(np.random.default_rng(3), 20_000)
    assert len(tokens) >= 50_000 and max(map(len, tokens)) <= 25
    _agree(tokens, "19 digits beside a halfway point", never_flagged=True)


def test_long_literals_are_flagged_or_right():
    tokens = pc.long_literals(np.random.default_rng(4), 300)
    flags = _agree(tokens, "long literals")
    counts = {f: int((flags == f).sum()) for f in (0, pc.UNDECIDED, pc.RANGE, pc.TOO_LONG)}
    assert counts[pc.UNDECIDED] >= 100 and counts[pc.TOO_LONG] >= 100 and counts[0] >= 100 and counts[pc.RANGE] >= 2, counts


def test_fp32_double_rounding():
    tokens = pc.f32_double_rounding(np.random.default_rng(5), 20_000)
    assert len(tokens) >= 20_000                                     # midpoints of 19 digits or fewer are left out
    _, want32 = pc.python_bits(tokens)
    assert (want32[0::2] == want32[1::2]).all() and not (want32 & 1).any()      # both sides of the fp32 midpoint go to the even one
    _agree(tokens, "fp32 double rounding", never_flagged=True)


def test_plain_spellings():
    f64, f32, flags = pc.core_parse(pc.PLAIN)
    _agree(pc.PLAIN, "plain spellings")
    spelled = dict(zip(pc.PLAIN, zip(f64.tolist(), f32.tolist(), flags.tolist())))
    assert spelled[b"-0.0"] == (1 << 63, 1 << 31, 0) and spelled[b"-0e0"] == (1 << 63, 1 << 31, 0) and spelled[b"-0"] == (0, 0, 0)
    assert spelled[b"NaN"] == (0x7FF8000000000000, 0x7FC00000, 0) and spelled[b"-Infinity"] == (0xFFF0000000000000, 0xFF800000, 0)
    assert spelled[b"Infinity"] == (0x7FF0000000000000, 0x7F800000, 0) and spelled[b"5e-324"] == (1, 0, 0)
    assert spelled[b"2.4703282292062327e-324"][2] == pc.RANGE and spelled[b"2.4703282292062328e-324"] == (1, 0, 0)
    assert spelled[b"1.7976931348623158e308"][:2] == (0x7FEFFFFFFFFFFFFF, 0x7F800000) and spelled[b"0e99999"][2] == pc.RANGE
    integers = [str(10 ** k + k).encode() for k in range(19)] + [str(10 ** k - 1).encode() for k in range(1, 20)]
    _agree(integers, "integers up to 19 digits", never_flagged=True)


def test_bad_tokens_get_the_grammar_flag_and_no_value():
    f64, f32, flags = pc.core_parse(pc.BAD_TOKENS)
    assert flags.tolist() == [pc.BAD] * len(pc.BAD_TOKENS), [t for t, f in zip(pc.BAD_TOKENS, flags.tolist()) if f != pc.BAD]
    assert not f64.any() and not f32.any()
    for t in pc.BAD_TOKENS:                                          # and json agrees that none of them is a number
        with pytest.raises(ValueError):
            json.loads(t)


def test_argument_errors_are_reported_without_a_gpu():
    from hippomm_amd import _lib
    lib = _lib.load()
    q = lib.hmm_json_parse_matrix_device_workspace_bytes
    assert q(1) == 8 and q(pc.GROUP_BYTES) == 8 and q(pc.GROUP_BYTES + 1) == 16 and q(0) == 0 and q(2 ** 41) == 0
    p = 4096                                                      # never dereferenced: every case is refused before a launch
    good = dict(text=p, begin=3, end=103, rows=3, cols=5, dtype=0, out=p, report=p, flagged=p, cap=4, ws=p, ws_bytes=8)

    def call(**change):
        a = dict(good, **change)
        rc = lib.hmm_json_parse_matrix_device(a["text"], a["begin"], a["end"], a["rows"], a["cols"], a["dtype"], a["out"], a["report"],
                                              a["flagged"], a["cap"], a["ws"], a["ws_bytes"], None)
        return rc, lib.hmm_last_error()

    for change, word in [(dict(text=None), b"null"), (dict(out=None), b"null"), (dict(report=None), b"null"), (dict(ws=None), b"null"),
                         (dict(flagged=None), b"null"), (dict(begin=103), b"empty span"), (dict(begin=104), b"empty span"),
                         (dict(rows=0), b"at least"), (dict(cols=0), b"at least"), (dict(rows=2 ** 31, cols=2), b"at most"),
                         (dict(rows=2 ** 31 + 1, cols=1), b"at most"), (dict(dtype=2), b"dtype"), (dict(dtype=-1), b"dtype"),
                         (dict(ws_bytes=7), b"workspace"), (dict(end=3 + pc.GROUP_BYTES + 1), b"workspace"), (dict(cap=-1), b"negative"),
                         (dict(out=p + 2), b"aligned"), (dict(dtype=1, out=p + 4), b"aligned"), (dict(report=p + 4), b"aligned"),
                         (dict(flagged=p + 4), b"aligned"), (dict(ws=p + 4), b"aligned"), (dict(end=2 ** 41), b"at most")]:
        rc, message = call(**change)
        assert rc == -1 and message.startswith(b"json_parse_matrix_device") and word in message, (change, rc, message)


def test_python_entry_points_validate_and_keep_their_defaults(tmp_path):
    from hippomm_amd import event_store as es
    feats = {"vision": np.random.default_rng(6).standard_normal((2, 1024)).astype(np.float32)}
    path = es.save_event({"features": feats}, tmp_path / "e.json", write_sidecars=False)
    with pytest.raises(ValueError):
        es.parse_event_features(path, matrices="bogus")
    with pytest.raises(ValueError):
        es.build_event_store(tmp_path, parse="bogus")
    with pytest.raises(ValueError):
        es.refresh_event_store(None, [], tmp_path, parse="bogus")
    with pytest.raises(TypeError):
        es.parse_matrix_device("[[1.0]]", (0, 7, 1, 1))
    with pytest.raises(ValueError):
        es.parse_matrix_device(b"[[1.0]]", (0, 7, 1, 1), dtype=np.int32)
    with pytest.raises(ValueError):
        es.parse_matrix_device(b"[[1.0]]", (0, 8, 1, 1))
    stats = {}
    got, _ = es.parse_event_features(path, stats=stats)              # no `matrices` argument: the host route, as before
    assert stats == {"device": 0, "host": 1, "json": 0} and isinstance(got["vision"], np.ndarray)
    assert got["vision"].tobytes() == feats["vision"].tobytes()
    assert es.matrix_parse_stats()["device"] == 0
