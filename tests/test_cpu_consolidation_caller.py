"""CPU: the consolidation caller without a GPU -- the host plans (plan_vision_rows / plan_audio_rows) against the fixture the
UNMODIFIED reference wrote (tests/golden/consolidation_caller_golden.json: row order, times, skipped counts, kept frames), the C
ABI of hmm_rows_gather (declared, exported, bound; every argument error a status code with the function's name, nothing
dereferenced or launched before the checks; n = 0 answered with HMM_OK), and, where the reference checkout is present, the
fixture's generator reproducing the committed file."""
import ctypes
import re
import subprocess
import sys
import types
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(Path(__file__).resolve().parent))
import consolidation_cases as K  # noqa: E402

HMM_OK, HMM_E_INVALID = 0, -1
ONE = 1 << 20                                                    # a 16-byte aligned non-null dummy
FAR = 1 << 40                                                    # another one, far from the first
GOLD = K.golden()
CASES = list(range(len(K.RECIPE["cases"])))
NAMES = [c["name"] for c in K.RECIPE["cases"]]


def test_the_fixture_was_written_from_this_recipe_and_far_from_the_threshold():
    assert GOLD["recipe"] == K.RECIPE and [c["name"] for c in GOLD["cases"]] == NAMES
    margins = [v["margin"] for c in GOLD["cases"] for v in (c["vision"], c["consolidated"]["vision"]) if v.get("margin") is not None]
    assert margins and min(margins) >= 1e-3 and GOLD["min_margin"] == 1e-3
    sizes = {len(c["vision"].get("order", [])) for c in GOLD["cases"]}
    assert {0, 1, 2, 3} <= sizes and max(sizes) >= 60
    big = GOLD["cases"][K.case_index("sixty_rows_six_clusters")]["vision"]
    assert len(big["kept"]) == 6 and len(big["order"]) == 60                 # selection drops most rows


def _order(memories, entries):
    ids = [m.mem_id for m in memories]
    return [[ids[mi], row] for mi, row, _, _ in entries]


def _tagged(ci):
    memories = K.case_memories(ci)
    for m, spec in zip(memories, K.RECIPE["cases"][ci]["memories"]):
        m.mem_id = spec["id"]
    return memories


@pytest.mark.parametrize("ci", CASES, ids=NAMES)
def test_plans_give_the_references_rows_times_and_skipped_counts(ci):
    from hippomm_amd.consolidation import plan_audio_rows, plan_vision_rows
    want = GOLD["cases"][ci]
    for sort_first, part in ((False, want), (True, want["consolidated"])):   # the helpers alone, and behind the call's own sort
        memories = _tagged(ci)
        if sort_first:
            memories.sort(key=lambda m: m.segment_info.start_time)
            assert [m.mem_id for m in memories] == part["memory_order"]
        entries, skipped = plan_vision_rows(memories)
        v = part["vision"]
        assert skipped == v["skipped"]
        assert _order(memories, entries) == v.get("order", [])
        if "order" in v:
            assert np.array([e[3] for e in entries]).tolist() == v["times"]
            assert [entries[i][2] for i in v["kept"]] == v["frames"]
            assert np.array([e[3] for e in entries])[v["kept"]].tolist() == v["frame_times"]
        entries, skipped = plan_audio_rows(memories)
        a = part["audio"]
        assert skipped == a["skipped"]
        assert _order(memories, entries) == a.get("order", [])
        assert all(e[1] is None and e[2] is None for e in entries)
        if "order" in a:
            assert np.array([e[3] for e in entries]).tolist() == a["times"] == a["audio_times"]


def test_a_none_frame_time_raises_the_type_error_of_pythons_sort():
    from hippomm_amd.consolidation import plan_vision_rows
    block = np.zeros((2, 1024), np.float32)
    memory = types.SimpleNamespace(modalities=["vision"], features={"vision": block},
                                   content={"frames": ["a.jpg", "b.jpg"], "frame_times": [1.0, None]})
    with pytest.raises(TypeError):
        plan_vision_rows([memory])
    memory.content["frame_times"] = [1.0]                                    # one row: nothing is compared, nothing raises
    assert plan_vision_rows([memory]) == ([(0, 0, "a.jpg", 1.0)], 0)


def test_plans_touch_shapes_only():
    """A block is asked for its shape and nothing else: the plan works on objects that have no values."""
    from hippomm_amd.consolidation import plan_vision_rows
    import torch
    block = torch.empty((3, 1024), dtype=torch.float32, device="meta")
    memory = types.SimpleNamespace(modalities=["vision"], features={"vision": block},
                                   content={"frames": list("abcd"), "frame_times": [3.0, 1.0, 2.0, 0.0]})
    entries, skipped = plan_vision_rows([memory])
    assert [(e[1], e[2]) for e in entries] == [(1, "b"), (2, "c"), (0, "a")] and skipped == 1     # frame 3: the whole (3,1024) block


def _lib():
    from hippomm_amd import _lib, build
    build.build()
    return _lib.load()


def test_rows_gather_is_declared_exported_and_bound_and_the_abi_version_stays():
    from hippomm_amd import _lib, build
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hippomm_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(hmm_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(build.build()))
    assert "hmm_rows_gather" in declared and hasattr(raw, "hmm_rows_gather") and "hmm_rows_gather" in _lib._SIGNATURES
    assert _lib.load().hmm_abi_version() == 7
    import hippomm_amd
    assert hippomm_amd.consolidate_short_term_memory is hippomm_amd.consolidation.consolidate_short_term_memory


def test_rows_gather_argument_errors_are_reported_without_a_gpu():
    lib = _lib()

    def refused(*args, say):
        assert lib.hmm_rows_gather(*args) == HMM_E_INVALID, args
        msg = lib.hmm_last_error()
        assert b"rows_gather" in msg and say in msg, msg

    #       table, n, dim, out, stream
    refused(ONE, 5, 77, FAR, None, say=b"dim must be 1024")
    refused(None, 5, 1024, FAR, None, say=b"null pointer")
    refused(ONE, 5, 1024, None, None, say=b"null pointer")
    refused(ONE, -1, 1024, FAR, None, say=b"negative")
    refused(ONE, 5, 1024, FAR + 8, None, say=b"16-byte aligned")
    refused(ONE + 4, 5, 1024, FAR, None, say=b"8-byte aligned")
    refused(None, 0, 77, None, None, say=b"dim must be 1024")                # the shape is checked even when there is nothing to do


def test_rows_gather_of_no_rows_returns_ok_without_a_launch():
    """No GPU on this host: a launch would fail, HMM_OK means none was tried."""
    lib = _lib()
    assert lib.hmm_rows_gather(None, 0, 1024, None, None) == HMM_OK
    assert lib.hmm_rows_gather(ONE, 0, 1024, FAR + 4, None) == HMM_OK


def test_an_empty_list_consolidates_to_none_and_a_wrong_route_name_is_refused():
    from hippomm_amd import consolidate_short_term_memory
    assert consolidate_short_term_memory([]) is None
    with pytest.raises(ValueError):
        consolidate_short_term_memory([], features="gpu")


def test_the_generator_reproduces_the_committed_fixture():
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import make_golden
    if not (Path(make_golden.REF) / "hippomm" / "core" / "hippocampal_memory.py").exists():
        pytest.skip("the reference checkout is not on this machine")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "golden" / "make_consolidation_caller_golden.py"), "--check"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reproduced" in r.stdout
