"""GPU: the device JSON writer (hmm_json_write_matrix_device behind event_store.matrix_json_bytes / event_json_bytes /
save_event(matrices="device")) writes the bytes of json.dumps -- per matrix at every seam of its launch plan, and per event file."""
import json
import logging
from pathlib import Path

import numpy as np
import pytest
import torch

import event_json_cases as jc
import recipes

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "event_golden.json"
G = jc.VALUES_PER_GROUP
SHAPES = [(1, 1), (1, 2), (3, 5), (2, 1024), (1025, 1), (33, 257),
          (1, G - 1), (2, G // 2), (1, G + 1),                    # one below, exactly at and one above a workgroup's values
          (5, (jc.VALUES_PER_SCAN_ROUND + 1) // 5)]                # one above a round of the scan of the workgroups' sums
assert jc.VALUES_PER_SCAN_ROUND % 5 == 4, "the last shape is meant to hold VALUES_PER_SCAN_ROUND + 1 values"


@pytest.fixture(autouse=True)
def _fresh_route():
    """Every test starts with the route on and the self-check already passed, unless it says otherwise."""
    from hippomm_amd import event_store as es
    es._device_route["on"], es._device_check["ok"] = True, True
    yield
    es._device_route["on"], es._device_check["ok"] = True, None


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matrix_bytes_at_every_seam(shape, dtype):
    from hippomm_amd import event_store as es
    m = jc.alternating(shape, dtype)
    on_device = torch.from_numpy(m).cuda()
    for close_indent in (0, 4, 7):
        want = jc.matrix_text(m, close_indent)
        stats = {}
        got = es.matrix_json_bytes(m, close_indent, stats=stats)
        assert stats == {"route": "device"}
        assert got == want, (close_indent, len(got), len(want), next(i for i, (a, b) in enumerate(zip(got + b"\0", want + b"\0")) if a != b))
        assert es.matrix_json_bytes(on_device, close_indent) == want, close_indent
    if shape == (3, 5):
        assert want.decode() == es._matrix_text(m.tolist()).replace("\n", "\n   ")      # the host writer's text, three spaces deeper


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_odd_values_at_the_edges_of_a_workgroups_range(dtype):
    from hippomm_amd import event_store as es
    m = jc.odd_at_group_edges(dtype)
    assert es.matrix_json_bytes(m, 4) == jc.matrix_text(m, 4)


def test_a_non_contiguous_matrix_is_made_contiguous():
    from hippomm_amd import event_store as es
    base = np.random.default_rng(4).standard_normal((40, 70)).astype(np.float32)
    want = jc.matrix_text(np.ascontiguousarray(base.T[::2]), 4)
    assert es.matrix_json_bytes(base.T[::2], 4) == want
    assert es.matrix_json_bytes(torch.from_numpy(base).cuda().T[::2], 4) == want


# ---- event files --------------------------------------------------------------------------------------------------------------------
def _sidecars(json_path):
    return {p.name: p.read_bytes() for p in sorted(json_path.parent.glob(json_path.stem + ".*.npy"))}


@pytest.mark.parametrize("where", ["numpy", "cuda"])
def test_golden_event_file(tmp_path, where):
    from hippomm_amd import event_store as es
    case = recipes.event_case()
    feats = {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if where == "cuda" and not k.endswith("_times") else v)
             for k, v in case["features"].items()}
    event = dict(case, features=feats)
    stats = {}
    host = es.save_event(case, tmp_path / "host" / "e.json")
    dev = es.save_event(event, tmp_path / "dev" / "e.json", matrices="device", stats=stats)
    assert stats == {"device": 2, "host": 0}
    assert dev.read_bytes() == GOLD.read_bytes() == es.event_json_text(case).encode("ascii")
    assert _sidecars(dev) == _sidecars(host) and len(_sidecars(dev)) == 2
    got = es.load_event_features(dev)
    for modality in ("vision", "audio"):
        np.testing.assert_array_equal(got[modality], case["features"][modality])
    # the default route is the parent commit's call: same file, same sidecars
    assert es.save_event(case, tmp_path / "host2" / "e.json", matrices="host").read_bytes() == host.read_bytes() == GOLD.read_bytes()


def test_mixed_event(tmp_path):
    """A device matrix beside everything the host path has to keep: a 1-D feature, an empty matrix, an integer list, a list of
    float rows and a *_times entry -- NaN, inf, -0.0 and a denormal-range value inside the device matrix."""
    from hippomm_amd import event_store as es
    case = recipes.event_case()
    rng = np.random.default_rng(5)
    v = rng.standard_normal((37, 1024)).astype(np.float32)
    v[3, 5], v[4, 5], v[7, 7], v[8, 7], v[9, 0] = np.nan, np.inf, 1e-30, -0.0, 123456792.0
    feats = {"vision": v, "vision_times": np.arange(37) * 0.5, "audio": np.zeros((0, 1024), np.float32), "audio_times": [],
             "depth": rng.standard_normal(1024).astype(np.float32), "ints": [[1, 2], [3, 4]], "rows": [[0.5, 1.5], [2.5, 3.5]],
             "wide": rng.standard_normal((2, 3))}
    host_event = dict(case, features=feats)
    dev_event = dict(case, features=dict(feats, vision=torch.from_numpy(v).cuda(), wide=torch.from_numpy(feats["wide"]).cuda()))
    want = json.dumps(es.event_to_dict(host_event), indent=2).encode("ascii")
    stats = {}
    assert es.event_json_bytes(dev_event, stats=stats) == want and stats == {"device": 2, "host": 0}
    assert es.event_json_bytes(host_event, matrices="device") == want
    a = es.save_event(host_event, tmp_path / "a" / "e.json")
    b = es.save_event(dev_event, tmp_path / "b" / "e.json", matrices="device")
    assert a.read_bytes() == b.read_bytes() == want
    assert _sidecars(a) == _sidecars(b) and len(_sidecars(a)) == 6


def test_a_token_in_the_events_own_strings_sends_the_whole_event_to_json(monkeypatch):
    from hippomm_amd import event_store as es

    class _Fixed:
        hex = "0" * 32
    monkeypatch.setattr(es.uuid, "uuid4", lambda: _Fixed)
    case = recipes.event_case()
    event = dict(case, summary="@@hmm_matrix_0_" + "0" * 32 + "@@",
                 features={k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if not k.endswith("_times") else v)
                           for k, v in case["features"].items()})
    assert es.event_json_bytes(event) == json.dumps(es.event_to_dict(dict(case, summary=event["summary"])), indent=2).encode("ascii")


# ---- self-check ---------------------------------------------------------------------------------------------------------------------
def test_self_check_passes_on_the_first_matrix_and_runs_once(monkeypatch):
    from hippomm_amd import event_store as es
    es._device_check["ok"] = None
    calls = []
    real = es._device_text_agrees
    monkeypatch.setattr(es, "_device_text_agrees", lambda *a: calls.append(1) or real(*a))
    m = jc.alternating((3, 5), np.float32)
    for _ in range(2):
        assert es.matrix_json_bytes(torch.from_numpy(m).cuda(), 4) == jc.matrix_text(m, 4)
    assert calls == [1] and es._device_check["ok"] is True


def test_a_failed_self_check_turns_the_route_off_and_the_file_is_still_the_references(monkeypatch, tmp_path, caplog):
    from hippomm_amd import event_store as es
    es._device_check["ok"] = None
    monkeypatch.setattr(es, "_device_text_agrees", lambda *a: False)
    case = recipes.event_case()
    event = dict(case, features={k: (torch.from_numpy(np.ascontiguousarray(v)).cuda() if k == "vision" else v)
                                 for k, v in case["features"].items()})
    stats = {}
    with caplog.at_level(logging.WARNING, logger="hippomm_amd.event_store"):
        path = es.save_event(event, tmp_path / "e.json", matrices="device", stats=stats)
    assert path.read_bytes() == GOLD.read_bytes()
    assert stats == {"device": 0, "host": 2} and es._device_check["ok"] is False
    assert any("disagrees" in r.getMessage() for r in caplog.records)
    one = {}
    assert es.matrix_json_bytes(case["features"]["vision"], 4, stats=one) == jc.matrix_text(case["features"]["vision"], 4)
    assert one == {"route": "host"}
