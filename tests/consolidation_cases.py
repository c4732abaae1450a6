"""Consolidation-caller cases shared by tests/test_cpu_consolidation_caller.py, tests/test_gpu_consolidation_caller.py and the
fixture's generator (tests/golden/make_consolidation_caller_golden.py): the recipe of
tests/golden/consolidation_caller_golden.json and the helpers that build a case's memories and rebuild a stacked matrix from it.

No feature value is stored anywhere: every block is drawn from the seed.  A row is the centre of its planted cluster plus noise of
0.05 per component, so two rows of one cluster have a cosine near 0.9975 and two rows of different clusters one near 0 (1024
components): every comparison the selection makes is about 0.1 away from the threshold of 0.9."""
from __future__ import annotations

import hashlib
import json
import types
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "consolidation_caller_golden.json"
SEED = 20261020
NOISE = 0.05
N_CENTRES = 8
MIN_MARGIN = 1e-3                    # the generator refuses a case whose selection compares a similarity closer to 0.9 than this


def _mem(id, start, end, *, vision=None, frames=None, frame_times=None, audio=None, modalities=("vision", "audio"), transcription=()):
    return {"id": id, "start": start, "end": end, "timestamp": 1700000000.5 + 10 * id, "source_time": start + 0.125,
            "modalities": list(modalities), "vision": vision, "frames": frames, "frame_times": frame_times, "audio": audio,
            "transcription": list(transcription)}


def _vis(shape, clusters, kind="numpy"):
    return {"shape": list(shape), "kind": kind, "clusters": list(clusters)}


def _aud(shape, cluster, start_time, end_time, kind="numpy"):
    return {"shape": list(shape), "kind": kind, "clusters": [cluster] * (int(np.prod(shape)) // 1024), "start_time": start_time,
            "end_time": end_time}


def _say(t0, t1, text):
    return {"start": t0, "end": t1, "text": text}


def _sixty():
    """About 60 rows in 6 clusters, 6 segments of 10 rows handed over out of time order; within a segment the clusters alternate, so
    the selection meets every cluster early and drops most rows."""
    order = [3, 0, 5, 1, 4, 2]
    mems = []
    for s in order:
        t0 = 10.0 * s
        mems.append(_mem(s, t0, t0 + 10.0, vision=_vis((10, 1024), [(s + j) % 6 for j in range(10)]), frames=10,
                         frame_times=[t0 + j for j in range(10)], audio=_aud((1, 1024), s % 6, t0, t0 + 10.0),
                         transcription=[_say(t0, t0 + 10.0, f"segment {s}")]))
    return mems


RECIPE = {
    "seed": SEED,
    "cases": [
        # memories out of time order; frame times tied across memories (2.0 twice, 3.0 twice); audio as (1,1024) and (1024,)
        {"name": "out_of_order_ties", "memories": [
            _mem(0, 4.0, 6.0, vision=_vis((2, 1024), [2, 0]), frames=2, frame_times=[4.0, 3.0], audio=_aud((1024,), 1, 4.0, 6.0),
                 transcription=[_say(4.0, 6.0, "third — 你好")]),
            _mem(1, 0.0, 2.0, vision=_vis((3, 1024), [0, 0, 1]), frames=3, frame_times=[0.0, 1.0, 2.0], audio=_aud((1, 1024), 0, 0.0, 2.0),
                 transcription=[_say(0.0, 2.0, "first")]),
            _mem(2, 2.0, 4.0, vision=_vis((2, 1024), [1, 2]), frames=2, frame_times=[2.0, 3.0], audio=_aud((1, 1024), 1, 2.0, 4.0))]},
        # a one-row block with two frames, a 1-D block, more frames than times
        {"name": "one_row_blocks_and_short_times", "memories": [
            _mem(0, 0.0, 2.0, vision=_vis((1, 1024), [0]), frames=2, frame_times=[0.0, 1.5], audio=_aud((1, 1024), 3, 0.0, 2.0)),
            _mem(1, 2.0, 3.0, vision=_vis((1024,), [1]), frames=1, frame_times=[2.0], modalities=("vision",)),
            _mem(2, 3.0, 6.0, vision=_vis((4, 1024), [1, 2, 2, 3]), frames=4, frame_times=[3.0, 4.0, 5.0], audio=_aud((1024,), 2, 3.0, 6.0),
                 transcription=[_say(3.0, 6.0, "kept")])]},
        # more frames than rows: frame 2 of a two-row block yields the whole (2,1024) matrix and is skipped; an audio block of two
        # rows is skipped as well, and its memory's transcription with it
        {"name": "more_frames_than_rows", "memories": [
            _mem(0, 0.0, 3.0, vision=_vis((2, 1024), [0, 1]), frames=3, frame_times=[0.0, 1.0, 2.0], audio=_aud((2, 1024), 0, 0.0, 3.0),
                 transcription=[_say(0.0, 3.0, "lost with its audio block")]),
            _mem(1, 3.0, 5.0, vision=_vis((2, 1024), [1, 2]), frames=2, frame_times=[3.0, 4.0], audio=_aud((1, 1024), 1, 3.0, 5.0),
                 transcription=[_say(3.0, 5.0, "stays")])]},
        # torch tensors, as the encoder hands them over
        {"name": "tensor_blocks", "memories": [
            _mem(0, 2.0, 4.0, vision=_vis((3, 1024), [1, 1, 0], "tensor"), frames=3, frame_times=[2.0, 2.5, 3.0],
                 audio=_aud((1, 1024), 4, 2.0, 4.0, "tensor")),
            _mem(1, 0.0, 2.0, vision=_vis((2, 1024), [0, 1], "tensor"), frames=2, frame_times=[0.0, 1.0], audio=_aud((1024,), 5, 0.0, 2.0, "tensor")),
            _mem(2, 4.0, 5.0, vision=_vis((1, 1024), [2], "tensor"), frames=1, frame_times=[4.0], audio=_aud((1, 1024), 4, 4.0, 5.0))]},
        {"name": "audio_only", "memories": [
            _mem(0, 1.0, 2.0, audio=_aud((1, 1024), 0, 1.0, 2.0), modalities=("audio",), transcription=[_say(1.0, 2.0, "b")]),
            _mem(1, 0.0, 1.0, audio=_aud((1024,), 1, 0.0, 1.0), modalities=("audio",), transcription=[_say(0.0, 1.0, "a")])]},
        {"name": "vision_only", "memories": [
            _mem(0, 0.0, 2.0, vision=_vis((2, 1024), [0, 1]), frames=2, frame_times=[0.0, 1.0], modalities=("vision",)),
            _mem(1, 2.0, 4.0, vision=_vis((2, 1024), [1, 1]), frames=2, frame_times=[2.0, 3.0], modalities=("vision",))]},
        # vision named but nothing to stack: the reference's empty dicts
        {"name": "nothing_to_stack", "memories": [
            _mem(0, 0.0, 1.0, vision=_vis((2, 1024), [0, 1]), modalities=("vision",)),
            _mem(1, 1.0, 2.0, vision=_vis((2, 1024), [0, 1]), frames=2, frame_times=[], modalities=("vision",))]},
        {"name": "n_is_1", "memories": [
            _mem(0, 0.0, 1.0, vision=_vis((1, 1024), [0]), frames=1, frame_times=[0.5], audio=_aud((1, 1024), 0, 0.0, 1.0))]},
        # two rows of one cluster: both kept without a comparison
        {"name": "n_is_2", "memories": [
            _mem(0, 0.0, 1.0, vision=_vis((2, 1024), [0, 0]), frames=2, frame_times=[0.0, 0.5], audio=_aud((1, 1024), 0, 0.0, 1.0)),
            _mem(1, 1.0, 2.0, audio=_aud((1, 1024), 0, 1.0, 2.0), modalities=("audio",))]},
        # three rows of one cluster: the first comparison happens, one row stays
        {"name": "n_is_3", "memories": [
            _mem(0, 1.0, 2.0, vision=_vis((1, 1024), [0]), frames=1, frame_times=[1.0], modalities=("vision",)),
            _mem(1, 0.0, 1.0, vision=_vis((2, 1024), [0, 0]), frames=2, frame_times=[0.0, 0.5], modalities=("vision",))]},
        {"name": "sixty_rows_six_clusters", "memories": _sixty()},
    ],
}


def case_index(name: str) -> int:
    return [c["name"] for c in RECIPE["cases"]].index(name)


def block(ci: int, mem_id: int, which: int, spec) -> np.ndarray:
    """The fp32 block of memory `mem_id` of case `ci` (which: 0 vision, 1 audio), a function of the seed alone."""
    centres = np.random.default_rng([SEED, ci, 7]).standard_normal((N_CENTRES, 1024))
    noise = np.random.default_rng([SEED, ci, mem_id, which]).standard_normal((len(spec["clusters"]), 1024))
    return (centres[spec["clusters"]] + NOISE * noise).astype(np.float32).reshape(spec["shape"])


def _as_given(a: np.ndarray, spec, mem_id: int, which: int):
    if spec["kind"] == "tensor":
        import torch
        return torch.from_numpy(a)
    return a


def case_memories(ci: int, memory=None, segment=None, convert=_as_given):
    """The memories of case `ci` in the caller's order.  memory / segment: constructors taking the reference's field names as
    keywords (default: plain namespaces).  convert(block, spec, mem_id, which) says in what form a block is handed over."""
    memory = memory or (lambda **k: types.SimpleNamespace(**k))
    segment = segment or (lambda **k: types.SimpleNamespace(**k))
    case = RECIPE["cases"][ci]
    out = []
    for m in case["memories"]:
        features, content = {}, {}
        if m["vision"] is not None:
            features["vision"] = convert(block(ci, m["id"], 0, m["vision"]), m["vision"], m["id"], 0)
        if m["frames"] is not None:
            content["frames"] = [f"frames/{case['name']}/{m['id']:02d}_{j:03d}.jpg" for j in range(m["frames"])]
        if m["frame_times"] is not None:
            content["frame_times"] = list(m["frame_times"])
        if m["audio"] is not None:
            features["audio"] = convert(block(ci, m["id"], 1, m["audio"]), m["audio"], m["id"], 1)
            content["audio"] = {"start_time": m["audio"]["start_time"], "end_time": m["audio"]["end_time"]}
        out.append(memory(features=features, content=content, timestamp=m["timestamp"], source_time=m["source_time"],
                          modalities=list(m["modalities"]), segment_info=segment(start_time=m["start"], end_time=m["end"]),
                          transcription=[dict(t) for t in m["transcription"]]))
    return out


def rows_by_bytes(ci: int, which: int) -> dict:
    """The bytes of every 1024-float row a case can stack -> [memory id, row index or None for "the whole block"]."""
    table = {}
    for m in RECIPE["cases"][ci]["memories"]:
        spec = m["vision" if which == 0 else "audio"]
        if spec is None:
            continue
        a = block(ci, m["id"], which, spec)
        if a.size == 1024:
            table[a.tobytes()] = [m["id"], None]
        elif a.ndim == 2 and a.shape[1] == 1024:
            for r in range(a.shape[0]):
                table[a[r].tobytes()] = [m["id"], r]
    return table


def rebuild(ci: int, which: int, order) -> np.ndarray:
    """The stacked matrix from the recipe: row i is the block row order[i] = [memory id, row index or None] names."""
    specs = {m["id"]: m["vision" if which == 0 else "audio"] for m in RECIPE["cases"][ci]["memories"]}
    rows = []
    for mem_id, r in order:
        a = block(ci, mem_id, which, specs[mem_id])
        rows.append(a.reshape(-1) if r is None else a[r])
    return np.stack(rows)


def digest(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def golden():
    return json.loads(GOLDEN.read_text())
