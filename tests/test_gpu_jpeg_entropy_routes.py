"""GPU: the device entropy pass inside decode_jpeg, segment_sequence and vision_pipeline -- the tensors, errors, segments and
scores of the host entropy route, with the Huffman pass of every eligible frame on the GPU; a self-check mismatch turns the pass off for the process."""
import io
import logging

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_entropy_corpus as jc
from test_cpu_jpeg import encode, frame, pillow
from test_gpu_jpeg_routes import _scene_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fresh_entropy_check(monkeypatch):
    from hippomm_amd import jpeg
    monkeypatch.setitem(jpeg._entropy_check, "ok", None)
    monkeypatch.delenv("HMM_JPEG_ENTROPY", raising=False)


def _damaged_file_only_pillow_takes():
    """A case of the damage sweep that the prepare pass takes, the host entropy pass refuses and Pillow still decodes."""
    from hippomm_amd import jpeg
    for g, d in jc.damage_sweep():
        if jc.prepare(d, g)[0] == jpeg.DECODED and jc.host_slot(d, g, (0, 0, g[0], g[1]))[0] == jpeg.UNSUPPORTED:
            try:
                Image.open(io.BytesIO(d)).convert("RGB")
            except Exception:                                               # noqa: BLE001 - Pillow refuses it too: not this one
                continue
            return d
    raise AssertionError("the sweep holds no such file")


def test_decode_jpeg_with_the_device_entropy_pass_equals_the_host_route():
    from hippomm_amd import decode_jpeg
    corpus = [d for _, d in jc.corpus()]
    im = frame(64, 48, seed=2)
    mixed = corpus + [encode(im, quality=90, progressive=True), encode(im, quality=90, restart_marker_blocks=3),
                      _damaged_file_only_pillow_takes()]
    host_stats, dev_stats = {}, {}
    want = decode_jpeg(mixed, device="cuda", stats=host_stats, entropy="host")
    got = decode_jpeg(mixed, device="cuda", stats=dev_stats, entropy="device")
    assert "entropy_device" not in host_stats
    assert dev_stats["entropy_device"] == len(corpus)                       # every eligible frame, none left to the host pass
    assert {k: dev_stats[k] for k in ("device", "host")} == host_stats == {"device": len(corpus) + 1, "host": 2}
    assert len(got) == len(want) == len(mixed)
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), k
        np.testing.assert_array_equal(a.cpu().numpy(), pillow(mixed[k]))
    window = (5, 3, 30, 20)
    same = [encode(frame(64, 48, seed=s), quality=85, subsampling=2) for s in range(3)]
    assert torch.equal(decode_jpeg(same, device="cuda", window=window, entropy="device"),
                       decode_jpeg(same, device="cuda", window=window, entropy="host"))


def test_decode_jpeg_raises_the_same_errors_and_reads_the_switch_at_call_time(monkeypatch):
    from hippomm_amd import decode_jpeg
    good = jc.corpus()[3][1]
    raised = []
    for mode in ("host", "device"):
        with pytest.raises(Exception) as exc:
            decode_jpeg([good, b"not an image", good], device="cuda", entropy=mode)
        raised.append((type(exc.value), str(exc.value).split(" at 0x")[0]))
    assert raised[0] == raised[1]
    with pytest.raises(ValueError, match="HMM_JPEG_ENTROPY"):
        decode_jpeg([good], device="cuda", entropy="gpu")
    stats = {}
    monkeypatch.setenv("HMM_JPEG_ENTROPY", "device")
    decode_jpeg([good], device="cuda", stats=stats)
    assert stats == {"device": 1, "host": 0, "entropy_device": 1}
    monkeypatch.setenv("HMM_JPEG_ENTROPY", "host")
    decode_jpeg([good], device="cuda", stats=stats)
    assert stats["device"] == 1
    monkeypatch.delenv("HMM_JPEG_ENTROPY")
    stats = {}
    decode_jpeg([good], device="cuda", stats=stats)
    assert stats == {"device": 1, "host": 0}


def test_segment_sequence_is_bitwise_the_same_with_the_device_entropy_pass(tmp_path, monkeypatch):
    from hippomm_amd import jpeg
    from hippomm_amd.frame_cache import FrameCache, PathScorer
    from hippomm_amd.segmentation import segment_sequence
    paths = _scene_frames(tmp_path, 8, size=(160, 96), seed=5, cut_every=3)
    times = [float(i) for i in range(8)]
    kw = dict(max_segment_duration=4.0, min_segment_duration=1.0, frame_similarity_threshold=0.7)

    def run():
        seen = []
        real = jpeg._entropy_on_device

        def spy(jobs, *a, **k):
            out = real(jobs, *a, **k)
            seen.append((len(out), len(jobs)))
            return out
        monkeypatch.setattr(jpeg, "_entropy_on_device", spy)
        cache = FrameCache()
        segs = segment_sequence(paths, times, None, None, scorer=PathScorer(cache), **kw)
        monkeypatch.setattr(jpeg, "_entropy_on_device", real)
        assert cache.device_decodes >= 8
        # every adjacent pair and a few distant ones, scored from the frames this run's cache decoded: float64 bit patterns
        pairs = [(paths[i + 1], paths[i]) for i in range(7)] + [(paths[7], paths[0]), (paths[4], paths[2])]
        scores = np.array(list(PathScorer(cache).score(pairs)), dtype=np.float64)
        with cache.lock:
            loaded = cache.load(paths, torch.device("cuda"))
            frames = torch.stack([loaded[q][0].gray[loaded[q][1]] for q in paths]).cpu()
        return [(s.start_time, s.end_time, tuple(s.frames)) for s in segs], seen, scores, frames

    want, host_calls, want_scores, want_frames = run()
    monkeypatch.setenv("HMM_JPEG_ENTROPY", "device")
    got, dev_calls, got_scores, got_frames = run()
    assert got == want and len(want) >= 2
    assert got_scores.tobytes() == want_scores.tobytes() and np.isfinite(want_scores).all()      # bit for bit
    assert torch.equal(got_frames, want_frames)                                                   # the gray frames behind them
    assert host_calls == []                                                  # unset: the kernel route is not even entered
    assert sum(n for n, _ in dev_calls) >= 8 and all(n == jobs for n, jobs in dev_calls)


def test_vision_pipeline_is_bitwise_the_same_with_the_device_entropy_pass(tmp_path, monkeypatch):
    """6 paths of one size, one of them progressive (Pillow's route inside the ring) and one with a restart interval (the host
    entropy pass): the preprocessed tensors have the same bits with the switch set and unset, with and without a consumer, and
    the four eligible frames go through the kernel."""
    from hippomm_amd import preprocess
    paths = _scene_frames(tmp_path, 6, size=(320, 240), seed=9)
    Image.open(paths[2]).save(paths[2], quality=90, progressive=True)
    Image.open(paths[4]).save(paths[4], quality=90, restart_marker_blocks=4)

    def run(consume):
        stats, ranges = {}, []
        x = preprocess.vision_pipeline(paths, "cuda", (lambda t, lo, hi: ranges.append((lo, hi))) if consume else None,
                                       stats=stats, workers=3, upload_min=2)
        torch.cuda.synchronize()
        return x.cpu(), stats, ranges

    want, host_stats, host_ranges = run(False)
    want_c, _, _ = run(True)
    assert "entropy_device" not in host_stats and host_stats["device_decoded"] == 5
    monkeypatch.setenv("HMM_JPEG_ENTROPY", "device")
    got, stats, _ = run(False)
    got_c, stats_c, ranges = run(True)
    assert torch.equal(got, want) and torch.equal(got_c, want) and torch.equal(want_c, want)
    assert stats["entropy_device"] == stats_c["entropy_device"] == 4
    assert stats["device_decoded"] == 5
    assert ranges[0][0] == 0 and ranges[-1][1] == 6 and all(hi - lo >= 2 for lo, hi in ranges)   # the two-frame rule stands


def test_vision_pipeline_redoes_a_frame_the_entropy_kernel_refuses(tmp_path, monkeypatch):
    """A file the prepare pass takes and both entropy passes refuse (its scan is cut short before the EOI marker): the kernel
    flags it, _decode_file's route redoes it, and the tensors equal the host route's."""
    from hippomm_amd import jpeg, preprocess
    paths = _scene_frames(tmp_path, 4, size=(320, 240), seed=11)
    data = open(paths[1], "rb").read()
    end = data.rindex(b"\xff\xd9")
    cut = data[:end - 40] + data[end:]                                       # the last bytes of the scan are missing
    g = jpeg.parse(cut)
    assert jc.prepare(cut, g)[0] == jpeg.DECODED and jc.host_slot(cut, g, (0, 0, g[0], g[1]))[0] == jpeg.UNSUPPORTED
    open(paths[1], "wb").write(cut)
    want = preprocess.vision_pipeline(paths, "cuda", workers=2, upload_min=2).cpu()
    monkeypatch.setenv("HMM_JPEG_ENTROPY", "device")
    stats = {}
    got = preprocess.vision_pipeline(paths, "cuda", stats=stats, workers=2, upload_min=2).cpu()
    assert torch.equal(got, want)
    assert stats["entropy_device"] == 3 and stats["device_decoded"] == 3


def test_self_check_mismatch_turns_the_device_entropy_pass_off(monkeypatch, caplog):
    from hippomm_amd import decode_jpeg, jpeg
    monkeypatch.setattr(jpeg, "_slots_equal", lambda a, b: False)
    sources = [encode(frame(130, 90, seed=s), quality=90, subsampling=2) for s in range(4)]
    stats = {}
    with caplog.at_level(logging.WARNING, logger="hippomm_amd.jpeg"):
        got = decode_jpeg(sources, device="cuda", stats=stats, entropy="device")
    assert jpeg._entropy_check["ok"] is False
    assert "device entropy pass disagrees" in caplog.text
    assert stats == {"device": 4, "host": 0, "entropy_device": 0}
    for g, s in zip(got, sources):
        np.testing.assert_array_equal(g.cpu().numpy(), pillow(s))
    stats = {}
    decode_jpeg(sources, device="cuda", stats=stats, entropy="device")      # stays off for the process
    assert stats["entropy_device"] == 0
