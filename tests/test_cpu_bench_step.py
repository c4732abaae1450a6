"""CPU: bench.py's launch logic and its step() at world_size 2 on gloo with stand-ins for the two GPU legs.

  * `--gpus N` with N > 1 and no torchrun environment self-launches; with fewer than N GPUs visible it must exit
    non-zero instead of silently running one rank; a rank whose WORLD_SIZE disagrees with --gpus refuses to run;
  * the synthetic video is the same whatever the sharding (frame i depends on i only);
  * make_step / timed_steps (the timed region of bench.py) under gloo: contiguous time shards of BASELINE cfg 5's shape,
    one all-gather, global selection == single-process selection on the gathered matrix; max-over-ranks timing.
The encoder leg is stood in by a fixed linear map of the frames, the selection leg by the oracle."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    sys.path.insert(0, str(ROOT))
    import bench
    return bench


def test_self_launch_refuses_when_gpus_are_missing():
    if torch.cuda.device_count() >= 2:
        pytest.skip("2+ GPUs visible")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 3 and "only" in r.stderr and not r.stdout.strip()


def test_rank_refuses_a_world_size_that_disagrees_with_gpus():
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "8"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 2 and "WORLD_SIZE=1" in r.stderr and not r.stdout.strip()


def test_synthetic_video_does_not_depend_on_the_sharding():
    bench = _bench()
    whole = bench.synthetic_frames(0, 20, "cpu")
    assert torch.equal(whole[7:15], bench.synthetic_frames(7, 15, "cpu"))
    assert torch.equal(whole[12:20], bench.synthetic_frames(12, 20, "cpu"))
    # frames of one scene are close, frames of different scenes are not
    flat = whole.flatten(1)
    flat = flat / flat.norm(dim=1, keepdim=True)
    sim = flat @ flat.T
    assert sim[0, 5] > 0.8 and sim[0, 6] < 0.5


def _encode_standin(frames):
    """(n,3,224,224) -> (n,1024): 16x16 average pooling of the pixels + a fixed random projection (deterministic, cheap)."""
    g = torch.Generator().manual_seed(123)
    proj = torch.randn(3 * 14 * 14, 1024, generator=g)
    pooled = torch.nn.functional.avg_pool2d(frames, 16).flatten(1)
    return pooled @ proj


def _worker(rank, world, port, n_frames, q):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import bench
        from hippomm_amd import sharding
        from oracle.consolidation_oracle import select_key_frames_oracle

        bounds = sharding.shard_bounds(n_frames, world)
        lo, hi = bounds[rank]
        counts = [b - a for a, b in bounds]
        frames = bench.synthetic_frames(lo, hi, "cpu")

        def select(f):
            return torch.from_numpy(select_key_frames_oracle(f.numpy(), None, 0.9).astype(np.int64))

        def reduce_max(x):
            t = torch.tensor([x], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())

        step = bench.make_step(frames, counts, _encode_standin, sharding.all_gather_embeddings, select)
        elapsed, (feats, kept) = bench.timed_steps(step, 2, 1, lambda: None, dist.barrier, reduce_max)
        full = _encode_standin(bench.synthetic_frames(0, n_frames, "cpu"))
        want = select_key_frames_oracle(full.numpy(), None, 0.9)
        q.put((rank, torch.equal(feats, full), kept.tolist() == want.tolist(), len(want), elapsed))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_frames", [45, 36])           # ragged (23 + 22) and even shards; scenes straddle the shard boundary
def test_bench_step_world2_gloo(n_frames):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() + n_frames) % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_frames, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    times = set()
    for rank, ok_feats, ok_kept, n_kept, elapsed in results:
        assert ok_feats, f"rank {rank}: gathered matrix != single-process matrix"
        assert ok_kept, f"rank {rank}: kept indices != single-process selection"
        assert 1 < n_kept < n_frames, "the synthetic video must make the selection drop some frames and keep several"
        times.add(round(elapsed, 9))
    assert len(times) == 1, "every rank must report the max-over-ranks time"


def test_gpu_count_comes_from_sysfs_not_from_hip(tmp_path, monkeypatch):
    """The self-launching parent counts GPUs from the KFD topology (nodes with SIMDs), narrowed by *_VISIBLE_DEVICES."""
    import bench
    for i, simd in enumerate((0, 256, 256, 256)):                # node 0 is the CPU agent
        d = tmp_path / str(i)
        d.mkdir()
        (d / "properties").write_text(f"cpu_cores_count {64 if simd == 0 else 0}\nsimd_count {simd}\nmem_banks_count 1\n")
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    none = str(tmp_path / "no_dri")
    assert bench.visible_gpu_count(str(tmp_path), none) == 3
    # a container maps only its own GPUs' render nodes: the host's other cards are in the topology but not usable
    dri = tmp_path / "dri"
    dri.mkdir()
    for i, minor in ((1, 128), (2, 129), (3, 130)):
        p = tmp_path / str(i) / "properties"
        p.write_text(p.read_text() + f"drm_render_minor {minor}\n")
    (dri / "renderD129").write_text("")
    assert bench.visible_gpu_count(str(tmp_path), str(dri)) == 1
    (dri / "renderD128").write_text("")
    assert bench.visible_gpu_count(str(tmp_path), str(dri)) == 2
    import functools
    monkeypatch.setattr(bench, "visible_gpu_count", functools.partial(bench.visible_gpu_count, dri=none))
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,2")
    assert bench.visible_gpu_count(str(tmp_path)) == 2
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "1")
    assert bench.visible_gpu_count(str(tmp_path)) == 1
    assert bench.visible_gpu_count(str(tmp_path / "absent")) == 0


def test_self_launch_kills_ranks_that_hang(monkeypatch, tmp_path, capsys):
    """launch_ranks gives the ranks a wall-clock limit: a group that does not finish (a rank stuck in a collective) is killed --
    children and grandchildren, they are a process group of their own -- and the run returns non-zero instead of hanging."""
    import time
    import bench
    marker = tmp_path / "grandchild.pid"
    script = tmp_path / "hang.py"
    script.write_text("import os, subprocess, sys, time\n"
                      f"p = subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(600)'])\n"
                      f"open({str(marker)!r}, 'w').write(str(p.pid))\n"
                      "time.sleep(600)\n")
    monkeypatch.setenv("HMM_BENCH_REHEARSAL", "1")
    monkeypatch.setattr(bench, "REHEARSAL", True)                       # no GPU count needed
    monkeypatch.setenv("HMM_BENCH_LAUNCH_TIMEOUT_S", "3")
    real_popen = bench.subprocess.Popen
    monkeypatch.setattr(bench.subprocess, "Popen",
                        lambda cmd, **kw: real_popen([bench.sys.executable, str(script)], **kw))   # stand-in for torch.distributed.run
    t0 = time.time()
    rc = bench.launch_ranks(2, ["--gpus", "2"])
    assert rc == 5 and time.time() - t0 < 30
    assert "did not finish within 3 s" in capsys.readouterr().err
    pid = int(marker.read_text())
    for _ in range(50):                                                  # the grandchild went with the group
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            break
        time.sleep(0.1)
    else:
        raise AssertionError("a grandchild of the killed launch is still alive")


def test_self_launch_takes_the_ranks_along_when_the_parent_is_terminated(tmp_path):
    """The ranks run in a session of their own, so a SIGTERM to the parent (an outer `timeout`, the driver) does not reach them
    by itself: launch_ranks turns it into an exception and kills the group on every way out."""
    import signal
    import subprocess
    import sys
    import time
    marker = tmp_path / "rank.pid"
    hang = tmp_path / "hang.py"
    hang.write_text(f"import os, time\nopen({str(marker)!r}, 'w').write(str(os.getpid()))\ntime.sleep(600)\n")
    parent = tmp_path / "parent.py"
    parent.write_text("import os, sys\n"
                      f"sys.path.insert(0, {str(Path(__file__).resolve().parent.parent)!r})\n"
                      "os.environ['HMM_BENCH_REHEARSAL'] = '1'\n"
                      "import bench\n"
                      "real = bench.subprocess.Popen\n"
                      f"bench.subprocess.Popen = lambda cmd, **kw: real([sys.executable, {str(hang)!r}], **kw)\n"
                      "sys.exit(bench.launch_ranks(2, ['--gpus', '2']))\n")
    p = subprocess.Popen([sys.executable, str(parent)], stderr=subprocess.PIPE, text=True)
    for _ in range(600):
        if marker.exists() and marker.read_text():
            break
        time.sleep(0.1)
    else:
        p.kill()
        raise AssertionError("the stand-in rank never started")
    p.send_signal(signal.SIGTERM)
    _, err = p.communicate(timeout=60)
    assert p.returncode == 130 and "killing the ranks' process group" in err
    pid = int(marker.read_text())
    for _ in range(100):
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            break
        time.sleep(0.1)
    else:
        raise AssertionError("the rank outlived its terminated parent")


def test_dump_outputs_writes_the_step_result_and_samples_rows_beyond_the_limit(tmp_path):
    """--dump-outputs: embeddings as float32, kept indices as float64; a matrix over the size limit is replaced by the same
    seeded sample of rows every time, named in embedding_rows.npy, and the files stay under the limit."""
    bench = _bench()
    feats = torch.randn(300, 1024, generator=torch.Generator().manual_seed(5))
    kept = torch.tensor([0, 7, 120, 299], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "all"), feats, kept)
    assert sorted(f.name for f in (tmp_path / "all").iterdir()) == ["embeddings.npy", "kept_indices.npy"]
    emb = np.load(tmp_path / "all" / "embeddings.npy")
    idx = np.load(tmp_path / "all" / "kept_indices.npy")
    assert emb.dtype == np.float32 and np.array_equal(emb, feats.numpy())
    assert idx.dtype == np.float64 and idx.tolist() == [0, 7, 120, 299]

    limit = 100 * 4096
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), feats, kept, limit_bytes=limit)
        assert sum(f.stat().st_size for f in (tmp_path / name).iterdir()) <= limit
    rows = np.load(tmp_path / "a" / "embedding_rows.npy")
    assert 50 < len(rows) < 100 and np.array_equal(np.load(tmp_path / "a" / "kept_indices.npy"), idx)
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "embedding_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "embeddings.npy"), feats.numpy()[rows.astype(np.int64)])
