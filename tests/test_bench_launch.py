"""bench.py --gpus N must never silently run a smaller job (VERDICT r5 'weak' 3): without a launcher it starts its own N
ranks, and it refuses — loudly, exit code 2 — when fewer than N devices are visible or when the launcher's WORLD_SIZE is
not N.  No GPU needed: this box has zero devices, so every N > 1 must be refused before anything renders."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RPT_BENCH_BACKEND")}
    env.update(kw)
    return env


def test_more_gpus_than_devices_is_refused_not_shrunk():
    import torch
    have = torch.cuda.device_count()
    n = have + 1 if have >= 1 else 2
    r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--steps", "1", "--warmup", "0"], capture_output=True,
                       text=True, env=_env(), timeout=600)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "refusing" in r.stderr and "--gpus %d" % n in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]  # no bench line under a false name


def test_world_size_that_is_not_gpus_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "1", "--warmup", "0"], capture_output=True,
                       text=True, env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=600)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    assert "does not match" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_self_launch_builds_one_rank_per_gpu(monkeypatch):
    """the command self_launch() runs: torch.distributed.run, --nproc-per-node N, loopback rendezvous, this file, the
    caller's own arguments"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setenv("RPT_BENCH_BACKEND", "gloo")  # (ranks may share a device: no device-count check)
    monkeypatch.setattr(sys, "argv", [BENCH, "--gpus", "8", "--steps", "5", "--warmup", "2"])

    class A:
        gpus = 8
    assert bench.self_launch(A()) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert os.path.samefile(cmd[cmd.index("--master-port") + 2], BENCH)
    assert cmd[-6:] == ["--gpus", "8", "--steps", "5", "--warmup", "2"]
    assert seen["env"]["RPT_BENCH_SELF_LAUNCHED"] == "1" and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_whole_small_frames_and_a_fixed_sample_of_large_ones(tmp_path):
    """--dump-outputs: a frame within the pixel limit is written whole as (H, W, 3) f32; a larger one as the same
    seeded sample of its pixels on every call; more than the byte limit in all is refused"""
    import numpy as np
    bench = _bench_module()
    W, H = 40, 30
    frame = np.random.default_rng(1).random(W * H * 3).astype(np.float32)
    whole = bench.frame_output(frame, W, H, W * H)
    assert whole.shape == (H, W, 3) and whole.dtype == np.float32 and (whole.reshape(-1) == frame).all()
    part = bench.frame_output(frame, W, H, 100)
    assert part.shape == (100, 3) and (part == bench.frame_output(frame.copy(), W, H, 100)).all()
    rows = frame.reshape(-1, 3)
    idx = [int(np.flatnonzero((rows == r).all(axis=1))[0]) for r in part]
    assert idx == sorted(set(idx))  # distinct pixels, in pixel order
    bench.dump_outputs(str(tmp_path / "d"), {"a": whole, "b": part})
    assert (np.load(str(tmp_path / "d" / "a.npy")) == whole).all() and (np.load(str(tmp_path / "d" / "b.npy")) == part).all()
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "e"), {"big": np.zeros(bench.DUMP_MAX_BYTES // 4 + 1, dtype=np.float32)})
    assert not (tmp_path / "e").exists()


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, env=_env(), timeout=600)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr[-500:]
