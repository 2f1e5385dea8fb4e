"""bench.py's launcher contract on CPU (no GPU is touched): `--gpus N` without a launcher starts
torch.distributed.run with N ranks as a child process and relays their lines; inside a launcher,
WORLD_SIZE must equal --gpus."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env.update(kw)
    return env


def test_gpus_2_spawns_two_ranks():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--launch-check"],
                       capture_output=True, text=True, timeout=300, env=_env(), cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert sorted(x["rank"] for x in lines) == [0, 1]
    assert all(x["world"] == 2 and x["launch_check"] for x in lines)


def test_world_size_must_match_gpus():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--launch-check"],
                       capture_output=True, text=True, timeout=300, env=_env(WORLD_SIZE="2", RANK="0"), cwd=REPO)
    assert p.returncode != 0
    assert "WORLD_SIZE=2 but --gpus 1" in p.stderr


def test_plain_run_is_the_default():
    """--full and --dump-outputs are off unless asked for; --steps sets the timed steps."""
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = bench.parse()
        sys.argv = ["bench.py", "--full", "--dump-outputs", "d", "--cpu-baseline", "0"]
        b = bench.parse()
    finally:
        sys.argv = argv
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    assert (b.full, b.dump_outputs, b.cpu_baseline) == (True, "d", 0)


def test_dump_outputs_float32_within_budget_and_repeatable(tmp_path, monkeypatch):
    """--dump-outputs: one float32 .npy per array; whole arrays within the byte budget, beyond it the same fraction
    of every array at positions that do not change from run to run (in their original order)."""
    import numpy as np
    import torch

    import bench
    arrays = {"loss": torch.tensor([1.5]), "params": torch.arange(3000, dtype=torch.float64) / 7,
              "grads": -torch.arange(1000, dtype=torch.float32).reshape(10, 100)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, t in arrays.items():
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == (t.numel(),)
        np.testing.assert_array_equal(a, t.reshape(-1).to(torch.float32).numpy())
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    total = 0
    for k, t in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, b)
        total += a.nbytes
        full = t.reshape(-1).to(torch.float32).numpy()
        if k != "loss":   # strictly monotone arrays: a sample in the original order is monotone, and a subset
            assert 0 < a.size < full.size and np.all(np.diff(np.abs(a)) > 0) and np.isin(a, full).all()
    assert total <= 4000
