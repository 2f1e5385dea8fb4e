"""bench.py on the GPU: a plain run times --steps steps, reports ms_per_step and none of the --full objects, and
--dump-outputs writes what the last timed step left (loss, flat parameters, flat gradients) as float32 arrays
(c5: more than the budget, so the seeded sample); --full adds its objects, each under its own switch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        *extra], capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


OTHERS_OFF = ["--cpu-baseline", "0", "--pipeline-steps", "0", "--configs", "0", "--neighbors-line", "0"]
POLICIES = ("fp32", "fwd32", "bf16x3", "fwd6")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["probes", "no-roofline"])
def test_full_adds_its_objects_under_their_switches(case):
    """--full measures what a plain run leaves out.  --no-roofline switches the live attention probes off and leaves
    the gather roofline on (the profiling scripts rely on its launches); --fp32-steps 0 drops the policy lines."""
    if case == "probes":
        d = _bench("--full", "--fp32-steps", "0", *OTHERS_OFF)
        r = d["roofline"]
        assert r["bound"] == "mfma" and r["launches"] == 3 * 4 and r["avg_launch_us"] > 0
        assert sorted(r["other_kernels"]) == ["dq", "dv", "pv", "qk"]
        assert not any(k in d for k in POLICIES)
    else:
        d = _bench("--full", "--no-roofline", "--fp32-steps", "2", *OTHERS_OFF)
        assert d["roofline"] is None
        for k in POLICIES:
            assert d[k]["steps"] == 2 and d[k]["ms_per_step"] > 0
    g = d["gather"]
    assert g["bound"] == "hbm" and g["avg_launch_us"] > 0 and g["rows"] > 0 and g["achieved"] > 0
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["cpu_baseline"] is None
    assert not any(k in d for k in ("pipeline", "c5", "c2", "c3", "neighbors"))


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["c4", "c2", "c5"])
def test_plain_run_line_and_dump(tmp_path, workload):
    d = _bench("--workload", workload, "--dump-outputs", str(tmp_path / "out"))
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "graphs/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0
    bs = 64 if workload == "c4" else 4
    assert d["value"] == pytest.approx(bs / (d["ms_per_step"] * 1e-3), rel=1e-2)
    assert d["cpu_baseline"] is None and d.get("gather") is None
    assert not any(k in d for k in ("fp32", "fwd32", "pipeline", "c5", "c2", "c3", "neighbors"))
    if workload == "c4":
        assert d["roofline"] is None
    if workload == "c5":
        assert d["optimizer"] is None and d["attention_kernel"] is None
    out = {k: np.load(tmp_path / "out" / f"{k}.npy") for k in ("loss", "params", "grads")}
    assert sorted(os.listdir(tmp_path / "out")) == ["grads.npy", "loss.npy", "params.npy"]
    assert all(a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all() for a in out.values())
    assert out["loss"].shape == (1,) and float(out["loss"][0]) == pytest.approx(d["final_loss"], abs=1e-4)
    assert out["params"].shape == out["grads"].shape and out["params"].size > 1000
    assert np.abs(out["grads"]).max() > 0
    total = sum(a.nbytes for a in out.values())
    assert total <= 64 * 10 ** 6
    if workload == "c5":   # the dense [V, 4] table and its gradient: ~80 MB, cut to nearly the whole budget
        assert total > 63 * 10 ** 6
