"""Integration: the supervised CLI trains with --attention edges --hops 2 end to end (a fresh child process, capped
steps), prints a finite loss and writes the reference's acc file."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")


def test_sup_cli_mutag_hops(tmp_path):
    run = tmp_path / "run" / "x"
    run.mkdir(parents=True)
    cmd = [sys.executable, os.path.join(PKG, "train_pytorch_U2GNN_Sup.py"), "--run_folder", str(run), "--num_epochs", "1",
           "--dataset", "MUTAG", "--model_name", "MUTAG", "--batch_size", "4", "--num_neighbors", "4",
           "--ff_hidden_size", "128", "--num_timesteps", "2", "--attention", "edges", "--hops", "2",
           "--precision", "fwdh", "--max_steps", "3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "hops=2" in r.stdout                       # the argument namespace the CLI prints first
    m = re.search(r"\| epoch\s+1 \|.*\| loss\s+(\S+) \| test acc", r.stdout)
    assert m, r.stdout[-2000:]
    assert math.isfinite(float(m.group(1)))
    acc = run.parent / "runs_pytorch_U2GNN_Sup" / "MUTAG" / "checkpoints" / "model_acc.txt"
    assert acc.read_text().startswith("epoch 1 fold 1 acc ")
