"""Integration: the supervised CLI trains with --attention edges --centrality 4 end to end (fresh child processes,
capped steps): a finite loss, the reference's acc file, and the same text whether each batch's adjacency is built on the
device or on the host (the training batches' degrees are gathered on the GPU from the store's, the evaluation batches'
come from the host arrays)."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "graph-transformer_amd")


def _cli(mode, tmp_path):
    run = tmp_path / mode / "run" / "x"
    run.mkdir(parents=True)
    cmd = [sys.executable, os.path.join(PKG, "train_pytorch_U2GNN_Sup.py"), "--run_folder", str(run), "--num_epochs", "1",
           "--dataset", "MUTAG", "--model_name", "MUTAG", "--batch_size", "4", "--num_neighbors", "4",
           "--ff_hidden_size", "128", "--num_timesteps", "2", "--attention", "edges", "--centrality", "4",
           "--max_steps", "3", "--adjacency", mode]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, U2GNN_PARAM_CHECKSUM="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "centrality=4" in r.stdout and f"adjacency='{mode}'" in r.stdout     # the namespace the CLI prints first
    lines = [re.sub(r"time:\s*\S+", "time: -", x) for x in r.stdout.splitlines() if x.startswith("| epoch")]
    sums = [x for x in r.stderr.splitlines() if x.startswith("param_checksum rank ")]
    assert len(lines) == 1 and len(sums) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    return run, lines, sums


def test_sup_cli_mutag_centrality_under_both_adjacencies(tmp_path):
    run, lines, sums = _cli("device", tmp_path)
    m = re.search(r"\| epoch\s+1 \|.*\| loss\s+(\S+) \| test acc", lines[0])
    assert m, lines
    assert math.isfinite(float(m.group(1)))
    acc = run.parent / "runs_pytorch_U2GNN_Sup" / "MUTAG" / "checkpoints" / "model_acc.txt"
    assert acc.read_text().startswith("epoch 1 fold 1 acc ")
    assert _cli("host", tmp_path)[1:] == (lines, sums)
