"""bench.py --dump-outputs: what the last timed step hands its caller, written as float32 / float64 .npy files (no GPU)."""
import importlib.util
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _job():
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 300), torch.nn.BatchNorm1d(300))
    return types.SimpleNamespace(model=model, last_out=torch.randn(4, 51))


def test_loss_logits_and_state_are_written_whole(tmp_path):
    bench, job = _bench(), _job()
    total = bench.dump_outputs(str(tmp_path), job, torch.tensor(2.5))
    names = sorted(os.listdir(tmp_path))
    assert "loss.npy" in names and "logits.npy" in names and "state.0.weight.npy" in names
    assert "state.1.num_batches_tracked.npy" in names and "state.1.running_var.npy" in names
    for n in names:
        assert np.load(tmp_path / n).dtype in (np.float32, np.float64), n
    assert np.array_equal(np.load(tmp_path / "state.0.weight.npy"), job.model[0].weight.detach().numpy())
    assert np.load(tmp_path / "logits.npy").shape == (4, 51) and float(np.load(tmp_path / "loss.npy")) == 2.5


def test_a_dump_over_budget_keeps_the_same_seeded_sample(tmp_path):
    bench, job = _bench(), _job()
    bench.DUMP_BYTES, bench.DUMP_SAMPLE = 40000, 1000  # the Linear's weight (19200 elements) does not fit whole
    a, b = tmp_path / "a", tmp_path / "b"
    assert bench.dump_outputs(str(a), job, torch.tensor(1.0)) <= 40000
    bench.dump_outputs(str(b), job, torch.tensor(1.0))
    w = np.load(a / "state.0.weight.npy")
    assert w.shape == (1000,) and np.array_equal(w, np.load(b / "state.0.weight.npy"))
    assert set(w.tolist()) <= set(job.model[0].weight.detach().numpy().reshape(-1).tolist())
    assert np.load(a / "state.0.bias.npy").shape == (300,)  # (small arrays stay whole)
