"""CPU: bench.py's command line and its output dump (no GPU: the dump is fed a host-side stand-in of a workload)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_times_one_block_and_full_restores_the_rest(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.blocks, a.full, a.dump_outputs) == (7, 2, 1, False, None)
    a = _parse(monkeypatch, "--full")
    assert a.full and a.blocks == 5
    assert _parse(monkeypatch, "--full", "--blocks", "2").blocks == 2
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def _workload():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(1, 4, 3), torch.nn.BatchNorm2d(4))
    return types.SimpleNamespace(models=[m, m], dev=torch.device("cpu"))


def test_dump_writes_every_output_as_float_npy(tmp_path):
    last = {"loss": torch.tensor(0.25), "parts": torch.arange(6, dtype=torch.float32), "labels": torch.arange(3)}
    bench.dump_outputs(str(tmp_path), _workload(), last)
    files = sorted(os.listdir(tmp_path))
    assert "step.loss.npy" in files and "model1.0.weight.npy" in files and "model0.1.num_batches_tracked.npy" in files
    assert all(f.endswith(".npy") for f in files)
    for f in files:
        assert np.load(tmp_path / f).dtype in (np.float32, np.float64), f
    assert np.load(tmp_path / "step.loss.npy").shape == () and float(np.load(tmp_path / "step.loss.npy")) == 0.25
    assert np.array_equal(np.load(tmp_path / "step.labels.npy"), np.arange(3.0))


def test_dump_of_large_outputs_is_a_fixed_sample_within_64_mb(tmp_path):
    g = torch.Generator().manual_seed(1)
    last = {"logits": torch.randn(48, 4, 224, 224, generator=g), "t_logits": torch.randn(48, 4, 224, 224, generator=g), "loss": torch.tensor(1.0)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _workload(), last)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64e6 + 4096 * len(os.listdir(tmp_path / "a"))      # (npy headers)
    lg = np.load(tmp_path / "a" / "step.logits.npy")
    assert 0 < lg.size < last["logits"].numel()
    assert np.isin(lg, last["logits"].numpy()).all()                   # a sample of the values, not something derived from them
    for f in os.listdir(tmp_path / "a"):                                # the same indices every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
