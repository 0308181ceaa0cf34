"""bench.py's host-side pieces that need no GPU: the --full / --dump-outputs options and the
output dump (whole tensor below the size cap, a fixed seeded sample above it)."""
import sys

import numpy as np
import torch

import bench


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_tensor(tmp_path):
    out = torch.linspace(-1, 1, 2 * 3 * 8 * 8).reshape(2, 3, 8, 8)
    bench.dump_outputs(str(tmp_path / "new" / "dir"), out)
    got = np.load(tmp_path / "new" / "dir" / "output.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 8, 8)
    assert np.array_equal(got, out.numpy())


def test_dump_outputs_sample_is_fixed_and_capped(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 100)
    out = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out)
    a, b = np.load(tmp_path / "a" / "output.npy"), np.load(tmp_path / "b" / "output.npy")
    assert a.dtype == np.float32 and a.nbytes == 400
    assert np.array_equal(a, b)
    # values are their own flat indices here: distinct, ascending elements of the output
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] <= 999
