"""bench.py --dump-outputs on the host: arrays within the budget are written whole, a larger one as a fixed sample."""
import os

import numpy as np
import torch

import bench


def test_write_outputs_keeps_the_budget_with_a_fixed_sample(tmp_path):
    small = torch.arange(10, dtype=torch.float32)
    big = torch.arange(100000, dtype=torch.float64).reshape(100, 1000)
    budget = 2 * 128 + 4 * 1000
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"small": small, "big": big}, budget=budget)
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.numpy())
    assert b.dtype == np.float32 and b.shape == (990,) and (np.diff(b) > 0).all() and b.min() >= 0 and b.max() < 100000
    np.testing.assert_array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget
    bench.write_outputs(str(tmp_path / "c"), {"big": big})  # the default budget holds it whole
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "big.npy"), big.numpy().astype(np.float32))
