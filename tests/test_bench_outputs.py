"""bench.py --dump-outputs without a GPU: what it writes, and that a sample of a large cost matrix is the same every time."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _load(folder):
    return {name: np.load(os.path.join(folder, name + ".npy")) for name in ("records", "costs", "cost_rows")}


def test_small_costs_are_written_whole(tmp_path):
    records = torch.arange(6 * 10, dtype=torch.float32).reshape(6, 10)
    costs = torch.rand(6, 16, generator=torch.Generator().manual_seed(1))
    bench.dump_outputs(str(tmp_path), records, costs)
    out = _load(str(tmp_path))
    assert out["records"].dtype == np.float32 and np.array_equal(out["records"], records.numpy())
    assert out["costs"].dtype == np.float32 and np.array_equal(out["costs"], costs.numpy())
    assert out["cost_rows"].dtype == np.float64 and np.array_equal(out["cost_rows"], np.arange(6))


def test_large_costs_are_a_fixed_sample_of_poses(tmp_path, monkeypatch):
    P, N = 64, 16
    monkeypatch.setattr(bench, "DUMP_COST_BYTES", 8 * 4 * N)      # room for 8 of the 64 rows
    records = torch.zeros(P, 10)
    costs = torch.arange(P * N, dtype=torch.float32).reshape(P, N)
    dumps = []
    for run in range(2):
        bench.dump_outputs(str(tmp_path / str(run)), records, costs)
        dumps.append(_load(str(tmp_path / str(run))))
    rows = dumps[0]["cost_rows"].astype(np.int64)
    assert len(rows) == 8 and len(set(rows.tolist())) == 8 and np.all(np.diff(rows) > 0) and rows.max() < P
    assert np.array_equal(dumps[0]["costs"], costs.numpy()[rows])
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
