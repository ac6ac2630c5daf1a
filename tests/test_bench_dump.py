"""bench.py --dump-outputs on the host: small outputs are written whole, large ones as a fixed, seeded sample of rows that
keeps the dump under its byte budget (what the EKF and MPC workloads need at their full batch)."""
import os

import numpy as np
import torch

import bench


def _outputs(B):
    return {"P": torch.arange(B * 36, dtype=torch.float64).reshape(B, 36), "delta": -torch.arange(B * 6, dtype=torch.float64).reshape(B, 6),
            "iter": torch.arange(B, dtype=torch.int32)}


def test_small_outputs_are_written_whole_as_float64(tmp_path):
    outs = _outputs(100)
    bench.dump_outputs(outs, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["P.npy", "delta.npy", "iter.npy"]
    for k, t in outs.items():
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, t.numpy())


def test_large_outputs_keep_a_seeded_sample_of_rows_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 2_000_000)
    B = 65536
    outs = _outputs(B)
    bench.dump_outputs(outs, str(tmp_path / "a"))
    bench.dump_outputs(outs, str(tmp_path / "b"))
    data = sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a"))
    assert 1_900_000 < data <= 2_000_000
    rows = np.load(tmp_path / "a" / "sampled_rows.npy").astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < B
    assert np.array_equal(np.load(tmp_path / "a" / "P.npy"), outs["P"].numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "delta.npy"), outs["delta"].numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "iter.npy"), np.arange(B, dtype=np.float64))  # 1-D outputs stay whole
    for f in os.listdir(tmp_path / "a"):  # the same sample on every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_the_budget_leaves_room_for_the_npy_headers():
    assert bench.DUMP_BYTES + 16 * 128 <= 64_000_000


def test_one_dimensional_outputs_beyond_half_the_budget_are_sampled_too(tmp_path, monkeypatch):
    """A batch so large that its per-item scalars alone fill the budget (millions of items): every output keeps the same
    sampled rows."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    B = 40000
    outs = _outputs(B)
    bench.dump_outputs(outs, str(tmp_path))
    assert sum(np.load(tmp_path / f).nbytes for f in os.listdir(tmp_path)) <= 200_000
    rows = np.load(tmp_path / "sampled_rows.npy").astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[-1] < B
    assert np.array_equal(np.load(tmp_path / "iter.npy"), rows.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "P.npy"), outs["P"].numpy()[rows])
