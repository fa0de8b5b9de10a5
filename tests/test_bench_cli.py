"""bench.py's command line around the timed steps: --dump-outputs writes
float64 .npy files within its size limit (a larger X as a fixed row sample),
and --repeats belongs to --full (a plain run times exactly --steps steps).
CPU only: nothing here creates a context."""
import os
import sys

import numpy as np
import pytest

import bench


def test_dump_outputs_writes_float64_arrays(tmp_path):
    X = bench.splitmix((37, 3), 3.0, 1)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), X, 0.25, 2.0)
    assert sorted(os.listdir(out)) == ["particles.npy", "scale.npy"]
    P = np.load(out / "particles.npy")
    assert P.dtype == np.float64
    np.testing.assert_array_equal(P, X)
    np.testing.assert_array_equal(np.load(out / "scale.npy"), np.array([0.25, 2.0]))


def test_dump_outputs_other_ranks_write_nothing(tmp_path):
    bench.dump_outputs(None, np.zeros((4, 2)), 1.0, 1.0)
    assert os.listdir(tmp_path) == []


def test_dump_outputs_samples_rows_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096 + 100 * 4 * 8)  # room for 100 x (3 + 1) doubles
    X = bench.splitmix((1000, 3), 3.0, 2)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), X, 0.5, 1.5)
    rows = np.load(tmp_path / "a" / "particle_rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 100
    idx = rows.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 1000
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "particles.npy"), X[idx])
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "particle_rows.npy"))  # the same sample every run
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_MAX_BYTES
    # a later dump of a small X into the same directory leaves no stale sample
    bench.dump_outputs(str(tmp_path / "a"), X[:10], 0.5, 1.5)
    assert sorted(os.listdir(tmp_path / "a")) == ["particles.npy", "scale.npy"]


def test_repeats_needs_full(monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--repeats", "3"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
    assert "--repeats needs --full" in capsys.readouterr().err
