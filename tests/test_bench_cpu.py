"""CPU tests of bench.py's --dump-outputs writer: the state is generated on the host (no GPU), written, read back."""
import os

import numpy as np
import pytest

import bench

NAMES = ("positions", "velocities", "masses", "radii")


def _state(nb, n, precision):
    return nb.init_bodies(nb.stock_config(particleCount=n), precision)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


@pytest.mark.parametrize("fp64", [False, True])
def test_dump_writes_whole_state(nb, tmp_path, fp64):
    state = _state(nb, 1000, nb.F64 if fp64 else nb.F32)
    bench.dump_outputs(str(tmp_path), state)
    got = _load(tmp_path)
    assert set(got) == set(NAMES) | {"num_bodies"}
    assert got["num_bodies"].dtype == np.float64 and got["num_bodies"].tolist() == [1000.0]
    for name, want in zip(NAMES, (state.Positions, state.Velocities, state.Masses, state.Radii)):
        assert got[name].dtype == (np.float64 if fp64 else np.float32), name
        assert np.array_equal(got[name], want), name


def test_dump_samples_a_large_state(nb, tmp_path, monkeypatch):
    """Above the size limit: a fixed sample of bodies, the same from run to run, within the limit."""
    limit = 24 * 400 + 4096
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    state = _state(nb, 1000, nb.F32)
    bench.dump_outputs(str(tmp_path / "a"), state)
    bench.dump_outputs(str(tmp_path / "b"), state)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(NAMES) | {"num_bodies", "sample_index"}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    idx = a["sample_index"].astype(np.int64)
    assert 0 < len(idx) < 1000 and np.all(np.diff(idx) > 0) and idx[-1] < 1000
    assert a["num_bodies"].tolist() == [1000.0]
    for name, want in zip(NAMES, (state.Positions, state.Velocities, state.Masses, state.Radii)):
        assert np.array_equal(a[name], want[idx]), name
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= limit
