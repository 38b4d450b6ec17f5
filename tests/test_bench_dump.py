"""CPU checks of bench.py's --dump-outputs writer and of the plain / --full split of its arguments (no GPU)."""
import subprocess
import sys

import numpy as np

from conftest import REPO


def _bench():
    sys.path.insert(0, str(REPO))
    import bench
    return bench


def test_dump_outputs_writes_every_array_as_float64(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(3)
    X, st = rng.normal(size=(7, 21, 6)), rng.integers(0, 6, 7).astype(np.int32)
    bench.dump_outputs(tmp_path / "d", {"x_out": X, "status": st})
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == ["status.npy", "x_out.npy"]
    x, s = np.load(tmp_path / "d" / "x_out.npy"), np.load(tmp_path / "d" / "status.npy")
    assert x.dtype == np.float64 and s.dtype == np.float64
    assert np.array_equal(x, X) and np.array_equal(s, st)


def test_dump_outputs_keeps_one_fixed_sample_of_rows_above_the_cap(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096)
    rng = np.random.default_rng(4)
    X, kk = rng.normal(size=(100, 3, 2)), rng.normal(size=100)   # 56 B per row + 8 B of index: 64 rows fit
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"x_out": X, "kkt": kk})
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "sample_index.npy"))     # the same rows every run
    assert idx.size == 64 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 100
    i = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "x_out.npy"), X[i])
    assert np.array_equal(np.load(tmp_path / "a" / "kkt.npy"), kk[i])
    assert sum(np.load(p).nbytes for p in (tmp_path / "a").iterdir()) <= 4096


def test_bench_has_the_full_and_dump_outputs_options():
    out = subprocess.run([sys.executable, str(REPO / "bench.py"), "--help"], capture_output=True, text=True, timeout=120,
                         check=True).stdout
    assert "--full" in out and "--dump-outputs DIR" in out
