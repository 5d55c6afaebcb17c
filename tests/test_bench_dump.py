"""bench.py --dump-outputs: the map of the last timed step as .npy files, so that two builds can be compared output for output."""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_the_whole_map_when_it_fits(tmp_path):
    import bench

    Z = np.random.default_rng(5).random((40, 24), dtype=np.float32)
    Z[3, 4] = np.nan
    bench.dump_outputs(str(tmp_path / "out"), Z)
    assert sorted(os.listdir(tmp_path / "out")) == ["power_map.npy"]
    got = np.load(tmp_path / "out" / "power_map.npy")
    assert got.dtype == np.float32 and np.array_equal(got, Z, equal_nan=True)


def test_dump_samples_the_same_rows_of_a_map_over_the_size_cap(tmp_path, monkeypatch):
    import bench

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 * 100 * 4)  # room for 64 rows of 100 cells
    Z = np.arange(1000 * 100, dtype=np.float32).reshape(1000, 100)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), Z)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["power_map.npy", "power_map_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_MAX_BYTES
    rows = np.load(tmp_path / "a" / "power_map_rows.npy")
    got = np.load(tmp_path / "a" / "power_map.npy")
    assert rows.dtype == np.float64 and got.dtype == np.float32
    assert rows.size == got.shape[0] > 0 and np.all(np.diff(rows) > 0)
    assert np.array_equal(got, Z[rows.astype(np.int64)])
    for f in files:  # a fixed, seeded sample: identical from run to run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_bench_refuses_zero_timed_steps():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--no-extras"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--steps must be >= 1" in out.stderr


@pytest.mark.gpu
def test_bench_dumps_the_timed_map_equal_to_the_oracle(tmp_path):
    """The dumped map of the default workload (BASELINE.json configs[1], hard validity) is the oracle's, row for row
    (tests/golden/cfg2_fullmap_crc.npz), and the JSON line reports the timed steps asked for."""
    import json
    import zlib

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1
    assert sorted(os.listdir(tmp_path)) == ["power_map.npy"]
    got = np.load(tmp_path / "power_map.npy")
    assert got.dtype == np.float32 and got.shape == (1024, 1024)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "cfg2_fullmap_crc.npz"))
    crcs = np.array([zlib.crc32(np.ascontiguousarray(got[i]).tobytes()) for i in range(got.shape[0])], np.uint32)
    assert int((crcs != gold["rx_hard_power_crc"]).sum()) == 0
