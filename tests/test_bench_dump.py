"""bench.py --dump-outputs (CPU): the files are float64, stay within the byte budget, and an
array that does not fit is written as the same sample of its elements every time."""
import os

import numpy as np

import bench
from rsmcrt_amd import abi


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 16)  # 8192 elements in all
    big = np.arange(30000, dtype=np.float64)
    arrays = {"jmean": big.reshape(30, 10, 100), "absorb": big[::-1].reshape(30, 10, 100),
              "nscatt": np.array([7.0]), "counters": np.arange(15, dtype=np.uint64),
              "det_bins": np.arange(75, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 16
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert all(v.dtype == np.float64 for v in got.values())
    # what fits is whole, in its own shape
    for k in ("nscatt", "counters", "det_bins"):
        assert np.array_equal(got[k], arrays[k].astype(np.float64))
    # what does not is a sample of distinct elements, the same for both arrays of that shape
    # (jmean[i] + absorb[i] = 29999 at every i) and for both calls
    assert 3000 < got["jmean"].size == got["absorb"].size < big.size
    assert np.all(np.diff(got["jmean"]) > 0)
    assert np.array_equal(got["jmean"] + got["absorb"], np.full(got["jmean"].shape, 29999.0))
    for f in files:
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f))


def test_dump_outputs_default_budget_is_64_mib():
    assert bench.DUMP_BYTES == 64 * 1024 * 1024


def test_dumped_counters_leave_out_the_engine_counters():
    c = np.arange(abi.NCOUNTERS, dtype=np.uint64)
    kept = bench.photon_counters(c)
    assert kept.size == abi.NCOUNTERS - len(abi.ENGINE_COUNTERS)
    assert abi.CTR["wave_iters"] not in kept.tolist() and abi.CTR["deposits"] in kept.tolist()
