"""The bucketed deposit fold (deposit.h: bk_scan, bk_place, bk_reduce) at the edges of
bk_reduce's loop: a wave's run of a piece's buckets, read in batches of 64 {id, fill} entries
and groups of RED_GROUP buckets, with records loaded four per lane whatever the fill.

The shapes are chosen for those edges, not for a workload: pieces of one or a few buckets with
small fills (most waves of the block and most lanes of a batch past the run's end), a last tile
cut by the grid's voxel count, hundreds of partly filled buckets, tiles that split into several
pieces, exhausted-pool ids beside real ones, and a small fold that reuses the list a large one
left behind (tiles without a bucket: fold_bench --check, tools/microbench/fold_bench.hip). Every tally must equal the oracle's; jmean to rtol 1e-12 (its
fp64 sums land in another order on every run)."""
import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.engine import Engine

pytestmark = pytest.mark.gpu

RTOL = 1e-12
SEED = 123456789
TILE_VOXELS = 16384    # deposit.h TILE_VOXELS
PIECE_RECORDS = 65536  # deposit.h MIN_PIECE_RECORDS: a tile with more records than this splits


def compare(gpu, cpu):
    assert gpu.counters_dict() == cpu.counters_dict()
    assert gpu.nscatt[0] == cpu.nscatt[0]
    for f in ("pos", "dir", "weight", "cell", "layer", "nscatt", "bounces", "draws", "status"):
        assert np.array_equal(gpu.records[f], cpu.records[f]), f
    np.testing.assert_allclose(gpu.jmean, cpu.jmean, rtol=RTOL, atol=1e-300)
    assert np.array_equal(gpu.absorb, cpu.absorb)
    assert np.array_equal(gpu.emission, cpu.emission)
    assert np.array_equal(gpu.det_bins, cpu.det_bins)
    np.testing.assert_allclose(gpu.moments, cpu.moments, rtol=RTOL, atol=1e-300)


def folded(sc, g, src, n):
    """One run on the bucketed path (checked: bk_reduce ran and was timed) and the oracle's."""
    with Engine(sc, g) as eng:
        assert eng.deposit_regime() == "buckets"
        eng.kernel_times()
        gpu = eng.run(src, n, seed=SEED, records=True)
        kt = eng.kernel_times()
    assert 0.0 < kt["fold_cu_ms"] < 1e3, kt
    cpu = O.run(sc, g, src, n, seed=SEED, records=True)
    return gpu, cpu


def tiles_touched(jmean):
    """Tiles (TILE_VOXELS voxels in x-fastest order) with a deposit, of all tiles."""
    j = jmean.ravel()
    n_tiles = (j.size + TILE_VOXELS - 1) // TILE_VOXELS
    return sum(bool(np.any(j[t * TILE_VOXELS:(t + 1) * TILE_VOXELS])) for t in range(n_tiles)), n_tiles


@pytest.mark.parametrize("n", [1, 7, 300])
def test_fold_few_buckets_one_cut_tile(n):
    """20^3 = 8000 voxels: one tile, cut by the voxel count. One or a few blocks file records, so
    the piece holds one to a few buckets with fills far below 256."""
    sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0)
    gpu, cpu = folded(sc, scene.grid(20, 20, 20, 1, 1, 1), scene.point_source(), n)
    compare(gpu, cpu)
    assert cpu.counter("deposits") > 0 and tiles_touched(cpu.jmean) == (1, 1)


def test_fold_two_tiles_partly_filled_buckets():
    """40 x 24 x 20 = 19200 voxels: two tiles, the second partial. Every persistent block opens a
    bucket per tile it deposits into, so the fold sees hundreds of partly filled buckets."""
    sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0)
    gpu, cpu = folded(sc, scene.grid(40, 24, 20, 1, 1, 1), scene.point_source(), 3000)
    compare(gpu, cpu)
    assert tiles_touched(cpu.jmean) == (2, 2)


@pytest.mark.parametrize("cap", [0, 49152], ids=["pool", "small-pool"])
def test_fold_split_tiles_pencil_beam(monkeypatch, cap):
    """The pencil beam of test_bucket_contention_pencil_beam on 64^3 (16 tiles): the beam's tiles
    hold far more than 256 buckets. By the oracle's deposit counter at least one tile holds more
    records than a piece may (deposits over the tiles with any deposit; the few single-voxel
    segments that the lean path adds without a record are far fewer than the margin asked for),
    so bk_scan cuts it into several pieces. With SMCRT_POOL_CAP the pool runs out, and the fold
    sees exhausted-pool ids beside real ones."""
    if cap:
        monkeypatch.setenv("SMCRT_POOL_CAP", str(cap))
    sc = builders.setup_sphere(0.5, 0.01, 0.9, 1.0, 1.0)
    src = scene.pencil_source((0.0, 0.0, -0.99), (0.0, 0.0, 1.0))
    gpu, cpu = folded(sc, scene.grid(64, 64, 64, 1, 1, 1), src, 20000)
    touched, n_tiles = tiles_touched(cpu.jmean)
    print(f"deposits {cpu.counter('deposits')}, tiles with deposits {touched} of {n_tiles}")
    assert n_tiles == 16
    assert cpu.counter("deposits") > 1.25 * PIECE_RECORDS * touched
    if cap:
        assert cpu.counter("deposits") > 4 * cap
    compare(gpu, cpu)


def test_fold_reuses_list_of_larger_fold():
    """Two launches back to back (FLAG_ASYNC_FOLD | FLAG_OVERLAP) into one set of device tallies,
    the second far smaller: its fold reuses the {id, fill} list the first one's left behind, and
    must read none of those entries. Against one oracle run of all the photons."""
    import torch
    sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0)
    g = scene.grid(64, 64, 64, 1, 1, 1)
    src = scene.point_source()
    nv = 64 ** 3
    dev = torch.device("cuda", 0)
    jm = torch.zeros(nv, dtype=torch.float64, device=dev)
    ab = torch.zeros(nv, dtype=torch.float64, device=dev)
    ctr = torch.zeros(abi.NCOUNTERS, dtype=torch.int64, device=dev)
    dt = abi.DeviceTallies()
    dt.jmean, dt.absorb, dt.counters = jm.data_ptr(), ab.data_ptr(), ctr.data_ptr()
    stream = torch.cuda.current_stream()
    n1, n2 = 20000, 40
    fl = abi.FLAG_PATHLENGTH | abi.FLAG_ASYNC_FOLD | abi.FLAG_OVERLAP
    with Engine(sc, g) as eng:
        assert eng.deposit_regime() == "buckets"
        eng.run_device(src, Engine.config(n1, seed=SEED, flags=fl), dt, stream.cuda_stream)
        eng.run_device(src, Engine.config(n2, seed=SEED, flags=fl, first_photon=n1), dt, stream.cuda_stream)
        eng.fence(stream.cuda_stream)
        torch.cuda.synchronize()
        eng.check()
    cpu = O.run(sc, g, src, n1 + n2, seed=SEED)
    np.testing.assert_allclose(jm.cpu().numpy().reshape(64, 64, 64), cpu.jmean, rtol=RTOL, atol=1e-300)
    assert np.array_equal(ab.cpu().numpy().reshape(64, 64, 64), cpu.absorb)
    c = ctr.cpu().numpy()  # (every counter but the engine's own diagnostics, as counters_dict())
    got = {name: int(c[i]) for name, i in abi.CTR.items() if name not in abi.ENGINE_COUNTERS}
    assert got == cpu.counters_dict()
