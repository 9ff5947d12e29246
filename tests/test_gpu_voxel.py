"""Voxel media on the GPU (include/smcrt.h "voxel media"): voxel_kernel (voxel.h)
against the serial restatement of the semantics (tests/voxel_ref.c), photon by photon. Counters,
photon records, absorb, emission and detector bins are equal; jmean agrees up to summation
order (test_gpu_parity.compare)."""
import ctypes as C

import numpy as np
import pytest

from rsmcrt_amd import abi, scene
from rsmcrt_amd.engine import Engine, SmcrtError, load_library
from rsmcrt_amd.escape import escape_config
from tests import voxel_ref as V
from tests.geom_cases import MEDIUM, SUBJECT, face_source
from tests.test_gpu_parity import RTOL, SEED, compare
from tests.test_voxel_cpu import cube_labels, cube_scenes, slab_case

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH


def both(vs, g, src, n, flags=PL, dets=(), first=0, seed=SEED):
    with Engine(vs, g, dets) as eng:
        gpu = eng.run(src, n, seed=seed, flags=flags, first_photon=first, records=True)
    cpu = V.run(vs, g, src, n, seed=seed, flags=flags, dets=dets, first_photon=first, records=True)
    return gpu, cpu


# ---- the instantiations: grid mode x emitter ---------------------------------------------------
# (nx = ny = nz, half-extent): mode 2 has every 2*max and every n a power of two, 1 every 2*max only
GRIDS = {2: (16, 1.0), 1: (12, 1.0), 0: (12, 0.05)}


def pattern_case(gm, general=False):
    """Three media in blocks of 2 x 2 x 2 voxels, label (i//2 + j//2 + k//2) % 3: two voxels that
    touch and differ in label always differ in refractive index. Lengths scale with the grid's
    half-extent (the optical depths do not), as tests/plan_cases.py scales its small scenes."""
    n, half = GRIDS[gm]
    i, j, k = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    lab = ((i // 2 + j // 2 + k // 2) % 3).astype(np.uint8)
    s = 1.0 / half
    media = [scene.mono(5.0 * s, 0.2 * s, 0.7, 1.0), scene.mono(10.0 * s, 0.3 * s, 0.6, 1.4),
             scene.mono(2.0 * s, 0.05 * s, 0.3, 1.2)]
    if general:
        src = scene.circular_source((0.1 * half, -0.2 * half, 0.3 * half), (1.0, 2.0, 2.0), 0.5 * half)
    else:
        src = scene.point_source((0.03 * half, 0.05 * half, 0.07 * half))  # inside a voxel, on no wall
    return scene.VoxelScene(lab, media), scene.grid(n, n, n, half, half, half), src


@pytest.mark.parametrize("general", [False, True], ids=["plain", "general"])
@pytest.mark.parametrize("gm", [0, 1, 2], ids=["G0", "G1", "G2"])
def test_instantiations(gm, general):
    vs, g, src = pattern_case(gm, general)
    gpu, cpu = both(vs, g, src, 2000)
    compare(gpu, cpu)
    assert cpu.counter("fresnel") >= 200 and cpu.counter("reflections") >= 50, cpu.counters_dict()
    assert cpu.counter("faults") == 0 and cpu.counter("sdf_evals") == 0
    assert cpu.counter("scatters") > 2000 and cpu.counter("absorbed") > 0 and cpu.counter("escaped") > 0


@pytest.mark.parametrize("n", [1, 65])
def test_wave_edges(n):
    """One photon, and one lane past a wave."""
    vs, g, src = pattern_case(2)
    gpu, cpu = both(vs, g, src, n)
    compare(gpu, cpu)
    assert cpu.counter("photons") == n


def test_photon_index_above_32_bits():
    """One lane past a wave, from an index with a high word: the generator's seed and the record's
    slot (index - first_photon) both take the whole 64-bit index."""
    vs, g, src = pattern_case(2)
    gpu, cpu = both(vs, g, src, 65, first=2 ** 40 + 7)
    compare(gpu, cpu)
    assert cpu.counter("photons") == 65 and cpu.counter("faults") == 0


def test_rays_through_voxel_edges():
    """Pencils along a face diagonal from a point with x == y: every crossing of an x wall ties
    with a y wall, and after it the photon stands within an ulp of the edge it passed. The
    crossed axis is the one the crossing itself names (the first with ldir set), also for the
    near-zero piece that follows a tie."""
    vs, g, _ = pattern_case(2)
    s = 2.0 ** -0.5
    for start, d in (((0.03, 0.03, 0.07), (s, s, 0.0)), ((0.03, 0.07, 0.03), (-s, 0.0, -s)),
                     ((-0.9, -0.9, -0.9), (3.0 ** -0.5,) * 3)):
        gpu, cpu = both(vs, g, scene.pencil_source(start, d), 64)
        compare(gpu, cpu)
        assert cpu.counter("fresnel") >= 64


# ---- the deposit regimes ------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["buckets", "sorted", "atomic"])
def test_deposit_regimes(monkeypatch, regime):
    """A 96^3 grid (54 tiles) of one scattering medium with an index-matched inclusion: records
    filed into per-tile buckets, records sorted by tile, fp64 atomics (chosen at scene creation).
    Which one ran is the plan's answer (smcrt_scene_deposit_regime); only the bucketed fold's
    bk_reduce counts fold_cu_ms."""
    if regime != "buckets":
        monkeypatch.setenv("SMCRT_DEPOSIT", regime)
    n = 96
    lab = np.zeros((n, n, n), dtype=np.uint8)
    lab[30:60, 40:70, 20:50] = 1
    vs = scene.VoxelScene(lab, [scene.mono(10.0, 0.1, 0.9, 1.0), scene.mono(4.0, 0.5, 0.5, 1.0)])
    g = scene.grid(n, n, n, 1.0, 1.0, 1.0)
    src = scene.point_source((0.003, 0.005, 0.007))
    with Engine(vs, g) as eng:
        eng.set_timing(True)
        assert eng.deposit_regime() == regime
        gpu = eng.run(src, 2000, seed=SEED, records=True)
        kt = eng.kernel_times()
    cpu = V.run(vs, g, src, 2000, seed=SEED, records=True)
    compare(gpu, cpu)
    assert cpu.counter("deposits") > 100_000 and cpu.counter("fresnel") == 0
    assert kt["launches"] == 1 and kt["lean_launches"] == 0 and kt["transport_ms"] > 0.0
    assert (kt["fold_cu_ms"] > 0.0) == (regime == "buckets"), kt


def test_tiny_grids():
    """Grids of one voxel, of one voxel across, of one layer: a checkerboard of two mismatched media."""
    for nx, ny, nz in ((1, 1, 1), (1, 7, 3), (2, 2, 1)):
        i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
        vs = scene.VoxelScene(((i + j + k) % 2).astype(np.uint8),
                              [scene.mono(3.0, 0.1, 0.5, 1.0), scene.mono(6.0, 0.2, 0.8, 1.5)])
        g = scene.grid(nx, ny, nz, 1.0, 1.0, 1.0)
        gpu, cpu = both(vs, g, scene.point_source((0.03, 0.05, 0.07)), 500)
        compare(gpu, cpu)
        assert cpu.counter("photons") == 500 and cpu.counter("faults") == 0


def test_void_and_detectors():
    """The slab of test_voxel_cpu between two layers of void, with its two circle detectors."""
    vs, g, src, dets = slab_case()
    gpu, cpu = both(vs, g, src, 2000, dets=dets)
    compare(gpu, cpu)
    assert cpu.counter("detector_hits") > 0
    assert gpu.detector(0).sum() > 0 and gpu.detector(1).sum() > 0


def test_bounce_cap():
    """A lossless voxel of n = 2 in a void of n = 1, a point source at its centre: photons with
    every |direction component| below cos 30 deg are trapped by total internal reflection (most of
    an isotropic source). The flight ends at its 1001st reflection, so the run ends by the cap."""
    lab = np.zeros((3, 3, 3), dtype=np.uint8)
    lab[1, 1, 1] = 1
    vs = scene.VoxelScene(lab, [scene.mono(0.0, 0.0, 0.0, 1.0), scene.mono(0.0, 0.0, 0.0, 2.0)])
    g = scene.grid(3, 3, 3, 1.0, 1.0, 1.0)
    gpu, cpu = both(vs, g, scene.point_source(), 2000)
    compare(gpu, cpu)
    assert cpu.counter("bounce_aborts") > 0
    assert gpu.counter("bounce_aborts") == cpu.counter("bounce_aborts") == cpu.counter("faults")
    assert np.all(cpu.records["bounces"][cpu.records["status"] == 3] == 1001)


def test_survival_bias_and_render_source():
    vs, g, src = pattern_case(2)
    gpu, cpu = both(vs, g, src, 2000, flags=PL | abi.FLAG_SURVIVAL_BIAS | abi.FLAG_RENDER_SOURCE)
    compare(gpu, cpu, exact_absorb=False)
    assert np.array_equal(gpu.emission, cpu.emission) and gpu.emission.sum() == 2000
    assert np.any(cpu.records["weight"] < 1.0)


def test_no_pathlength():
    """The same trajectories and counters without SMCRT_FLAG_PATHLENGTH, and no deposit."""
    vs, g, src = pattern_case(2)
    gpu, cpu = both(vs, g, src, 2000, flags=0)
    compare(gpu, cpu)
    assert not gpu.jmean.any() and gpu.counter("deposits") == 0
    with_pl = V.run(vs, g, src, 2000, seed=SEED, records=True)
    for f in ("pos", "dir", "cell", "layer", "nscatt", "draws", "status"):
        assert np.array_equal(with_pl.records[f], cpu.records[f]), f
    a, b = with_pl.counters_dict(), cpu.counters_dict()
    assert a.pop("deposits") > 0 and b.pop("deposits") == 0 and a == b


def test_voxelise():
    """An SDF scene as its voxel twin; empty space needs an `outside` medium."""
    sdf, vs, g = cube_scenes(SUBJECT, MEDIUM)
    src = face_source()
    with Engine(sdf, g) as eng:
        twin = eng.voxelise()
    assert np.array_equal(twin.volume(g), cube_labels()) and np.array_equal(twin.labels, vs.labels)
    assert twin.media == [SUBJECT, MEDIUM]
    gpu, cpu = both(twin, g, src, 2000)
    compare(gpu, cpu)
    assert cpu.counter("fresnel") > 100
    ball = scene.Scene([scene.sphere(0.6, SUBJECT, 1)])
    with Engine(ball, g) as eng:
        with pytest.raises(ValueError, match="outside"):
            eng.voxelise()
        twin = eng.voxelise(outside=MEDIUM)
        lay, kap = eng.classify([(0.0, 0.0, 0.0), (0.9, 0.9, 0.9)])
    assert list(lay) == [1, 0] and twin.media == [SUBJECT, MEDIUM]
    vol = twin.volume(g)
    assert vol[8, 8, 8] == 0 and vol[0, 0, 0] == 1 and 0 < np.count_nonzero(vol == 0) < vol.size
    gpu, cpu = both(twin, g, src, 1000)
    compare(gpu, cpu)


def test_shard_invariance():
    vs, g, src = pattern_case(2)
    with Engine(vs, g) as eng:
        whole = eng.run(src, 2000, seed=SEED)
        parts = eng.run(src, 1000, seed=SEED, first_photon=0)
        parts = eng.run(src, 1000, seed=SEED, first_photon=1000, result=parts)
    assert whole.counters_dict() == parts.counters_dict()
    assert np.array_equal(whole.absorb, parts.absorb) and whole.nscatt[0] == parts.nscatt[0]
    np.testing.assert_allclose(whole.jmean, parts.jmean, rtol=RTOL, atol=1e-300)


def test_refusals():
    """What a voxel scene has no code for answers UNSUPPORTED and names voxel scenes; the scene
    still runs afterwards. classify and scene_info work."""
    vs, g, src = pattern_case(2)
    L = load_library()
    with Engine(vs, g) as eng:
        for flag in (abi.FLAG_TEST_KERNEL, abi.FLAG_TEST_KERNEL | abi.FLAG_END_EARLY, abi.FLAG_END_EARLY,
                     abi.FLAG_TRACK_PATHS, abi.FLAG_PHASOR):
            with pytest.raises(SmcrtError, match="UNSUPPORTED.*voxel"):
                eng.run(src, 10, flags=PL | flag)
            with pytest.raises(SmcrtError, match="UNSUPPORTED.*voxel"):
                eng.run_device(src, eng.config(10, SEED, PL | flag), abi.DeviceTallies())
        inv = abi.InverseConfig()
        inv.layer, inv.flags, inv.max_steps = 1, abi.INVERSE_FIND_MUS, 1
        d = C.c_uint64(0)
        calls = [lambda: eng.run_origins([(0.0, 0.0, 0.0)], 10),
                 lambda: eng.escape(escape_config(grid_size=(2, 2, 2)), 10),
                 lambda: eng.inverse(src, inv, 10, [-1.0]),
                 lambda: eng.set_path_tracking(0, 10),
                 lambda: eng.paths(),
                 lambda: eng.set_phasor(),
                 lambda: eng.phasor(),
                 lambda: eng.reset_phasor(),
                 lambda: eng.invoxel_segments()]
        for call in calls:
            with pytest.raises(SmcrtError, match="UNSUPPORTED.*voxel"):
                call()
        st = L.smcrt_scene_set_spectral(eng._h, C.c_int32(0), None, C.c_int32(abi.SPECTRAL_UPDATE), C.c_uint64(1),
                                        C.byref(d), None)
        assert st == abi.ERR_UNSUPPORTED and b"voxel" in L.smcrt_last_error()
        gg, n_top, n_dets = abi.Grid(), C.c_int32(), C.c_int32()
        assert L.smcrt_scene_info(eng._h, C.byref(gg), C.byref(n_top), C.byref(n_dets)) == abi.OK
        assert (gg.nx, gg.ny, gg.nz, n_top.value, n_dets.value) == (16, 16, 16, 3, 0)
        lay, kap = eng.classify([(0.03, 0.05, 0.07), (-0.99, -0.99, -0.99), (1.5, 0.0, 0.0), (0.3, -0.3, 0.6)])
        vol = vs.volume(g)
        assert list(lay) == [vol[8, 8, 8] + 1, vol[0, 0, 0] + 1, 0, vol[10, 5, 12] + 1]
        assert list(kap) == [vs.media[l - 1].kappa if l else 0.0 for l in lay]
        eng.check()
        gpu = eng.run(src, 500, seed=SEED, records=True)
    compare(gpu, V.run(vs, g, src, 500, seed=SEED, records=True))


def test_set_optprops():
    """A medium changed between two runs: each run is the restatement's with the table it ran on."""
    vs, g, src = pattern_case(2)
    new = scene.mono(7.0, 1.0, 0.2, 1.1)
    with Engine(vs, g) as eng:
        before = eng.run(src, 1000, seed=SEED, records=True)
        eng.set_optprops(1, new.mus, new.mua, new.hgg, new.n)
        assert eng.get_optprops(1)[0] == 2 and eng.get_optprops(1)[2:] == (new.mua, new.hgg, new.n)
        after = eng.run(src, 1000, seed=SEED, records=True)
    compare(before, V.run(vs, g, src, 1000, seed=SEED, records=True))
    changed = scene.VoxelScene(vs.labels, [vs.media[0], new, vs.media[2]])
    want = V.run(changed, g, src, 1000, seed=SEED, records=True)
    compare(after, want)
    assert not np.array_equal(before.records["draws"], after.records["draws"])
