"""Mesh media on the GPU (include/smcrt.h "mesh media"): mesh_kernel (mesh.h) against
the serial restatement of the semantics with its brute-force cast (tests/mesh_ref.c), photon by
photon. Counters, photon records, absorb, emission and detector bins are equal; jmean agrees up to
summation order (test_gpu_parity.compare, as tests/test_gpu_voxel.py holds the voxel kernel)."""
import ctypes as C

import numpy as np
import pytest

from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.engine import Comm, Engine, SmcrtError, load_library
from rsmcrt_amd.escape import escape_config
from tests import mesh_cases as M
from tests import mesh_ref as R
from tests.geom_cases import MEDIUM, SUBJECT, face_source
from tests.test_gpu_parity import RTOL, SEED, compare

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH
N = 20000
INSIDE = (0.03, 0.05, 0.07)  # inside a voxel, on no wall, inside every test surface around the origin


def both(ms, g, src, n=N, flags=PL, dets=(), first=0, seed=SEED):
    with Engine(ms, g, dets) as eng:
        gpu = eng.run(src, n, seed=seed, flags=flags, first_photon=first, records=True)
    cpu = R.run(ms, g, src, n, seed=seed, flags=flags, dets=dets, first_photon=first, records=True)
    return gpu, cpu


def test_fresnel_cube():
    gpu, cpu = both(M.cube_scene(), M.grid16(), face_source())
    compare(gpu, cpu)
    assert cpu.counter("fresnel") > 5000 and cpu.counter("reflections") > 500 and cpu.counter("faults") == 0
    assert cpu.counter("sdf_evals") == 0 and cpu.counter("scatters") > N


def test_icosphere():
    gpu, cpu = both(M.sphere_scene(2), M.grid16(), scene.point_source(INSIDE))
    compare(gpu, cpu)
    assert cpu.counter("fresnel") > N and cpu.counter("reflections") > 1000 and cpu.counter("faults") == 0
    assert set(np.unique(cpu.records["layer"])) == {1, 2}


def test_nested_spheres_with_a_void():
    gpu, cpu = both(M.nested_scene(), M.grid16(), face_source())
    compare(gpu, cpu)
    assert cpu.counter("fresnel") > 5000 and cpu.counter("faults") == 0
    assert set(np.unique(cpu.records["layer"])) == {1, 3}  # (nothing ends in the void)


def test_torus():
    gpu, cpu = both(M.torus_scene(), M.grid16(), scene.point_source((0.55, 0.02, 0.03)))
    compare(gpu, cpu)
    assert cpu.counter("fresnel") > N and cpu.counter("faults") == 0


def test_tetrahedron_one_node():
    gpu, cpu = both(M.tetra_scene(), M.grid16(), scene.point_source(INSIDE))
    compare(gpu, cpu)
    assert cpu.counter("fresnel") > N and cpu.counter("reflections") > 1000 and cpu.counter("faults") == 0


def test_ambient_scatters():
    gpu, cpu = both(M.ambient_scatters_scene(), M.grid16(), scene.point_source(INSIDE))
    compare(gpu, cpu)
    assert cpu.counter("scatters") > 5 * N and cpu.counter("fresnel") > 1000 and cpu.counter("faults") == 0


def test_inconsistent_labels():
    """The status-3 photons of a scene labelled inconsistently on purpose are an ordinary counted result."""
    gpu, cpu = both(M.nested_scene(consistent=False), M.grid16(), face_source())
    compare(gpu, cpu)
    assert gpu.counter("faults") == np.count_nonzero(gpu.records["status"] == 3) > 1000
    assert gpu.counter("bounce_aborts") == 0


# ---- the instantiations: grid mode x emitter -------------------------------------------------------
GRIDS = {2: (16, 1.0), 1: (12, 1.0), 0: (12, 0.05)}  # test_gpu_voxel's: mode 2, 1, 0


@pytest.mark.parametrize("general", [False, True], ids=["plain", "general"])
@pytest.mark.parametrize("gm", [0, 1, 2], ids=["G0", "G1", "G2"])
def test_instantiations(gm, general):
    """icosphere(1) scaled with the grid's half-extent (the optical depths are not)."""
    n, half = GRIDS[gm]
    s = 1.0 / half
    ms = scene.MeshScene([scene.mono(10.0 * s, 0.3 * s, 0.6, 1.4), scene.mono(1.0 * s, 0.02 * s, 0.3, 1.0)], ambient=1)
    ms.add_surface(*builders.icosphere(1, 0.6 * half, (0.05 * half, 0.0, -0.1 * half)), 0, 1)
    if general:
        src = scene.circular_source((0.1 * half, -0.2 * half, 0.3 * half), (1.0, 2.0, 2.0), 0.5 * half)
    else:
        src = scene.point_source((0.03 * half, 0.05 * half, 0.07 * half))
    gpu, cpu = both(ms, scene.grid(n, n, n, half, half, half), src, 4000)
    compare(gpu, cpu)
    assert cpu.counter("fresnel") >= 2000 and cpu.counter("reflections") >= 100 and cpu.counter("faults") == 0
    assert cpu.counter("absorbed") > 0 and cpu.counter("escaped") > 0


@pytest.mark.parametrize("n", [1, 63, 20001])
def test_photon_counts(n):
    gpu, cpu = both(M.sphere_scene(1), M.grid16(), scene.point_source(INSIDE), n)
    compare(gpu, cpu)
    assert cpu.counter("photons") == n


def test_photon_index_above_32_bits():
    """One lane past a wave, from an index with a high word: the generator's seed and the record's
    slot (index - first_photon) both take the whole 64-bit index."""
    gpu, cpu = both(M.cube_scene(), M.grid16(), face_source(), 65, first=2 ** 40 + 7)
    compare(gpu, cpu)
    assert cpu.counter("photons") == 65 and cpu.counter("faults") == 0


def test_first_photon_and_accumulation():
    """A non-zero first_photon; two runs accumulating into one Result are the run of both."""
    ms, g, src = M.sphere_scene(1), M.grid16(), scene.point_source(INSIDE)
    gpu, cpu = both(ms, g, src, 3000, first=10 ** 12 + 7)
    compare(gpu, cpu)
    with Engine(ms, g) as eng:
        whole = eng.run(src, 2000, seed=SEED)
        parts = eng.run(src, 1000, seed=SEED, first_photon=0)
        parts = eng.run(src, 1000, seed=SEED, first_photon=1000, result=parts)
    assert whole.counters_dict() == parts.counters_dict()
    assert np.array_equal(whole.absorb, parts.absorb) and whole.nscatt[0] == parts.nscatt[0]
    np.testing.assert_allclose(whole.jmean, parts.jmean, rtol=RTOL, atol=1e-300)
    want = R.run(ms, g, src, 2000, seed=SEED)
    assert whole.counters_dict() == want.counters_dict()


@pytest.mark.parametrize("regime", ["buckets", "sorted", "atomic"])
def test_deposit_regimes(monkeypatch, regime):
    """test_gpu_voxel's 96^3 grid (54 tiles): which regime ran is the plan's answer."""
    if regime != "buckets":
        monkeypatch.setenv("SMCRT_DEPOSIT", regime)
    g = scene.grid(96, 96, 96, 1.0, 1.0, 1.0)
    ms = scene.MeshScene([scene.mono(4.0, 0.5, 0.5, 1.0), scene.mono(10.0, 0.1, 0.9, 1.0)], ambient=1)
    ms.add_surface(*builders.icosphere(2, 0.5), 0, 1)
    src = scene.point_source((0.003, 0.005, 0.007))
    with Engine(ms, g) as eng:
        eng.set_timing(True)
        assert eng.deposit_regime() == regime
        gpu = eng.run(src, 2000, seed=SEED, records=True)
        kt = eng.kernel_times()
    cpu = R.run(ms, g, src, 2000, seed=SEED, records=True)
    compare(gpu, cpu)
    assert cpu.counter("deposits") > 100_000 and cpu.counter("fresnel") == 0
    assert kt["launches"] == 1 and kt["lean_launches"] == 0 and kt["transport_ms"] > 0.0
    assert (kt["fold_cu_ms"] > 0.0) == (regime == "buckets"), kt
    # the casts' node visits: at least one per cast, at most all nodes (639 for 320 triangles) per cast
    assert cpu.counter("grid_updates") <= kt["far_steps"] <= 639 * cpu.counter("grid_updates")


def test_survival_bias_and_render_source():
    gpu, cpu = both(M.sphere_scene(2), M.grid16(), scene.point_source(INSIDE),
                    flags=PL | abi.FLAG_SURVIVAL_BIAS | abi.FLAG_RENDER_SOURCE)
    compare(gpu, cpu, exact_absorb=False)
    assert np.array_equal(gpu.emission, cpu.emission) and gpu.emission.sum() == N
    assert np.any(cpu.records["weight"] < 1.0)


def test_detectors_of_each_kind():
    """A circle, an annulus, a camera and a fibre on the nested spheres."""
    dets = [scene.circle_dect((0.0, 0.0, -0.95), (0.0, 0.0, -1.0), 1, 0.8, 50),
            scene.annulus_dect((0.0, 0.0, 0.95), (0.0, 0.0, 1.0), 1, 0.2, 0.9, 40),
            scene.camera((-0.9, -0.9, -0.9), (1.8, 0.0, 0.0), (0.0, 1.8, 0.0), 1, 16, 1.0),
            scene.fibre_dect((0.9, 0.0, 0.0), (1.0, 0.0, 0.0), 1, 20)]
    gpu, cpu = both(M.nested_scene(), M.grid16(), scene.point_source(INSIDE), dets=dets)
    compare(gpu, cpu)
    assert cpu.counter("detector_hits") > 100
    assert gpu.detector(0).sum() > 0 and gpu.detector(1).sum() > 0


def test_no_pathlength():
    """flags = 0: the same trajectories and counters, no walk and no deposit."""
    ms, g, src = M.sphere_scene(2), M.grid16(), scene.point_source(INSIDE)
    gpu, cpu = both(ms, g, src, flags=0)
    compare(gpu, cpu)
    assert not gpu.jmean.any() and gpu.counter("deposits") == 0
    with_pl = R.run(ms, g, src, N, seed=SEED, records=True)
    for f in ("dir", "layer", "nscatt", "draws", "status"):
        assert np.array_equal(with_pl.records[f], cpu.records[f]), f


@pytest.mark.parametrize("case", ["shell", "ambient"])
def test_no_pathlength_through_a_void(case):
    """flags = 0 with void legs. In the nested spheres' shell every void leg ends on a surface and is
    jumped to it. In a void ambient medium a leg that meets nothing has dlen = inf: the jump puts the
    position at infinity, outside the grid, and the photon has escaped. (A zero direction component
    would make 0 * inf = NaN of that position; no photon of this run has one, as the assertion on
    the reference's records says, so the records compare with ==.)"""
    if case == "shell":
        ms, src, n = M.nested_scene(), face_source(), N
    else:
        ms, src, n = M.sphere_scene(2, outer=M.VOID), scene.point_source(INSIDE), 4000
    gpu, cpu = both(ms, M.grid16(), src, n, flags=0)
    compare(gpu, cpu)
    assert not gpu.jmean.any() and gpu.counter("deposits") == 0 and cpu.counter("faults") == 0
    assert cpu.counter("fresnel") > 1000 and cpu.counter("escaped") > 100
    pos, escaped = cpu.records["pos"], cpu.records["status"] == 2
    assert not np.isnan(pos).any()
    if case == "ambient":  # every escape is a leg to infinity, and nothing else is
        assert np.array_equal(np.isinf(pos).all(axis=1), escaped) and np.array_equal(np.isinf(pos).any(axis=1), escaped)
    else:
        assert np.isfinite(pos).all()


def test_run_device():
    """smcrt_run_device serves the scene: its device tallies are smcrt_run's."""
    import torch
    ms, g, src = M.sphere_scene(1), M.grid16(), scene.point_source(INSIDE)
    n = 2000
    dev = torch.device("cuda", 0)
    jm = torch.zeros(g.nx * g.ny * g.nz, dtype=torch.float64, device=dev)
    ab = torch.zeros(g.nx * g.ny * g.nz, dtype=torch.float64, device=dev)
    ctr = torch.zeros(abi.NCOUNTERS, dtype=torch.int64, device=dev)
    dt = abi.DeviceTallies()
    dt.jmean, dt.absorb, dt.counters = jm.data_ptr(), ab.data_ptr(), ctr.data_ptr()
    stream = torch.cuda.current_stream()
    with Engine(ms, g) as eng:
        eng.run_device(src, Engine.config(n, seed=SEED, flags=PL), dt, stream.cuda_stream)
        eng.fence(stream.cuda_stream)
        torch.cuda.synchronize()
    want = R.run(ms, g, src, n, seed=SEED)
    c = ctr.cpu().numpy()
    assert {k: int(c[i]) for k, i in abi.CTR.items() if k != "wave_iters"} == want.counters_dict()
    assert np.array_equal(ab.cpu().numpy().reshape(want.absorb.shape), want.absorb)
    np.testing.assert_allclose(jm.cpu().numpy().reshape(want.jmean.shape), want.jmean, rtol=RTOL, atol=1e-300)


def test_refusals():
    """What a mesh scene has no code for answers UNSUPPORTED and names mesh scenes; the scene still
    runs afterwards. classify, scene_info and set_optprops work."""
    ms, g, src = M.nested_scene(), M.grid16(), scene.point_source(INSIDE)
    L = load_library()
    comm = Comm(Comm.unique_id(), 1, 0, 0)  # one rank on this GPU, as test_reduce_device_tallies_one_rank
    with Engine(ms, g) as eng:
        for flag in (abi.FLAG_TEST_KERNEL, abi.FLAG_TEST_KERNEL | abi.FLAG_END_EARLY, abi.FLAG_END_EARLY,
                     abi.FLAG_TRACK_PATHS, abi.FLAG_PHASOR):
            with pytest.raises(SmcrtError, match="UNSUPPORTED.*mesh"):
                eng.run(src, 10, flags=PL | flag)
            with pytest.raises(SmcrtError, match="UNSUPPORTED.*mesh"):
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
                 lambda: eng.invoxel_segments(),
                 lambda: eng.reduce_device_tallies(comm, abi.DeviceTallies())]
        for call in calls:
            with pytest.raises(SmcrtError, match="UNSUPPORTED.*mesh"):
                call()
        st = L.smcrt_scene_set_spectral(eng._h, C.c_int32(0), None, C.c_int32(abi.SPECTRAL_UPDATE), C.c_uint64(1),
                                        C.byref(d), None)
        assert st == abi.ERR_UNSUPPORTED and b"mesh" in L.smcrt_last_error()
        with pytest.raises(ValueError, match="mesh"):
            eng.voxelise()
        gg, n_top, n_dets = abi.Grid(), C.c_int32(), C.c_int32()
        assert L.smcrt_scene_info(eng._h, C.byref(gg), C.byref(n_top), C.byref(n_dets)) == abi.OK
        assert (gg.nx, gg.ny, gg.nz, n_top.value, n_dets.value) == (16, 16, 16, 3, 0)
        lay, kap = eng.classify([(0.9, 0.9, 0.9), (0.0, 0.0, 0.6), (0.05, 0.0, -0.1), (1.5, 0.0, 0.0)])
        assert list(lay) == [1, 2, 3, 0] and list(kap) == [MEDIUM.kappa, 0.0, M.GLASS.kappa, 0.0]
        eng.check()
        before = eng.run(src, 1000, seed=SEED, records=True)
        new = scene.mono(7.0, 1.0, 0.2, 1.1)
        eng.set_optprops(2, new.mus, new.mua, new.hgg, new.n)
        assert eng.get_optprops(2)[2:] == (new.mua, new.hgg, new.n)
        after = eng.run(src, 1000, seed=SEED, records=True)
    comm.close()
    compare(before, R.run(ms, g, src, 1000, seed=SEED, records=True))
    changed = M.nested_scene()
    changed.media[2] = new
    compare(after, R.run(changed, g, src, 1000, seed=SEED, records=True))
