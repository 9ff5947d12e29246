"""The volume source on the GPU (include/smcrt.h "volume source"): emit_ext's case SMCRT_SRC_VOLUME
against smcrt_volume_sample, the same text run on the host (which tests/test_volume_source_cpu.py
holds against the rule restated in Python), on every general-emitter instantiation of
transport_kernel and on voxel_kernel and mesh_kernel; positions and directions bit for bit through
recorded paths and photon records; the transport that follows, through Beer's law in an absorbing
box; the table's semantics, the refusals, and rsmcrt_amd.fluorescence on three stacked layers."""
import ctypes as C
import math

import numpy as np
import pytest

from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.engine import Engine, MultiEngine, SmcrtError, load_library
from rsmcrt_amd.escape import escape_config
from rsmcrt_amd.fluorescence import fluorescence
from tests import mesh_cases, plan_cases, planprobe
from tests.test_gpu_phasor import near_vacuum

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH
RS = abi.FLAG_PATHLENGTH | abi.FLAG_RENDER_SOURCE
SEED = 20261020
VOL = scene.volume_source


def grid8():
    return scene.grid(8, 8, 8, 1.0, 1.0, 1.0)


def grid543():
    return scene.grid(5, 4, 3, 1.0, 0.75, 0.4)


def nvox(g):
    return g.nx * g.ny * g.nz


def sparse_weights(g, seed=5, k=150):
    """About k voxels with weights in [0.2, 1), the first and the last voxel among them; the rest 0."""
    rng = np.random.default_rng(seed)
    n = nvox(g)
    w = np.zeros(n)
    idx = np.unique(np.concatenate([rng.integers(0, n, min(k, n)), [0, n - 1]]))
    w[idx] = rng.uniform(0.2, 1.0, len(idx))
    return w


def host_sample(w, g, n, seed=SEED, first=0):
    """smcrt_volume_sample: (pos, dir, voxel)."""
    L = load_library()
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
    pos, d, vox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int64)
    st = L.smcrt_volume_sample(w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(g), seed, first, n,
                               pos.ctypes.data_as(C.POINTER(C.c_double)), d.ctypes.data_as(C.POINTER(C.c_double)),
                               vox.ctypes.data_as(C.POINTER(C.c_int64)))
    assert st == abi.OK, L.smcrt_last_error()
    return pos, d, vox


def recell(pos, g):
    """The grid's own rule (update_voxels: floor(n * (p + max) / (2 * max)), 0-based here), linearised x fastest."""
    c = [np.floor(n * (pos[:, a] + m) / (2.0 * m)).astype(np.int64) for a, (n, m) in
         enumerate(((g.nx, g.xmax), (g.ny, g.ymax), (g.nz, g.zmax)))]
    return c[0] + g.nx * (c[1] + g.ny * c[2])


def expected_emission(w, g, n, seed=SEED, first=0):
    """The histogram of the host sampler's voxels, shaped as Result.emission; first the condition on
    the inputs: every sampled position re-cells to the voxel that was picked."""
    pos, _, vox = host_sample(w, g, n, seed, first)
    assert np.array_equal(recell(pos, g), vox), "a sampled position re-cells to another voxel: choose other inputs"
    return np.bincount(vox, minlength=nvox(g)).astype(np.float64).reshape(g.nz, g.ny, g.nx)


def check_emission(eng, w, g, n, seed=SEED, first=0):
    res = eng.run(VOL(), n, seed=seed, flags=RS, first_photon=first)
    assert res.counter("photons") == n and res.counter("faults") == 0 and res.counter("emit_retries") == 0
    assert np.array_equal(res.emission, expected_emission(w, g, n, seed, first))
    return res


# ---- 1. emission is the host sampler's ---------------------------------------------------------------
XSRC_CASES = [c for c in plan_cases.group("matrix") if c.kernel[0] == "transport_kernel" and c.kernel[3] == 1]


def test_the_matrix_holds_every_general_emitter_instantiation():
    assert sorted(c.kernel for c in XSRC_CASES) == sorted(k for k in plan_cases.TRANSPORT_KERNELS if k[3] == 1)
    assert len(XSRC_CASES) == 9


@pytest.mark.parametrize("case", XSRC_CASES, ids=[c.id for c in XSRC_CASES])
def test_emission_on_every_xsrc_instantiation(case, monkeypatch):
    """The scene, grid and environment of the matching case of tests/plan_cases.py give the grid
    mode, the faces' place and COOP; the volume source makes the launch a general-emitter one."""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    sc, g = case.scene(), case.scene_grid()
    plan = planprobe.plan(sc, g, env=case.env)
    assert plan["status"] == abi.OK, plan["error"]
    assert plan_cases.kernel_of(plan, True, PL) == case.kernel
    w = sparse_weights(g, seed=len(case.id))
    with Engine(sc, g) as eng:
        eng.set_volume_source(w)
        info = eng.volume_source_info()
        assert info["n_positive"] == info["n_reachable"] == np.count_nonzero(w)
        eng.kernel_times()
        check_emission(eng, w, g, 20001)
        assert eng.kernel_times()["lean_launches"] == 0  # (a volume source never runs the lean path)


@pytest.mark.parametrize("n", [1, 63, 20001])
@pytest.mark.parametrize("gname", ["8x8x8", "5x4x3"])
def test_emission_photon_counts(gname, n):
    g = grid8() if gname == "8x8x8" else grid543()
    sc = scene.Scene([scene.box((2.0 * g.xmax, 2.0 * g.ymax, 2.0 * g.zmax), scene.mono(5.0, 0.5, 0.7, 1.0), 1)])
    w = sparse_weights(g, seed=n, k=20)
    with Engine(sc, g) as eng:
        eng.set_volume_source(w.reshape(g.nz, g.ny, g.nx))  # (the 3-D form)
        check_emission(eng, w, g, n)


def test_two_shards_equal_the_whole():
    g = grid543()
    sc = scene.Scene([scene.box((2.0, 1.5, 0.8), scene.mono(5.0, 0.5, 0.7, 1.0), 1)])
    w = sparse_weights(g, seed=2, k=20)
    with Engine(sc, g) as eng:
        eng.set_volume_source(w)
        whole = eng.run(VOL(), 5000, seed=SEED, flags=RS, first_photon=100, records=True)
        a = check_emission(eng, w, g, 1777, first=100)
        b = check_emission(eng, w, g, 5000 - 1777, first=100 + 1777)
        ra = eng.run(VOL(), 1777, seed=SEED, flags=RS, first_photon=100, records=True)
    assert np.array_equal(a.emission + b.emission, whole.emission)
    assert np.array_equal(a.absorb + b.absorb, whole.absorb)
    assert np.array_equal(ra.records, whole.records[:1777])
    for name in ("photons", "scatters", "absorbed", "escaped", "rng_draws"):
        assert a.counter(name) + b.counter(name) == whole.counter(name), name


@pytest.mark.parametrize("gm", [0, 1, 2], ids=["G0", "G1", "G2"])
def test_emission_on_a_voxel_scene(gm):
    from tests.test_gpu_voxel import pattern_case
    vs, g, _ = pattern_case(gm)
    w = sparse_weights(g, seed=gm)
    with Engine(vs, g) as eng:
        eng.set_volume_source(w)
        check_emission(eng, w, g, 20001)


def test_emission_on_a_mesh_scene():
    ms, g = mesh_cases.sphere_scene(), mesh_cases.grid16()
    w = sparse_weights(g, seed=16)
    with Engine(ms, g) as eng:
        eng.set_volume_source(w)
        check_emission(eng, w, g, 20001)


# ---- 2. positions and directions, bit for bit ---------------------------------------------------------
def test_first_path_vertex_is_the_sampled_position():
    g = grid8()
    sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 0.7)
    w = sparse_weights(g, seed=3, k=40)
    n = 2000
    pos, _, _ = host_sample(w, g, n)
    with Engine(sc, g) as eng:
        eng.set_volume_source(w)
        eng.set_path_tracking(0, 64)
        res = eng.run(VOL(), n, seed=SEED, flags=PL | abi.FLAG_TRACK_PATHS)
        hdr, vtx, counts = eng.paths()
    assert res.counter("faults") == 0 and counts["n_paths"] == 64 and counts["n_dropped"] == 0
    assert sorted(hdr["photon"]) == list(range(64))
    first = vtx[hdr["offset"], :3]
    assert np.array_equal(first, pos[hdr["photon"].astype(np.int64)])


def test_vacuum_records_and_draws():
    g = grid8()
    sc = near_vacuum(1.0)
    w = sparse_weights(g, seed=4, k=60)
    n = 20000
    pos, d, _ = host_sample(w, g, n)
    with Engine(sc, g) as eng:
        eng.set_volume_source(w)
        vol = eng.run(VOL(), n, seed=SEED, flags=PL, records=True)
        pt = eng.run(scene.point_source((0.1, 0.2, 0.3)), n, seed=SEED, flags=PL)
    r = vol.records
    assert np.all(r["status"] == 2) and np.all(r["nscatt"] == 0) and vol.counter("faults") == 0
    assert np.array_equal(r["dir"], d)
    cross = np.linalg.norm(np.cross(r["pos"] - pos, d), axis=1)
    assert np.all(cross <= 1e-12 * np.linalg.norm(r["pos"], axis=1)), float(cross.max())
    assert np.all(np.einsum("ij,ij->i", r["pos"] - pos, d) > 0.0)  # ahead of the start
    assert pt.counter("scatters") == 0
    assert vol.counter("rng_draws") == pt.counter("rng_draws") + 4 * n


# ---- 3. transport after emission --------------------------------------------------------------------
def test_beer_lambert_from_one_voxel():
    """A homogeneous, index-matched, purely absorbing box (albedo 0) that fills the grid, all weight
    in one voxel: a photon escapes when its first free path exceeds its distance l to the wall, so
    the expected escapes are sum(exp(-mua * l_i)) over the sampled photons, variance sum(p (1 - p))."""
    g = grid8()
    mua = 1.5
    sc = scene.Scene([scene.box((2.0, 2.0, 2.0), scene.mono(0.0, mua, 0.0, 1.0), 1)])
    w = np.zeros(nvox(g))
    w[2 + 8 * (5 + 8 * 3)] = 3.0
    n = 20000
    pos, d, vox = host_sample(w, g, n)
    assert np.all(vox == 2 + 8 * (5 + 8 * 3))
    with np.errstate(divide="ignore"):
        t = np.where(d > 0.0, (1.0 - pos) / d, np.where(d < 0.0, (-1.0 - pos) / d, np.inf))
    l = t.min(axis=1)
    p = np.exp(-mua * l)
    with Engine(sc, g) as eng:
        eng.set_volume_source(w)
        res = eng.run(VOL(), n, seed=SEED, flags=PL)
    assert res.counter("faults") == 0 and res.counter("scatters") == 0
    assert res.counter("escaped") + res.counter("absorbed") == n
    z = (res.counter("escaped") - p.sum()) / math.sqrt((p * (1.0 - p)).sum())
    print(f"escaped {res.counter('escaped')}, expected {p.sum():.1f}, z = {z:+.2f}")
    assert abs(z) <= 5.0


# ---- 4. twins ------------------------------------------------------------------------------------------
def test_sdf_scene_and_its_voxel_twin_emit_alike():
    g = grid8()
    sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 0.7)
    w = sparse_weights(g, seed=8, k=50)
    with Engine(sc, g) as eng:
        eng.set_volume_source(w)
        a = eng.run(VOL(), 20000, seed=SEED, flags=RS)
        twin = eng.voxelise()
    with Engine(twin, g) as veng:
        veng.set_volume_source(w)
        b = veng.run(VOL(), 20000, seed=SEED, flags=RS)
    assert a.emission.sum() == 20000 and np.array_equal(a.emission, b.emission)


# ---- 5. table semantics -----------------------------------------------------------------------------
def test_table_semantics():
    g = grid8()
    sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 0.7)
    src = scene.point_source((0.1, -0.2, 0.3))
    w1, w2 = sparse_weights(g, seed=1, k=30), sparse_weights(g, seed=2, k=30)
    tiny = np.zeros(nvox(g))
    tiny[10], tiny[11] = 1e30, 1e-30
    with Engine(sc, g) as eng:
        assert eng.volume_source_info() == {"n_positive": 0, "n_reachable": 0, "total": 0.0}
        with pytest.raises(SmcrtError, match="INVALID_ARG.*smcrt_scene_set_volume_source"):
            eng.run(VOL(), 10)
        before = eng.run(src, 3000, seed=SEED, flags=RS, records=True)
        eng.set_volume_source(w1)
        check_emission(eng, w1, g, 3000)
        eng.set_volume_source(w2)  # replaces the first
        check_emission(eng, w2, g, 3000)
        assert eng.volume_source_info()["total"] == float(np.cumsum(w2)[-1])
        after = eng.run(src, 3000, seed=SEED, flags=RS, records=True)  # a point source beside a table
        eng.set_volume_source(tiny)
        assert eng.volume_source_info() == {"n_positive": 2, "n_reachable": 1, "total": 1e30}
        one = eng.run(VOL(), 500, seed=SEED, flags=RS)
        with pytest.raises(SmcrtError, match="INVALID_ARG.*voxel 7"):
            bad = w1.copy()
            bad[7] = -1.0
            eng.set_volume_source(bad)
        assert eng.volume_source_info()["total"] == 1e30  # (a refused table leaves the old one)
        with pytest.raises(ValueError):
            eng.set_volume_source(np.ones(5))
        eng.set_volume_source(None)
        assert eng.volume_source_info()["n_positive"] == 0
        with pytest.raises(SmcrtError, match="INVALID_ARG.*smcrt_scene_set_volume_source"):
            eng.run(VOL(), 10)
    assert one.emission.reshape(-1)[10] == 500 and one.emission.sum() == 500
    assert np.array_equal(before.records, after.records) and before.counters_dict() == after.counters_dict()
    assert np.array_equal(before.absorb, after.absorb) and np.array_equal(before.emission, after.emission)


# ---- 6. refusals -----------------------------------------------------------------------------------
def test_refusals():
    g = grid8()
    sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 0.7)
    inv = abi.InverseConfig()
    inv.layer, inv.flags, inv.max_steps = 1, abi.INVERSE_FIND_MUS, 1
    with Engine(sc, g) as eng:
        eng.set_volume_source(np.ones(nvox(g)))
        for call in (lambda: eng.run_origins([(0.0, 0.0, 0.0)], 10, source=VOL()),
                     lambda: eng.escape(escape_config(grid_size=(2, 2, 2)), 10, source=VOL()),
                     lambda: eng.inverse(VOL(), inv, 10, [-1.0])):
            with pytest.raises(SmcrtError, match="UNSUPPORTED.*volume"):
                call()
        assert eng.run(VOL(), 100, seed=SEED).counter("photons") == 100  # the scene still runs
    with MultiEngine(sc, g, devices=[0]) as me:
        with pytest.raises(SmcrtError, match="UNSUPPORTED.*volume"):
            me.run(VOL(), 100)
        with pytest.raises(SmcrtError, match="UNSUPPORTED.*volume"):
            me.accumulate(VOL(), 100)


# ---- 7. fluorescence() ------------------------------------------------------------------------------
def test_fluorescence_three_layers():
    """Three stacked slabs (z in [-1, -0.25], [-0.25, 0.25], [0.25, 1]) on an 8^3 grid, whose voxel
    planes end on the slabs' faces; the fluorophore is in the middle one."""
    g = grid8()
    slabs = [(-1.0, -0.25, scene.mono(8.0, 0.5, 0.8, 1.0)), (-0.25, 0.25, scene.mono(10.0, 1.5, 0.9, 1.0)),
             (0.25, 1.0, scene.mono(4.0, 0.25, 0.7, 1.0))]
    sdfs = []
    for i, (lo, hi, opt) in enumerate(slabs):
        t = scene.invert(scene.translate((0.0, 0.0, 0.5 * (lo + hi))))
        sdfs.append(scene.box((2.0, 2.0, hi - lo), opt, i + 1, transform=t))
    sc = scene.Scene(sdfs)
    src = scene.pencil_source((0.05, 0.07, 0.999), (0.0, 0.0, -1.0))
    n_ex, n_em = 20000, 20000
    with Engine(sc, g) as eng:
        before = [eng.get_optprops(i) for i in range(3)]
        out = fluorescence(eng, src, n_ex, n_em, {2: 0.25}, emission_props={1: (6.0, 0.5, 0.5, 1.0)}, seed=SEED,
                           flags=RS)
        after = [eng.get_optprops(i) for i in range(3)]
        again = eng.run(src, n_ex, seed=SEED, flags=RS)
    w = out.weights
    assert w.shape == (8, 8, 8) and not w[:3].any() and not w[5:].any() and w[3:5].sum() > 0.0
    assert np.array_equal(w[3:5], out.excitation.absorb[3:5] * 0.25)
    em = out.emission
    assert em.emission.sum() == n_em and np.all(em.emission[w == 0.0] == 0.0)
    assert em.counter("absorbed") + em.counter("escaped") == n_em and em.counter("faults") == 0
    assert out.per_excitation_photon == w.sum() / (float(n_ex) * float(n_em))
    assert after == before
    assert np.array_equal(again.absorb, out.excitation.absorb) and again.counters_dict() == out.excitation.counters_dict()
