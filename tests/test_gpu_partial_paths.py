"""Partial path lengths on the GPU (include/smcrt.h "partial path lengths", ppath.h): the PPL
instantiations of voxel_kernel and mesh_kernel. The lengths are checked against closed forms, against
the pinned fluence grid (the sum of a medium's lengths is the sum of jmean over its voxels up to the
float rounding of each deposit) and, for the use they exist for, against the CPU restatement's run
of a scene with another absorption; the ordinary tallies of a tracking run are held to the CPU
restatements exactly as an untracked run's are."""
import functools
import math
import os
import re

import numpy as np
import pytest

from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd import partialpaths as PPH
from rsmcrt_amd.engine import Engine, SmcrtError
from tests import mesh_cases as M
from tests import mesh_ref as R
from tests import voxel_ref as V
from tests.geom_cases import face_source
from tests.test_gpu_mesh import GRIDS as MESH_GRIDS
from tests.test_gpu_mesh import INSIDE
from tests.test_gpu_parity import SEED, compare
from tests.test_gpu_voxel import pattern_case
from tests.test_voxel_cpu import slab_case

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH
PP = abi.FLAG_PARTIAL_PATHS
ALL = (0, 2 ** 64 - 1)  # the range trigger on every photon
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smcrt.h")
CAP = int(re.search(r"#define SMCRT_PPATH_MAX_MEDIA (\d+)", open(HEADER).read()).group(1))
VOID = scene.mono(0.0, 0.0, 0.0, 1.0)


def ref_of(sc):
    return V if isinstance(sc, scene.VoxelScene) else R


def tracked(sc, g, src, n, dets=(), flags=PL, first=0, rng=ALL, max_records=65536, seed=SEED, setup=None):
    """A tracking run: (Result with photon records, headers, lengths, counts)."""
    with Engine(sc, g, dets) as eng:
        if setup:
            setup(eng)
        eng.set_partial_paths(rng[0], rng[1], max_records)
        res = eng.run(src, n, seed=seed, flags=flags | PP, first_photon=first, records=True)
        hdr, lens, counts = eng.partial_paths()
    assert len(hdr) == len(lens) == counts["n_records"] and lens.shape[1] == sc.n_media
    return res, hdr, lens, counts


def check_sorted(hdr):
    """Records come out sorted by (photon, hit), and a photon's ordinals are 0, 1, ..."""
    key = list(zip(hdr["photon"].tolist(), hdr["hit"].tolist()))
    assert key == sorted(key)
    prev = None
    for p, h in key:
        assert h == (0 if p != prev else want), (p, h)
        prev, want = p, h + 1


# ---- the shared cases and their CPU restatements (computed once) ------------------------------------
@functools.lru_cache(maxsize=None)
def pattern():
    vs, g, src = pattern_case(2)
    return vs, g, src, V.run(vs, g, src, 2000, seed=SEED, records=True)


@functools.lru_cache(maxsize=None)
def mesh_box():
    ms, g, src = M.cube_scene(), M.grid16(), face_source()
    return ms, g, src, R.run(ms, g, src, 2000, seed=SEED, records=True)


@functools.lru_cache(maxsize=None)
def slab():
    vs, g, src, dets = slab_case()
    return vs, g, src, dets, V.run(vs, g, src, 2000, seed=SEED, dets=dets, records=True)


def slab_labels(axis, n_media=3):
    """Slabs of 3, 5 and 8 voxels along `axis` of a 16^3 grid, all index-matched voids."""
    idx = np.repeat([0, 1, 2], [3, 5, 8])
    shape = [1, 1, 1]
    shape[axis] = 16
    lab = np.broadcast_to(idx.reshape(shape), (16, 16, 16)).astype(np.uint8)  # (nx, ny, nz)
    return scene.VoxelScene(np.ascontiguousarray(lab), [VOID] * n_media), scene.grid(16, 16, 16, 1.0, 1.0, 1.0)


EPS = 2.0 ** -10  # the pencil starts this far inside the face
STRAIGHT = {"+z": (2, scene.pencil_source((0.03, 0.05, -1.0 + EPS), (0.0, 0.0, 1.0)), [0.375 - EPS, 0.625, 1.0]),
            "-x": (0, scene.pencil_source((1.0 - EPS, 0.05, 0.07), (-1.0, 0.0, 0.0)), [0.375, 0.625, 1.0 - EPS])}


def check_straight(hdr, lens, want):
    assert len(hdr) == 65 and np.all(hdr["detector"] == -1) and np.all(hdr["hit"] == 0)
    assert hdr["photon"].tolist() == list(range(65))
    assert np.all(hdr["status"] == 2) and np.all(hdr["nscatt"] == 0) and np.all(hdr["weight"] == 1.0)
    # at most 16 walls are crossed and each skips 1e-8; fp64 rounding is far below that
    for m in range(3):
        print(f"medium {m}: len {lens[0, m]!r}, thickness {want[m]!r}, short by {want[m] - lens[0, m]:.3e}")
        assert abs(lens[0, m] - want[m]) <= 17 * 1e-8, (m, lens[0, m], want[m])
    assert not lens[:, 3:].any()
    assert np.all(lens == lens[0])  # the same path 65 times: bit-identical


# ---- 1. tracking perturbs nothing ----------------------------------------------------------------
@pytest.mark.parametrize("case", [pattern, mesh_box], ids=["voxel", "mesh"])
def test_tracking_perturbs_nothing(case):
    sc, g, src, cpu = case()
    gpu, hdr, lens, counts = tracked(sc, g, src, 2000)
    compare(gpu, cpu)
    assert counts == {"n_records": 2000, "n_dropped": 0}
    assert hdr["photon"].tolist() == list(range(2000))
    for f in ("status", "layer", "nscatt", "weight", "dir"):
        assert np.array_equal(hdr[f], gpu.records[f]), f
    assert np.array_equal(hdr["start"], gpu.records["pos"])


# ---- 2. closed form, straight through --------------------------------------------------------------
@pytest.mark.parametrize("way", ["+z", "-x"])
def test_straight_through(way):
    axis, src, want = STRAIGHT[way]
    vs, g = slab_labels(axis)
    _, hdr, lens, _ = tracked(vs, g, src, 65)
    check_straight(hdr, lens, want)


# ---- 3. the tie to the pinned fluence -----------------------------------------------------------------
TIE_RTOL = 2.0 ** -23  # each deposit is float(dc) of the dc added to len: 2^-24 relative, term by term


def check_tie(lens, jmean, labels, n_media):
    """labels: the medium of each voxel, in jmean's shape; None: all media summed."""
    for m in range(n_media) if labels is not None else [None]:
        a = math.fsum(lens[:, m]) if m is not None else math.fsum(lens.ravel())
        b = math.fsum(jmean[labels == m]) if m is not None else math.fsum(jmean.ravel())
        print(f"medium {m}: sum len {a!r}, sum jmean {b!r}, rel {abs(a - b) / b:.3e}")
        assert b > 0.0 and abs(a - b) <= TIE_RTOL * b, (m, a, b)


def test_tie_to_fluence_voxel():
    vs, g, src, cpu = pattern()
    gpu, hdr, lens, counts = tracked(vs, g, src, 2000)
    assert counts == {"n_records": 2000, "n_dropped": 0} and cpu.counter("fresnel") >= 200
    check_tie(lens, gpu.jmean, vs.labels.reshape(gpu.jmean.shape), 3)
    compare(gpu, cpu)  # so the restatement's pinned grid is tied too


def test_tie_to_fluence_mesh_box():
    ms, g, src, cpu = mesh_box()
    # the box's faces lie on voxel walls, so every voxel is in one medium: asserted at the centres and corners
    c = (np.arange(16) + 0.5) / 8.0 - 1.0
    z, y, x = np.meshgrid(c, c, c, indexing="ij")  # (nz, ny, nx), the shape of jmean
    centres = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    with Engine(ms, g) as eng:
        lay, _ = eng.classify(centres)
        for dx in (-0.45, 0.45):
            for dy in (-0.45, 0.45):
                for dz in (-0.45, 0.45):
                    corner, _ = eng.classify(centres + np.array([dx, dy, dz]) / 8.0)
                    assert np.array_equal(corner, lay)
    labels = (lay - 1).reshape(16, 16, 16)
    inner = (np.abs(x) < 0.5) & (np.abs(y) < 0.5) & (np.abs(z) < 0.5)
    assert np.array_equal(labels == 0, inner) and np.array_equal(labels == 1, ~inner)
    gpu, hdr, lens, counts = tracked(ms, g, src, 2000)
    assert counts == {"n_records": 2000, "n_dropped": 0} and cpu.counter("fresnel") > 500
    check_tie(lens, gpu.jmean, labels, 2)


def test_tie_to_fluence_mesh_sphere():
    """Voxels at the sphere's surface hold two media: the tie summed over all media only."""
    ms, g, src = M.sphere_scene(2), M.grid16(), scene.point_source(INSIDE)
    gpu, hdr, lens, counts = tracked(ms, g, src, 2000)
    assert counts == {"n_records": 2000, "n_dropped": 0} and gpu.counter("fresnel") > 2000
    assert lens[:, 0].sum() > 0.0 and lens[:, 1].sum() > 0.0
    check_tie(lens, gpu.jmean, None, 2)


# ---- every PPL instantiation: grid mode x emitter, both kernels ---------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["plain", "general"])
@pytest.mark.parametrize("gm", [0, 1, 2], ids=["G0", "G1", "G2"])
@pytest.mark.parametrize("kind", ["voxel", "mesh"])
def test_instantiations(kind, gm, general):
    """The cases of test_gpu_voxel's and test_gpu_mesh's test_instantiations, tracked: the tallies
    against the restatement, and the tie (per medium on labels; summed on the icosphere)."""
    if kind == "voxel":
        sc, g, src = pattern_case(gm, general)
        labels = lambda shape: sc.labels.reshape(shape)
    else:
        n, half = MESH_GRIDS[gm]
        s = 1.0 / half
        sc = scene.MeshScene([scene.mono(10.0 * s, 0.3 * s, 0.6, 1.4), scene.mono(1.0 * s, 0.02 * s, 0.3, 1.0)], ambient=1)
        sc.add_surface(*builders.icosphere(1, 0.6 * half, (0.05 * half, 0.0, -0.1 * half)), 0, 1)
        g = scene.grid(n, n, n, half, half, half)
        src = (scene.circular_source((0.1 * half, -0.2 * half, 0.3 * half), (1.0, 2.0, 2.0), 0.5 * half) if general
               else scene.point_source((0.03 * half, 0.05 * half, 0.07 * half)))
        labels = lambda shape: None
    gpu, hdr, lens, counts = tracked(sc, g, src, 1000)
    compare(gpu, ref_of(sc).run(sc, g, src, 1000, seed=SEED, records=True))
    assert counts == {"n_records": 1000, "n_dropped": 0} and gpu.counter("fresnel") > 100
    assert np.array_equal(hdr["weight"], gpu.records["weight"]) and np.array_equal(hdr["nscatt"], gpu.records["nscatt"])
    check_tie(lens, gpu.jmean, labels(gpu.jmean.shape), sc.n_media)


# ---- 4. the detector trigger ------------------------------------------------------------------------
def test_detector_trigger():
    vs, g, src, dets, cpu = slab()
    gpu, hdr, lens, counts = tracked(vs, g, src, 2000, dets=dets)
    compare(gpu, cpu)
    assert counts["n_dropped"] == 0
    det = hdr["detector"] >= 0
    assert np.count_nonzero(det) == gpu.counter("detector_hits") > 0  # (a)
    for d in range(2):  # (b)
        assert hdr["weight"][hdr["detector"] == d].sum() == gpu.detector(d).sum() > 0
    check_sorted(hdr)  # (c)
    assert np.count_nonzero(~det) == 2000 and np.all(hdr["status"][det] == 0)
    # (d) both detectors sit in the void layers, where a leg can only end by leaving the grid: the
    # scoring leg of this scene is always the photon's last
    final = {int(h["photon"]): (h, l) for h, l in zip(hdr[~det], lens[~det])}
    for h, l in zip(hdr[det], lens[det]):
        fh, fl = final[int(h["photon"])]
        assert np.all(fl >= l)
        assert fh["status"] == 2 and fh["nscatt"] == h["nscatt"] and fh["hit"] > h["hit"]
        assert np.array_equal(fl, l)
        assert h["point_sep"] > 0.0 and np.array_equal(h["dir"], fh["dir"]) and h["layer"] == 1
    assert np.any(lens[det][:, 1] > 0.02)  # (through the slab and scattered on the way)


# ---- 5. scheduling invariance ----------------------------------------------------------------------
def test_scheduling_invariance():
    vs, g, src, _ = pattern()
    with Engine(vs, g) as eng:
        eng.set_partial_paths(*ALL, 65536)
        eng.run(src, 2000, seed=SEED, flags=PL | PP)
        whole = eng.partial_paths()
        parts = []
        for first, n in ((0, 700), (700, 1300)):
            eng.run(src, n, seed=SEED, flags=PL | PP, first_photon=first)
            parts.append(eng.partial_paths())
        assert [p[2]["n_records"] for p in parts] == [700, 1300]  # (each tracking run starts with an empty arena)
        hdr = np.concatenate([p[0] for p in parts])
        lens = np.concatenate([p[1] for p in parts])
        assert hdr.tobytes() == whole[0].tobytes() and lens.tobytes() == whole[1].tobytes()
        # across the 32-bit boundary of the photon index
        first = 2 ** 32 - 1
        eng.run(src, 65, seed=SEED, flags=PL | PP, first_photon=first)
        h65, l65, c65 = eng.partial_paths()
        assert c65 == {"n_records": 65, "n_dropped": 0}
        assert h65["photon"].tolist() == list(range(first, first + 65))
        for k in (0, 1, 64):
            eng.run(src, 1, seed=SEED, flags=PL | PP, first_photon=first + k)
            h1, l1, _ = eng.partial_paths()
            assert len(h1) == 1 and h1.tobytes() == h65[k:k + 1].tobytes() and l1.tobytes() == l65[k:k + 1].tobytes()


# ---- 6. arena limits ----------------------------------------------------------------------------------
def test_arena_limits():
    vs, g, src, _ = pattern()
    cpu = V.run(vs, g, src, 100, seed=SEED, records=True)
    gpu, hdr, lens, counts = tracked(vs, g, src, 100, max_records=10)
    assert counts == {"n_records": 10, "n_dropped": 90} and len(hdr) == 10
    compare(gpu, cpu)
    first = 1000
    cpu = V.run(vs, g, src, 100, seed=SEED, first_photon=first, records=True)
    gpu, hdr, lens, counts = tracked(vs, g, src, 100, first=first, rng=(first + 5, 7))
    assert counts == {"n_records": 7, "n_dropped": 0}
    assert hdr["photon"].tolist() == list(range(first + 5, first + 12))
    assert np.array_equal(hdr["weight"], gpu.records["weight"][5:12])
    compare(gpu, cpu)
    gpu, hdr, lens, counts = tracked(vs, g, src, 100, rng=(0, 0))
    assert counts == {"n_records": 0, "n_dropped": 0} and len(hdr) == 0 and lens.shape == (0, 3)


# ---- 7. survival bias and the volume source ------------------------------------------------------------
def test_survival_bias():
    vs, g, src, _ = pattern()
    flags = PL | abi.FLAG_SURVIVAL_BIAS
    cpu = V.run(vs, g, src, 2000, seed=SEED, flags=flags, records=True)
    gpu, hdr, lens, counts = tracked(vs, g, src, 2000, flags=flags)
    compare(gpu, cpu, exact_absorb=False)
    assert counts == {"n_records": 2000, "n_dropped": 0}
    assert np.array_equal(hdr["weight"], cpu.records["weight"]) and np.any(hdr["weight"] < 1.0)


def test_volume_source():
    """The restatement has no volume source: the untracked run of the same engine stands in for it."""
    vs, g, _, _ = pattern()
    w = np.zeros(16 ** 3)
    w[np.random.default_rng(3).choice(16 ** 3, 40, replace=False)] = 1.0
    src = scene.volume_source()
    with Engine(vs, g) as eng:
        eng.set_volume_source(w)
        plain = eng.run(src, 2000, seed=SEED, flags=PL, records=True)
    gpu, hdr, lens, counts = tracked(vs, g, src, 2000, setup=lambda eng: eng.set_volume_source(w))
    compare(gpu, plain)
    assert counts == {"n_records": 2000, "n_dropped": 0} and gpu.counter("scatters") > 2000
    check_tie(lens, gpu.jmean, vs.labels.reshape(gpu.jmean.shape), 3)


# ---- 8. white Monte Carlo: the use the feature exists for ------------------------------------------------
def test_white_monte_carlo():
    """The slab's transmission under mua = 10 from one run without absorption, against the CPU
    restatement's run of the absorbing slab. Both detectors sit in the void layers (mua = 0), so
    the part of the scoring leg behind the detector's plane does not enter the factor."""
    vs_b, g, src, dets = slab_case()
    slab_b = vs_b.media[1]
    assert slab_b.mua > 0.0
    vs_a = scene.VoxelScene(vs_b.labels, [vs_b.media[0], scene.mono(slab_b.mus, 0.0, slab_b.hgg, slab_b.n)])
    n = 20000
    gpu, hdr, lens, counts = tracked(vs_a, g, src, n, dets=dets, rng=(0, 0))
    assert counts["n_dropped"] == 0 and gpu.counter("absorbed") == 0
    sel = hdr["detector"] == 1
    w = PPH.reweight(hdr["weight"][sel], lens[sel], [0.0, 0.0], [vs_b.media[0].mua, slab_b.mua])
    per_photon = np.zeros(n)
    np.add.at(per_photon, hdr["photon"][sel].astype(np.int64), w)
    est, var_a = per_photon.mean(), per_photon.var(ddof=1)
    p_b = V.run(vs_b, g, src, n, seed=SEED + 1, dets=dets).detector(1).sum() / n
    bound = 5.0 * math.sqrt(var_a / n + p_b * (1.0 - p_b) / n)
    print(f"white Monte Carlo T = {est:.5f}, the restatement's T = {p_b:.5f}, |diff| = {abs(est - p_b):.2e}, bound {bound:.2e}")
    assert 0.0 < p_b < 1.0 and abs(est - p_b) <= bound
    assert per_photon[per_photon > 0].max() < 1.0 and gpu.detector(1).sum() / n > est  # (absorption only takes away)


# ---- 9. refusals and the cap ---------------------------------------------------------------------------
def test_refusals():
    vs, g, src, _ = pattern()
    with Engine(builders.setup_scat_test(10.0), scene.grid(8, 8, 8, 1.0, 1.0, 1.0)) as eng:
        for call in (lambda: eng.run(scene.point_source(), 10, flags=PL | PP),
                     lambda: eng.set_partial_paths(0, 10),
                     lambda: eng.set_partial_paths(None),
                     lambda: eng.partial_paths()):
            with pytest.raises(SmcrtError, match="UNSUPPORTED.*SDF scenes"):
                call()
        eng.run(scene.point_source(), 10)
    with Engine(vs, g) as eng:
        with pytest.raises(SmcrtError, match="INVALID_ARG.*smcrt_scene_set_partial_paths"):  # no configuration
            eng.run(src, 10, flags=PL | PP)
        with pytest.raises(SmcrtError, match="INVALID_ARG.*not configured"):
            eng.partial_paths()
        for bad in ((0, 10, 0), (2 ** 64 - 1, 2, 10)):
            with pytest.raises(SmcrtError, match="INVALID_ARG"):
                eng.set_partial_paths(*bad)
        eng.set_partial_paths(0, 10)
        with pytest.raises(SmcrtError, match="INVALID_ARG.*SMCRT_FLAG_PATHLENGTH"):
            eng.run(src, 10, flags=PP)
        with pytest.raises(SmcrtError, match="INVALID_ARG.*smcrt_run only"):
            eng.run_device(src, eng.config(10, SEED, PL | PP), abi.DeviceTallies())
        eng.set_partial_paths(None)
        with pytest.raises(SmcrtError, match="INVALID_ARG.*smcrt_scene_set_partial_paths"):
            eng.run(src, 10, flags=PL | PP)
        gpu = eng.run(src, 500, seed=SEED, records=True)
    compare(gpu, V.run(vs, g, src, 500, seed=SEED, records=True))


def test_media_cap():
    assert CAP == abi.PPATH_MAX_MEDIA
    axis, src, want = STRAIGHT["+z"]
    vs, g = slab_labels(axis, n_media=CAP)
    _, hdr, lens, _ = tracked(vs, g, src, 65)
    check_straight(hdr, lens, want)
    vs, g = slab_labels(axis, n_media=CAP + 1)
    with Engine(vs, g) as eng:
        with pytest.raises(SmcrtError, match=rf"UNSUPPORTED.*cap of {CAP}\b"):
            eng.set_partial_paths(*ALL)
        res = eng.run(src, 65, seed=SEED, records=True)  # the scene still runs untracked
    assert res.counter("photons") == 65 and np.all(res.records["status"] == 2)


# ---- 10. photon counts ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_photon_counts(n):
    ms, g, src = M.sphere_scene(1), M.grid16(), scene.point_source(INSIDE)
    gpu, hdr, lens, counts = tracked(ms, g, src, n)
    compare(gpu, R.run(ms, g, src, n, seed=SEED, records=True))
    assert counts == {"n_records": n, "n_dropped": 0} and hdr["photon"].tolist() == list(range(n))
    assert np.all(lens.sum(axis=1) > 0.0)
