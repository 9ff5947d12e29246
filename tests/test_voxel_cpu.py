"""Voxel media without a GPU (include/smcrt.h "voxel media").

The serial restatement of the semantics (tests/voxel_ref.c) is pinned to physics the project
already trusts: van de Hulst's slab (validation1) as labels, a straight track and a Fresnel cube
against the SDF oracle on the same geometry. Then the new entry point's validation, which runs
before any device call, and the header / abi.py mirror."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, scene
from tests import voxel_ref as V
from tests.geom_cases import MEDIUM, SUBJECT, face_source
from tests.test_gpu_phasor import PENCIL_DIR, PENCIL_START

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smcrt.h")


def cube_labels(n=16, lo=4, hi=11):
    """Medium 0 in the voxels lo..hi of every axis (the box [-0.5, 0.5]^3 on a 16^3 grid of
    half-extent 1), medium 1 around it."""
    lab = np.ones((n, n, n), dtype=np.uint8)
    lab[lo:hi + 1, lo:hi + 1, lo:hi + 1] = 0
    return lab


def cube_scenes(inner, outer):
    """The SDF scene (inner box [-0.5, 0.5]^3 in a 2 x 2 x 2 box), its voxel twin, and the grid."""
    sdf = scene.Scene([scene.box((1.0, 1.0, 1.0), inner, 1), scene.box((2.0, 2.0, 2.0), outer, 2)])
    return sdf, scene.VoxelScene(cube_labels(), [inner, outer]), scene.grid(16, 16, 16, 1.0, 1.0, 1.0)


# ---- 1. validation1 as labels ---------------------------------------------------------------
def slab_case():
    g = scene.grid(5, 5, 6, 50.0, 50.0, 0.015)  # the slab faces z = +-0.01 are voxel walls
    lab = np.ones((5, 5, 6), dtype=np.uint8)
    lab[:, :, 0] = lab[:, :, 5] = 0
    vs = scene.VoxelScene(lab, [scene.mono(0.0, 0.0, 0.0, 1.0), scene.mono(90.0, 10.0, 0.75, 1.0)])
    src = scene.pencil_source((0.0, 0.0, -0.012), (0.0, 0.0, 1.0))
    dets = [scene.circle_dect((0.0, 0.0, -0.0125), (0.0, 0.0, -1.0), 1, 20.0, 100),
            scene.circle_dect((0.0, 0.0, 0.0125), (0.0, 0.0, 1.0), 1, 20.0, 100)]
    return vs, g, src, dets


def test_slab_vdhulst(kats):
    """tools/validateHGG.py:14,26: diffuse R and T of a matched slab (a = 0.9, b = 2, g = 0.75), the
    slab being four layers of voxels between two layers of void."""
    k = kats["validation1_RT"]
    vs, g, src, dets = slab_case()
    n = 200000
    r = V.run(vs, g, src, n, dets=dets)
    R = r.detector(0).sum() / n
    T = r.detector(1).sum() / n
    print(f"R = {R:.5f} (want {k['R']}), T = {T:.5f} (want {k['T']})")
    for got, want in ((R, k["R"]), (T, k["T"])):
        sigma = math.sqrt(want * (1 - want) / n)
        assert abs(got - want) < 5 * sigma + 1e-3, (got, want)  # test_validation1_vdhulst's tolerance
    assert r.counter("faults") == 0 and r.counter("sdf_evals") == 0


# ---- 2. a straight track -----------------------------------------------------------------------
def test_straight_track_matches_sdf_oracle():
    """A pencil through two near-vacuum media: the restatement deposits what the SDF oracle does,
    voxel by voxel. Tolerance: the SDF path splits a voxel's traverse into up to ~100 sphere-trace
    pieces, each rounded to fp32 (2^-24 relative each, 1e-5 in all), and the snap moves positions
    by 1e-8 per crossing."""
    vac = scene.mono(1e-9, 0.0, 0.0, 1.0)
    sdf, vs, g = cube_scenes(vac, vac)
    src = scene.pencil_source(PENCIL_START, PENCIL_DIR)
    n = 64
    want = O.run(sdf, g, src, n)
    got = V.run(vs, g, src, n)
    assert np.array_equal(got.jmean > 0.0, want.jmean > 0.0)
    assert np.count_nonzero(want.jmean) >= 16
    err = np.abs(got.jmean - want.jmean)
    tol = 1e-5 * np.abs(want.jmean) + n * 1e-8
    print(f"straight track: {np.count_nonzero(want.jmean)} voxels, worst error / tolerance {np.max(err / tol):.3e}")
    assert np.all(err <= tol)
    assert got.counter("escaped") == want.counter("escaped") == n


# ---- 3. a Fresnel cube ---------------------------------------------------------------------------
def _batches(run, n, nb):
    """`run(first, count, result)` over nb batches: the accumulated Result and the per-batch jmean
    sums over the inner and the outer voxels."""
    inner = (cube_labels() == 0).transpose(2, 1, 0)  # (nz, ny, nx), as Result.jmean
    res, path_in, path_out, prev = None, [], [], np.zeros(inner.shape)
    for b in range(nb):
        res = run(b * (n // nb), n // nb, res)
        d = res.jmean - prev
        prev = res.jmean.copy()
        path_in.append(d[inner].sum() / (n // nb))
        path_out.append(d[~inner].sum() / (n // nb))
    return res, np.array(path_in), np.array(path_out)


def test_fresnel_cube_matches_sdf_oracle():
    """The restatement against the SDF oracle on an index-mismatched cube whose faces are voxel
    walls: six quantities, each within 5 standard errors of the difference of two independent
    runs. The two paths differ physically only within ~1e-6 of the cube's edges (blended
    calcNormal) and by the 1e-8 micro-steps. No photon and no voxel is left out."""
    sdf, vs, g = cube_scenes(SUBJECT, MEDIUM)
    src = face_source()
    n, nb = 20000, 20
    nsc = {}

    def run_v(first, count, res):
        r = V.run(vs, g, src, count, seed=1234567, first_photon=first, records=True)
        nsc.setdefault("v", []).append(r.records["nscatt"].astype(np.float64))
        return r if res is None else res.merge(r)

    def run_o(first, count, res):
        r = O.run(sdf, g, src, count, seed=7654321, first_photon=first, records=True)
        nsc.setdefault("o", []).append(r.records["nscatt"].astype(np.float64))
        return r if res is None else res.merge(r)

    rv, vin, vout = _batches(run_v, n, nb)
    ro, oin, oout = _batches(run_o, n, nb)
    assert rv.counter("photons") == ro.counter("photons") == n
    assert rv.counter("faults") == 0 and ro.counter("faults") == 0
    assert rv.counter("fresnel") > 1000

    def binom(r, num, den_count):
        p = r.counter(num) / den_count
        return p, math.sqrt(p * (1.0 - p) / den_count)

    rows = []
    for name in ("absorbed", "escaped"):
        rows.append((name + " fraction", binom(rv, name, n), binom(ro, name, n)))
    rows.append(("reflections per Fresnel event", binom(rv, "reflections", rv.counter("fresnel")),
                 binom(ro, "reflections", ro.counter("fresnel"))))
    sv, so = np.concatenate(nsc["v"]), np.concatenate(nsc["o"])
    rows.append(("mean nscatt", (sv.mean(), sv.std(ddof=1) / math.sqrt(n)), (so.mean(), so.std(ddof=1) / math.sqrt(n))))
    for name, a, b in (("path per photon, inner voxels", vin, oin), ("path per photon, outer voxels", vout, oout)):
        rows.append((name, (a.mean(), a.std(ddof=1) / math.sqrt(nb)), (b.mean(), b.std(ddof=1) / math.sqrt(nb))))
    bad = []
    for name, (a, sa), (b, sb) in rows:
        z = (a - b) / math.sqrt(sa * sa + sb * sb)
        print(f"{name}: voxel {a:.6g} +- {sa:.2g}, SDF {b:.6g} +- {sb:.2g}, z = {z:+.2f}")
        if not abs(z) < 5.0:
            bad.append((name, z))
    assert not bad, bad


# ---- 4. validation before any device call ----------------------------------------------------
def _create(L, labels, media, n_media, grid, dets=None, n_dets=0):
    h = C.c_void_p()
    lp = labels.ctypes.data_as(C.POINTER(C.c_uint8)) if labels is not None else None
    st = L.smcrt_voxel_scene_create(lp, media, n_media, C.byref(grid) if grid is not None else None, dets, n_dets, 0,
                                    C.byref(h))
    msg = L.smcrt_last_error().decode()
    if st == abi.OK:
        L.smcrt_scene_destroy(h)
    return st, msg


def test_create_validates_without_a_device(lib_path):
    from rsmcrt_amd import engine
    L = engine.load_library(lib_path)
    g = scene.grid(2, 3, 4, 1.0, 1.0, 1.0)
    lab = np.zeros(24, dtype=np.uint8)
    ok = scene.VoxelScene(lab, [scene.mono(1.0, 0.1, 0.5, 1.3), scene.mono(0.0, 0.0, 0.0, 1.0)])

    def media(*rows):
        arr = (abi.Medium * len(rows))()
        for a, (mus, mua, hgg, n) in zip(arr, rows):
            a.mus, a.mua, a.hgg, a.n = mus, mua, hgg, n
        return arr

    good = (1.0, 0.1, 0.5, 1.3)
    bad_label = lab.copy()
    bad_label[2 * 3 * 2 + 2 * 1 + 1] = 2  # voxel (1, 1, 2)
    cases = [
        ("labels NULL", (None, ok.media_array(), 2, g), "NULL"),
        ("media NULL", (lab, None, 2, g), "NULL"),
        ("grid NULL", (lab, ok.media_array(), 2, None), "NULL"),
        ("n_media 0", (lab, ok.media_array(), 0, g), "n_media"),
        ("n_media 257", (lab, (abi.Medium * 257)(), 257, g), "n_media"),
        ("label >= n_media", (bad_label, ok.media_array(), 2, g), "voxel (1, 1, 2)"),
        ("mus < 0", (lab, media((-1.0, 0.1, 0.5, 1.3)), 1, g), "medium 0"),
        ("mua < 0", (lab, media(good, (1.0, -0.1, 0.5, 1.3)), 2, g), "medium 1"),
        ("|hgg| > 1", (lab, media((1.0, 0.1, 1.5, 1.3)), 1, g), "hgg"),
        ("n <= 0", (lab, media((1.0, 0.1, 0.5, 0.0)), 1, g), "n must be"),
        ("nx < 1", (lab, ok.media_array(), 2, scene.grid(0, 3, 4, 1.0, 1.0, 1.0)), "grid"),
        ("zmax <= 0", (lab, ok.media_array(), 2, scene.grid(2, 3, 4, 1.0, 1.0, 0.0)), "grid"),
    ]
    for name, args, word in cases:
        st, msg = _create(L, *args)
        assert st == abi.ERR_INVALID_ARG, (name, st, msg)
        assert word in msg, (name, msg)
    st, msg = _create(L, lab, ok.media_array(), 2, g, None, 1)  # detectors announced but absent
    assert st == abi.ERR_INVALID_ARG and msg
    # valid arguments: a scene where there is a GPU, NO_DEVICE where there is none
    st, msg = _create(L, lab, ok.media_array(), 2, g)
    assert st == (abi.OK if engine.device_count() > 0 else abi.ERR_NO_DEVICE), (st, msg)

    for shape in ((2, 3), (2, 3, 4, 1), (0,)):
        with pytest.raises(ValueError):
            scene.VoxelScene(np.zeros(shape, dtype=np.uint8), [scene.mono(*good)])
    with pytest.raises(ValueError):
        scene.VoxelScene(np.zeros((2, 3, 4)), [])
    with pytest.raises(ValueError):
        scene.VoxelScene(np.full((2, 3, 4), 300), [scene.mono(*good)])
    with pytest.raises(ValueError):
        scene.VoxelScene(np.zeros((3, 3, 4)), [scene.mono(*good)]).check_grid(g)
    # (nx, ny, nz) indexing against the flat x-fastest order
    vol = np.arange(24).reshape(2, 3, 4)
    vs = scene.VoxelScene(vol, [scene.mono(*good)] * 24)
    assert vs.labels[1 + 2 * (2 + 3 * 3)] == vol[1, 2, 3] and np.array_equal(vs.volume(g), vol)
    assert np.array_equal(scene.VoxelScene(vs.labels, vs.media).labels, vs.labels)


# ---- 5. the header and its mirror ---------------------------------------------------------------
def test_header_mirror(lib_path, tmp_path):
    assert "smcrt_voxel_scene_create" in abi.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    assert "smcrt_voxel_scene_create" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    src = tmp_path / "layout.c"
    src.write_text("\n".join(['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
                              'printf("size %zu\\n", sizeof(smcrt_medium));',
                              'printf("version %d\\n", (int)SMCRT_ABI_VERSION);'] +
                             [f'printf("{f} %zu\\n", offsetof(smcrt_medium, {f}));' for f in ("mus", "mua", "hgg", "n")] +
                             ["return 0;}"]))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.Medium) == 32
    assert int(got["version"]) == abi.SMCRT_ABI_VERSION == 5  # (additive: the version stays)
    for f in ("mus", "mua", "hgg", "n"):
        assert int(got[f]) == getattr(abi.Medium, f).offset, f
