"""The phasor tally on the GPU (SMCRT_FLAG_PHASOR, include/smcrt.h "phasor tally").

A photon adds weight * exp(i k phase) to the voxel it leaves at every voxel wall it crosses,
phase being the emitter's start phase plus the path walked through the grid. Straight tracks
through a near-vacuum are checked against a numpy line walker (`walk`), the emitter's phase and
the per-photon wavenumber with the double-slit source, the k = 0 tally against the run's
counters, and a run with the flag against the same run without it and against the oracle on each
of the twelve PHAS instantiations of transport_kernel."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.engine import Engine, SmcrtError
from rsmcrt_amd.escape import escape_config
from tests import plan_cases, planprobe
from tests.test_gpu_parity import RTOL, SEED, compare

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH
PH = abi.FLAG_PATHLENGTH | abi.FLAG_PHASOR
SNAP = 1e-8  # update_pos puts a photon that crossed a wall at wall +- 1e-8 (inttau2.f90:393)


# ---- the line walker ----------------------------------------------------------------------
def walk(start, d, g):
    """A straight line from `start` (inside grid `g`) along unit vector `d`: the flat index (x
    fastest) of the voxel left and the path length from `start` at each voxel wall crossed, the
    crossing that leaves the grid included; and the number of walls crossed per axis."""
    start, d = np.asarray(start, dtype=np.float64), np.asarray(d, dtype=np.float64)
    n = np.array([g.nx, g.ny, g.nz])
    half = np.array([g.xmax, g.ymax, g.zmax])
    h = 2.0 * half / n
    ev = []
    for a in range(3):
        if d[a] != 0.0:
            t = (np.arange(n[a] + 1) * h[a] - half[a] - start[a]) / d[a]
            ev += [(tt, a) for tt in t if tt > 0.0]
    ev.sort()
    cells, ts, per_axis, t_prev = [], [], [0, 0, 0], 0.0
    for tt, a in ev:
        mid = start + d * (0.5 * (t_prev + tt))
        idx = np.floor((mid + half) / h).astype(int)
        if np.any(idx < 0) or np.any(idx >= n):
            break  # (the previous crossing left the grid)
        assert tt - t_prev > 1e-6, "the line passes a voxel edge too closely to say which voxel it leaves"
        cells.append(int(idx[0] + n[0] * (idx[1] + n[1] * idx[2])))
        ts.append(tt)
        per_axis[a] += 1
        t_prev = tt
    return np.array(cells), np.array(ts), per_axis


def phasor_of(cells, phases, k, nvox, weight=1.0):
    out = np.zeros(nvox, dtype=np.complex128)
    np.add.at(out, cells, weight * (np.cos(k * phases) + 1j * np.sin(k * phases)))
    return out


def near_vacuum(half):
    """One box medium of half-width `half` that no photon interacts in (mus = 1e-9, mua = 0)."""
    return scene.Scene([scene.box((2.0 * half,) * 3, scene.mono(1e-9, 0.0, 0.0, 1.0), 1)])


def assert_close(got, want, atol, what):
    """Re and Im of each cell within atol (per cell) + RTOL * |want|; prints the worst ratio first."""
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    tol = atol + RTOL * np.abs(want)
    worst = float(np.max(err / np.where(tol > 0.0, tol, 1.0)))
    print(f"{what}: max |error| {err.max():.3e}, worst error / tolerance {worst:.3e}")
    assert np.all(err <= tol), (what, int(np.argmax(err - tol)), float(err.max()))


# ---- 1. straight track, exact phases ----------------------------------------------------------
PENCIL_DIR = np.array([0.3, 0.2, -0.93]) / np.linalg.norm([0.3, 0.2, -0.93])
PENCIL_START = (-0.21, -0.13, 0.9)  # inside the top voxel layer of the 8^3 grid of half-width 1
PENCIL_K = 2.0 * math.pi / 0.37


def pencil_scene():
    return near_vacuum(2.0), scene.grid(8, 8, 8, 1, 1, 1), scene.pencil_source(PENCIL_START, PENCIL_DIR)


@pytest.mark.parametrize("n", [64, 3000])
def test_straight_track(n):
    """All N photons are the same line, so phasor == N * walker: one wave, then several blocks."""
    sc, g, src = pencil_scene()
    cells, ts, per_axis = walk(PENCIL_START, PENCIL_DIR, g)
    assert min(per_axis) >= 1 and len(set(cells)) == len(cells)  # x, y and z walls; each voxel left once
    with Engine(sc, g) as eng:
        eng.set_phasor(PENCIL_K)
        res = eng.run(src, n, seed=SEED, flags=PH)
        got = eng.phasor()
    assert res.counter("photons") == n and res.counter("faults") == 0 and res.counter("scatters") == 0
    want = n * phasor_of(cells, ts, PENCIL_K, got.size)
    # the snap to wall +- 1e-8 shifts the later geometry of a segment
    atol = 2.0 * n * PENCIL_K * len(cells) * SNAP / np.abs(PENCIL_DIR).min()
    flat = got.ravel()
    assert_close(flat, want, atol, f"straight track, N = {n}")
    visited = np.zeros(got.size, dtype=bool)
    visited[cells] = True
    assert np.all(flat[~visited] == 0.0)
    assert np.all(np.abs(flat[visited]) > 0.5 * n)  # (the tolerance is far below the values)


# ---- 2. the emitter's phase and the per-photon wavenumber: dslit -------------------------------
def test_dslit_emitter_phase():
    """Each photon's line is rebuilt from its record: backed up to the emission plane z2 and to
    the slit plane z1 = 10000 lambda - 5 (photon.f90:746-759). Its start phase is the distance
    between the two points and k = 2 pi / lambda. The sum of the walker over the photons fails if
    the emitter's phase or the sampled wavelength is dropped."""
    lam, n = 0.01, 256
    g = scene.grid(16, 16, 16, 5, 5, 5)
    src = scene.attach_spectrum(scene.dslit_source(), scene.spectrum_constant(lam))
    with Engine(near_vacuum(6.0), g) as eng:
        eng.set_phasor()
        res = eng.run(src, n, seed=SEED, flags=PH, records=True)
        got = eng.phasor().ravel()
    assert res.counter("photons") == n and res.counter("faults") == 0 and res.counter("scatters") == 0
    assert res.counter("emit_retries") == 0
    k = 2.0 * math.pi / lam
    z2 = 5.0 - (1.e-5 * (2.0 * (5.0 / 400.0)))
    z1 = (10000.0 * lam) - 5.0
    want = np.zeros(got.size, dtype=np.complex128)
    want_no_phase = np.zeros_like(want)
    atol = np.zeros(got.size)
    for r in res.records:
        pos, d = np.array(r["pos"]), np.array(r["dir"])
        emit = pos + d * ((z2 - pos[2]) / d[2])
        slit = pos + d * ((z1 - pos[2]) / d[2])
        phase0 = float(np.linalg.norm(emit - slit))
        assert 89.0 < phase0 < 92.0 and d[2] < 0.0
        cells, ts, per_axis = walk(emit, d, g)
        want += phasor_of(cells, phase0 + ts, k, got.size)
        want_no_phase += phasor_of(cells, ts, k, got.size)
        # as in test 1, per photon, over the axes whose walls the line crosses (a snap on an axis
        # only shifts the later crossings of that axis), plus the back-projection's k * 1e-9
        crossed = [a for a in range(3) if per_axis[a]]
        atol[cells] += 2.0 * k * len(cells) * SNAP / np.abs(d[crossed]).min() + k * 1e-9
    print(f"dslit: per-cell tolerance up to {atol.max():.3e}, median {np.median(atol[atol > 0]):.3e}")
    assert_close(got, want, atol, "dslit")
    assert np.all(got[atol == 0.0] == 0.0)
    # the check has teeth: without the emitter's phase the same cells miss by far more than atol
    miss = np.maximum(np.abs((want_no_phase - want).real), np.abs((want_no_phase - want).imag))
    assert np.count_nonzero(miss > 10.0 * atol) > np.count_nonzero(atol) // 2


# ---- 3. k = 0 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("survival", [False, True], ids=["unit-weights", "survival-bias"])
def test_k_zero_counts_wall_crossings(survival):
    """With k = 0 the tally is real: the weight that left each voxel through a wall. Every segment
    (update_grids call) has at most one piece that ends inside a voxel, hence the counter bounds;
    with k = 40 and the same photons no cell can exceed its k = 0 value."""
    sc, g, src = plan_cases.fresnel_sphere(), scene.grid(16, 16, 16, 1, 1, 1), scene.point_source()
    flags = PH | (abi.FLAG_SURVIVAL_BIAS if survival else 0)
    with Engine(sc, g) as eng:
        eng.set_phasor(0.0)
        r0 = eng.run(src, 2000, seed=SEED, flags=flags)
        p0 = eng.phasor()
        eng.set_phasor(40.0)  # (a new configuration starts from a zero grid)
        rk = eng.run(src, 2000, seed=SEED, flags=flags)
        pk = eng.phasor()
    assert r0.counters_dict() == rk.counters_dict()
    assert r0.counter("scatters") > 2000 and r0.counter("fresnel") > 0
    assert np.all(p0.imag == 0.0)
    dep, upd = r0.counter("deposits"), r0.counter("grid_updates")
    total = p0.real.sum()
    if not survival:
        assert np.array_equal(p0.real, np.rint(p0.real)) and p0.real.min() >= 0.0
        assert dep - upd <= total <= dep, (dep, upd, total)
    else:
        assert 0.0 < total < dep  # (weights below 1)
    print(f"k = 0: sum Re {total}, deposits {dep}, grid updates {upd}; k = 40: max |phasor| / Re_0 "
          f"{np.max(np.abs(pk)[p0.real > 0] / p0.real[p0.real > 0]):.6f}")
    assert np.all(np.abs(pk) <= p0.real * (1.0 + 1e-12))


# ---- 4. the flag changes nothing else, on each of the twelve instantiations ---------------------
# grid mode -> nx, ny, nz, half-extent (plan_cases.GRIDS' kinds at no more than 16^3: 2: every
# 2 * max and n a power of two; 1: every 2 * max only; 0: neither)
SMALL_GRIDS = {2: (16, 16, 16, 1.0), 1: (12, 12, 12, 1.0), 0: (12, 12, 12, 0.05)}


def wall_source():  # test_far_field_march's: photons that march ~2/1e-3 steps along a side wall
    return scene.uniform_source((-1.0, -1.0, 0.9999999), (1e-3, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, 0.0, -1.0))


def forty_spheres():
    return builders.setup_sphere_scene(builders.random_sphere_list(40))


def _flag_cases():
    out = []
    for gm in (2, 1, 0):
        for xsrc in (0, 1):
            for coop in (0, 1):
                point = plan_cases.point_off_face if gm == 0 else scene.point_source
                src = (plan_cases.circular_small if gm == 0 else plan_cases.circular) if xsrc else point
                out.append((f"G{gm}-x{xsrc}-c{coop}", plan_cases.coop_spheres if coop else plan_cases.sphere,
                            SMALL_GRIDS[gm], src, 2000, gm, xsrc, coop, False))
    # COOP scenes whose lone wall photons take the far-field march without the flag
    out.append(("G2-x0-c1-far", forty_spheres, SMALL_GRIDS[2], wall_source, 100, 2, 0, 1, True))
    return out


FLAG_CASES = _flag_cases()


@pytest.mark.parametrize("case", FLAG_CASES, ids=[c[0] for c in FLAG_CASES])
def test_flag_changes_nothing_else(case, monkeypatch):
    """transport_kernel<false, GM, XSRC, COOP, false, PHAS = true> against <.., PHAS = false> and
    the oracle: counters (WAVE_ITERS aside), records, absorb, emission and detector bins equal,
    jmean at 1e-12. The far march and glance are skipped with the flag (far_steps == 0) and the
    ordinary path gives the same photons."""
    name, make_scene, (nx, ny, nz, ext), make_src, n, gm, xsrc, coop, far = case
    monkeypatch.setenv("SMCRT_LEAN", "0")  # (without the flag too: the same kernel but for PHAS)
    sc, g, src = make_scene(), scene.grid(nx, ny, nz, ext, ext, ext), make_src()
    plan = planprobe.plan(sc, g, env={"SMCRT_LEAN": "0"})
    assert plan["status"] == abi.OK, plan["error"]
    assert plan["grid_mode"] == gm and (plan["coop_lanes"] > 0) == bool(coop)
    assert plan_cases.kernel_of(plan, xsrc)[0] == "transport_kernel"
    assert (src.kind not in (abi.SRC_POINT, abi.SRC_PENCIL, abi.SRC_UNIFORM)) == bool(xsrc)
    with Engine(sc, g) as eng:
        eng.kernel_times()
        plain = eng.run(src, n, seed=SEED, flags=PL, records=True)
        kt_plain = eng.kernel_times()
        eng.set_phasor(3.0)
        flagged = eng.run(src, n, seed=SEED, flags=PH, records=True)
        kt_flag = eng.kernel_times()
        ph = eng.phasor()
    assert kt_plain["lean_launches"] == 0 and kt_flag["lean_launches"] == 0
    assert kt_flag["far_steps"] == 0, kt_flag
    if far:
        assert kt_plain["far_steps"] > plain.counter("grid_updates") // 2, kt_plain  # (it would have run)
    compare(flagged, plain)  # (counters_dict leaves the engine's WAVE_ITERS out)
    cpu = O.run(sc, g, src, n, seed=SEED, flags=PL, records=True)
    assert cpu.counter("photons") == n and cpu.counter("faults") == 0
    compare(flagged, cpu)
    compare(plain, cpu)
    assert np.count_nonzero(ph) > 0 and np.all(np.abs(ph) <= flagged.counter("deposits"))


# ---- 5. accumulate, reset, and who refuses the flag ----------------------------------------------
def test_accumulate_and_reset():
    sc, g, src = pencil_scene()
    with Engine(sc, g) as eng:
        eng.set_phasor(PENCIL_K)
        eng.run(src, 100, seed=SEED, flags=PH)
        a = eng.phasor()
        eng.reset_phasor()
        assert np.all(eng.phasor() == 0.0)
        eng.run(src, 50, seed=SEED, flags=PH, first_photon=100)
        b = eng.phasor()
        eng.reset_phasor()
        eng.run(src, 100, seed=SEED, flags=PH)
        eng.run(src, 50, seed=SEED, flags=PH, first_photon=100)
        both = eng.phasor()
        np.testing.assert_allclose(both, a + b, rtol=RTOL, atol=1e-300)
        assert np.count_nonzero(a) > 10
        # a run without the flag leaves the grid alone
        eng.run(src, 50, seed=SEED, flags=PL)
        assert np.array_equal(eng.phasor(), both)
        # the reader adds into its output
        out = np.ones(2 * g.nx * g.ny * g.nz)
        from rsmcrt_amd.engine import _check, load_library
        _check(load_library().smcrt_scene_read_phasor(eng._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        assert np.array_equal(out[0::2], 1.0 + both.real.ravel()) and np.array_equal(out[1::2], 1.0 + both.imag.ravel())
        eng.reset_phasor()
        assert np.all(eng.phasor() == 0.0)
        eng.set_phasor(None)
        with pytest.raises(SmcrtError, match="INVALID_ARG"):
            eng.run(src, 10, seed=SEED, flags=PH)
        with pytest.raises(SmcrtError, match="INVALID_ARG"):
            eng.phasor()
        with pytest.raises(SmcrtError, match="INVALID_ARG"):
            eng.reset_phasor()


def test_refusals():
    sc, g, src = pencil_scene()
    with Engine(sc, g) as eng:
        with pytest.raises(SmcrtError, match="INVALID_ARG"):  # the flag without a configured scene
            eng.run(src, 10, seed=SEED, flags=PH)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(SmcrtError, match="INVALID_ARG"):
                eng.set_phasor(bad)
        with pytest.raises(SmcrtError, match="INVALID_ARG"):  # (a refused configuration configures nothing)
            eng.run(src, 10, seed=SEED, flags=PH)
        eng.set_phasor()
        with pytest.raises(SmcrtError, match="INVALID_ARG"):  # the tally lives in the voxel walk
            eng.run(src, 10, seed=SEED, flags=abi.FLAG_PHASOR)
        eng.set_path_tracking(range_count=10)
        with pytest.raises(SmcrtError, match="UNSUPPORTED"):
            eng.run(src, 10, seed=SEED, flags=PH | abi.FLAG_TRACK_PATHS)
        with pytest.raises(SmcrtError, match="INVALID_ARG"):  # smcrt_run only
            eng.run_origins([(0.0, 0.0, 0.0)], 10, flags=PH)
        with pytest.raises(SmcrtError, match="INVALID_ARG"):
            eng.run_device(src, eng.config(10, SEED, PH), abi.DeviceTallies())
        with pytest.raises(SmcrtError, match="INVALID_ARG"):
            eng.escape(escape_config(grid_size=(2, 2, 2)), 10, flags=PH)
        inv = abi.InverseConfig()
        inv.layer, inv.flags, inv.max_steps = 1, abi.INVERSE_FIND_MUS, 1
        with pytest.raises(SmcrtError, match="INVALID_ARG"):
            eng.inverse(src, inv, 10, [-1.0], flags=PH)
        assert np.all(eng.phasor() == 0.0)  # none of them tallied anything
        eng.run(src, 10, seed=SEED, flags=PH)
        assert np.count_nonzero(eng.phasor()) > 10
