"""Scattering-medium layers without a GPU (DESIGN.md §3.5 "Scattering media"): (a) the reference
of tests/analytic_ref.py (scatter_cumulative) against itself, against exact moments and against
scene A's closed form, (b) the conditions on the grid and the parameters, from the reference
alone, (c) a plain numpy random walk written here, and the three CPU restatements, under the
assertions tests/test_gpu_scatter_analytic.py makes of the HIP path, and (d) negative controls:
the same assertions must reject a reference that is slightly wrong.
"""
import math
import os

import numpy as np
import pytest
from scipy import special

from oracle import pyoracle as O
from rsmcrt_amd import abi
from tests import analytic_cases as AC
from tests import analytic_ref as AR
from tests import mesh_ref as M
from tests import voxel_ref as V

RUN = {"sdf": O.run, "voxel": V.run, "mesh": M.run}
CASES = list(AC.S_CASES)
MUS, MUA = AC.S_MUS, AC.S_MUA
MUT = MUS + MUA
# photons per batch (x 24): the walk's 4.08e6 take 4 to 6 s a case; the restatements' 4.8e5 keep a
# test within 6 s of one core (the SDF restatement runs 0.1 M photons/s of these scenes)
N_WALK = 170_000
N_CPU = 40_000
# below the GPU run's count more layers are pooled: 3.1e-3 of the absorptions at 9.6e5 photons at
# the most (g = -0.5 along z), against the 1e-3 that holds at 2.016e7
CPU_POOL_CAP = 5e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_RUNS = {}


def cpu_run(case, form, flags=abi.FLAG_PATHLENGTH):
    if (case, form, flags) not in _RUNS:
        sc, src = AC.scene_s(case, form)
        g = AC.grid_s()
        _RUNS[case, form, flags] = AC.run_layers(
            lambda first, n: RUN[form](sc, g, src, n, seed=AC.SEED, first_photon=first, flags=flags),
            N_CPU, keep_grid=case == "mirror")
    return _RUNS[case, form, flags]


# --------------------------------------------------------------- a plain numpy random walk ----
def _deposit(faces, x0, x1, length):
    """The track of straight segments, projected onto one axis from x0 to x1 with the lengths
    `length`, in every layer: the cumulative F(e) = sum length * clip((e - lo) / (hi - lo), 0, 1)
    at every face e, from sorted positions alone, and its differences."""
    lo, hi = np.minimum(x0, x1), np.maximum(x0, x1)
    w = hi - lo
    flat = w < 1e-9                     # (parallel to the layers: all of it where it lies)
    rate = np.where(flat, 0.0, length / np.where(flat, 1.0, w))
    i_lo = np.searchsorted(faces, lo, side="right")   # the first face beyond lo
    i_hi = np.searchsorted(faces, hi, side="left")    # the first face at or beyond hi
    n = len(faces) + 1

    def below(idx, wts):
        return np.cumsum(np.bincount(idx, weights=wts, minlength=n))[:len(faces)]

    done = below(i_hi, length)
    inside_rate = below(i_lo, rate) - below(i_hi, rate)
    inside_start = below(i_lo, rate * lo) - below(i_hi, rate * lo)
    inside_flat = below(i_lo, np.where(flat, length, 0.0)) - below(i_hi, np.where(flat, length, 0.0))
    assert np.all(inside_flat == 0.0)
    return np.diff(done + faces * inside_rate - inside_start)


def _isotropic(rng, n):
    c = 2.0 * rng.random(n) - 1.0
    s = np.sqrt(1.0 - c * c)
    phi = 2.0 * math.pi * rng.random(n)
    return np.stack([s * np.cos(phi), s * np.sin(phi), c], axis=1)


def _henyey_greenstein(rng, d, g):
    """New directions at the angle theta to d, cos theta drawn from the Henyey-Greenstein
    distribution, the azimuth uniform, in an orthonormal frame (u, v, d) built by cross products."""
    n = len(d)
    xi = rng.random(n)
    if g == 0.0:
        c = 2.0 * xi - 1.0
    else:
        c = (1.0 + g * g - ((1.0 - g * g) / (1.0 - g + 2.0 * g * xi)) ** 2) / (2.0 * g)
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    phi = 2.0 * math.pi * rng.random(n)
    axis = np.zeros_like(d)
    axis[np.arange(n), np.argmin(np.abs(d), axis=1)] = 1.0
    u = np.cross(d, axis)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(d, u)
    return c[:, None] * d + s[:, None] * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)


def walk(case, n_batch, batches=AC.BATCHES, seed=20240607):
    """The case as an analogue random walk in an infinite medium, tallied like analytic_cases.run_layers."""
    kind, pos, direction, g = AC.S_CASES[case]
    faces = AC.faces_s()
    rng = np.random.default_rng(seed)
    a = MUS / MUT
    ab, jm = [[], [], []], [[], [], []]
    scatters = 0
    grid = np.zeros(AC.S_NZ * AC.S_NY * AC.S_NX) if case == "mirror" else None
    for _ in range(batches):
        p = np.tile(np.array(pos, dtype=np.float64), (n_batch, 1))
        d = _isotropic(rng, n_batch) if kind == "point" else np.tile(np.array(direction, dtype=np.float64), (n_batch, 1))
        sab = [np.zeros(len(f) - 1) for f in faces]
        sjm = [np.zeros(len(f) - 1) for f in faces]
        while len(p):
            s = -np.log(1.0 - rng.random(len(p))) / MUT
            q = p + s[:, None] * d
            assert np.all(np.abs(q) < np.array(AC.S_HALF)), "the walk left the grid"
            for ax in range(3):
                sjm[ax] += _deposit(faces[ax], p[:, ax], q[:, ax], s)
            p = q
            absorbed = rng.random(len(p)) >= a
            idx = [np.searchsorted(faces[ax], p[absorbed, ax], side="right") - 1 for ax in range(3)]
            for ax in range(3):
                sab[ax] += np.bincount(idx[ax], minlength=len(faces[ax]) - 1)
            if grid is not None:
                grid += np.bincount((idx[2] * AC.S_NY + idx[1]) * AC.S_NX + idx[0], minlength=len(grid))
            p, d = p[~absorbed], d[~absorbed]
            scatters += len(p)
            d = _henyey_greenstein(rng, d, g)
        for ax in range(3):
            ab[ax].append(sab[ax])
            jm[ax].append(sjm[ax])
    n = n_batch * batches
    return {"ab": [np.array(x) for x in ab], "jm": [np.array(x) for x in jm],
            "ctr": {"scatters": scatters, "absorbed": n, "escaped": 0, "faults": 0, "photons": n},
            "grid": None if grid is None else grid.reshape(AC.S_NZ, AC.S_NY, AC.S_NX)}


def walk_run(case):
    if ("walk", case) not in _RUNS:
        _RUNS["walk", case] = walk(case, N_WALK)
    return _RUNS["walk", case]


# ---------------------------------------------------------------- (a) the reference itself ----
def test_exponential_integral():
    x = np.concatenate([[0.0], np.logspace(-6, 2, 200)])
    assert np.abs(AR.exp_integral_2(x) - special.expn(2, x)).max() <= 1e-14   # reached: 1.4e-15


@pytest.mark.parametrize("case", CASES)
def test_layers_sum_to_one(case):
    """Every photon is absorbed somewhere: reached 5e-10 to 1.1e-8 (point sources) and 1.8e-8 (the
    beams' transverse axes)."""
    for p in AC.reference_s(case):
        assert abs(p.sum() - 1.0) <= 1e-6


def _moments_from_cumulative(g, mu0):
    """(<x>, <x^2>) of the absorption sites from the cumulative C(x) itself, by parts:
    <x^n> = int_0^inf n x^(n-1) (C(inf) - C(x)) dx + the same on the other side, in 16-point
    Gauss-Legendre panels 0.25 wide out to 5 (C is smooth off the source's plane)."""
    gx, gw = AR._gl(16)
    pe = np.linspace(0.0, 5.0, 21)
    x = (pe[:-1, None] + np.diff(pe)[:, None] * gx[None, :]).ravel()
    w = (np.diff(pe)[:, None] * gw[None, :]).ravel()
    c = AR.scatter_cumulative(np.concatenate([x, -x, [5.0, -5.0]]), MUS, MUA, g, mu0)
    up, down = c[-2] - c[:len(x)], c[len(x):2 * len(x)] - c[-1]     # the mass beyond x, beyond -x
    assert c[-2] - c[-1] == pytest.approx(1.0, abs=1e-6)
    return float((w * (up - down)).sum()), float((w * 2.0 * x * (up + down)).sum())


@pytest.mark.parametrize("g", [0.8, 0.0, -0.5])
def test_second_moment(g):
    """<x^2> = 2 / (3 mut^2 (1 - a)(1 - a g)): from phi_0's curvature at k = 0, by the continued
    fraction and by the banded solve, and from the layers' cumulative (reached: 1.2e-7)."""
    want = AR.scatter_moments(MUS, MUA, g)[0]
    k = np.array([1e-3])
    q = np.zeros((201, 1))
    q[0] = 1.0
    for phi in (AR.phi0_point(k, MUS, MUA, g, 200)[0], AR.phi0_solve(1j * k, MUS, MUA, g, q, 200)[0]):
        got = 2.0 * (1.0 - MUA * float(phi.real[0])) / float(k[0]) ** 2
        assert got == pytest.approx(want, rel=1e-5), (got, want)
    m1, m2 = _moments_from_cumulative(g, None)
    print(g, m1, m2, want, m2 / want - 1.0)
    assert m2 == pytest.approx(want, rel=2e-6) and abs(m1) <= 1e-8


@pytest.mark.parametrize("g", [0.8, 0.0, -0.5])
@pytest.mark.parametrize("mu0", [1.0, -1.0, 0.0])
def test_beam_first_moment(g, mu0):
    """<x> of a beam's absorption sites = mu0 / (mut (1 - a g)), from the moment generating
    function's slope at 0; for g = 0.8, and g = -0.5 along the beam, also from the layers'
    cumulative (reached: 3.3e-10)."""
    want = mu0 * AR.scatter_moments(MUS, MUA, g)[1]
    h = 1e-4
    m, ok = AR.scatter_mgf(np.array([h, -h]), MUS, MUA, g, mu0)
    assert ok.all() and (m[0] - m[1]) / (2.0 * h) == pytest.approx(want, rel=1e-6, abs=1e-9)
    if g == 0.8 or (g, mu0) == (-0.5, 1.0):
        m1, _ = _moments_from_cumulative(g, mu0)
        print(g, mu0, m1, want)
        assert m1 == pytest.approx(want, abs=1e-8)


def test_no_scattering_is_scene_a():
    """mus = 0: the layers are scene A's per-voxel closed form (point_source_track) summed over a
    grid 10 wide on either side of the source (exp(-2 * 10) of the photons get further)."""
    mu = AC.A_MU
    src = (0.09, -0.05, 0.10)
    wide = AR.faces(80, 10.0)
    xe = AR.faces(12, 1.5)
    t = AR.point_source_track(xe, wide, wide, src, mu)
    p = AR.scatter_layers_point(xe, src[0], 0.0, mu, 0.0)
    print(np.abs(mu * t.sum(axis=(0, 1)) - p).max())
    assert np.abs(mu * t.sum(axis=(0, 1)) - p).max() <= 1e-10   # reached: 8.5e-12


@pytest.mark.parametrize("g", [0.8, -0.5])
def test_continued_fraction_equals_banded_solve(g):
    k = np.concatenate([[1e-3], np.logspace(-1, 3, 60)])
    q = np.zeros((1001, 1))
    q[0] = 1.0
    a, _ = AR.phi0_point(k, MUS, MUA, g, 1000)
    b, _ = AR.phi0_solve(1j * k, MUS, MUA, g, q, 1000)
    assert np.abs(b / a - 1.0).max() <= 1e-14   # reached: 5.6e-16


# ------------------------------------------------------- (b) the conditions of the cases ----
@pytest.mark.parametrize("case", CASES)
def test_conditions(case):
    """From the reference alone: expected escapes over the GPU run at most 1e-3; enough layers with
    N p >= MIN_EVENTS on every axis, the others at most 1e-3 of the absorptions; the reference's
    own error, by doubling the k-range, the k-resolution and L, at most 1e-2 of a layer's standard
    error at the GPU run's photon count."""
    n = AC.N_GPU_S
    esc = n * AC.escape_bound(case)
    p, p2 = AC.reference_s(case), AC.reference_s(case, doubled=True)
    own = [int(np.count_nonzero(n * a >= AC.MIN_EVENTS)) for a in p]
    pooled = [float(a[n * a < AC.MIN_EVENTS].sum()) for a in p]
    err = max(float(np.abs((a - b) / np.sqrt(np.maximum(a, 1e-300) / n))[n * a >= AC.MIN_EVENTS].max()) for a, b in zip(p, p2))
    print(case, "escapes", esc, "layers", own, "pooled", pooled, "error", err)
    assert esc <= AC.S_ESCAPE_CAP
    assert min(own) >= AC.S_MIN_LAYERS[case] and max(pooled) <= AC.S_POOL_CAP
    assert err <= AC.S_REF_ERR_CAP
    assert len(set(AC.S_EDGES)) == 3 and len({AC.S_NX, AC.S_NY, AC.S_NZ}) == 3
    kind, pos, _, _ = AC.S_CASES[case]
    for a, (e, s) in enumerate(zip(AC.faces_s(), pos)):   # where the source sits in its voxel
        on_face = np.min(np.abs(e - s)) < 1e-9
        on_centre = np.min(np.abs(0.5 * (e[1:] + e[:-1]) - s)) < 1e-9
        assert (on_face, on_centre) == ((a == 1, a != 1) if case == "mirror" else (False, False))


# --------------------------------------- (c) the walk and the restatements against it ----
def _check(case, run, weighted=False):
    st = AC.evaluate_s(run, run["ctr"]["photons"] // AC.BATCHES, AC.reference_s(case), weighted=weighted)
    print(AC.flat_s(st))
    AC.check_s(st, min_layers=4, pool_cap=CPU_POOL_CAP)
    if case == "mirror":
        ms = AC.mirror_stats(run["grid"])
        print(ms)
        AC.check_mirror(ms, min_orbits=20)
    return st


@pytest.mark.parametrize("case", CASES)
def test_walk(case):
    _check(case, walk_run(case))


@pytest.mark.parametrize("form", AC.FORMS)
@pytest.mark.parametrize("case", CASES)
def test_restatement(case, form):
    run = cpu_run(case, form)
    _check(case, run)
    assert run["ctr"]["scatters"] > 2 * run["ctr"]["photons"]


@pytest.mark.parametrize("form", AC.FORMS)
def test_restatement_survival_bias(form):
    _check("iso-g0.8", cpu_run("iso-g0.8", form, abi.FLAG_PATHLENGTH | abi.FLAG_SURVIVAL_BIAS), weighted=True)


# ------------------------------------------------------------------ (d) negative controls ----
# A reference that is wrong on purpose must fail the assertions the right one passes. The photon
# count at which each control first trips a statistic (a layer group of an axis or the counter),
# found by running the SDF restatement on the ladder 2.4e5, 9.6e5, 2.52e6, 5.04e6, 1.008e7, 2.016e7
# (the right reference passes every statistic on every rung):
#   g + 1 %               iso g=0.8 and mirror 2.52e6, iso g=-0.5 5.04e6, the beams 2.4e5 (the axial layers)
#   mut + 1 %, a fixed    2.4e5 in every case (the total track is 1 / mua per photon)
#   mua + 1 %             2.4e5 (iso g=-0.5, beam +z), 9.6e5 (the others)
#   mus + 1 %             9.6e5 (beam +z), 2.52e6 (iso g=-0.5, beam -z), 5.04e6 (iso g=0.8, g=0, mirror)
#   g_2 = g, isotropic for g != 0, the beam reversed, any two axes swapped, the source moved by a
#   tenth of a voxel edge along x, y or z: 2.4e5, the lowest rung, in every case
#   S-mirror, x reversed in the voxels above the source's y: 2.4e5 (the orbits and the x halves)
# So every control is rejected below the GPU tests' 2.016e7 photons, mus + 1 % included; none is
# left uncovered. Here each control must fail on the restatement's run of (c) where its count of
# first rejection is within that run's 9.6e5, and on the SDF restatement's layer sums at 2.016e7
# photons (tests/golden/scatter_layers_*.npz, the tallies the GPU tests reproduce bit for bit).
N_CPU_TOTAL = N_CPU * AC.BATCHES
FIRST = {
    "iso-g0.8": {"g+1%": 2_520_000, "mut+1%": 240_000, "mua+1%": 960_000, "mus+1%": 5_040_000, "g2=g": 240_000,
                 "isotropic": 240_000, "x-y-swapped": 240_000, "x-z-swapped": 240_000, "y-z-swapped": 240_000,
                 "source+0.1dx": 240_000, "source+0.1dy": 240_000, "source+0.1dz": 240_000},
    "beam-z+": {"g+1%": 240_000, "mut+1%": 240_000, "mua+1%": 240_000, "mus+1%": 960_000, "g2=g": 240_000,
                "isotropic": 240_000, "reversed": 240_000, "x-y-swapped": 240_000, "x-z-swapped": 240_000,
                "y-z-swapped": 240_000, "source+0.1dx": 240_000, "source+0.1dy": 240_000, "source+0.1dz": 240_000},
    "beam-z-": {"reversed": 240_000, "g+1%": 240_000, "mus+1%": 2_520_000},
    "iso-g0": {"mut+1%": 240_000, "mus+1%": 5_040_000, "x-y-swapped": 240_000},
    "iso-g-0.5": {"g+1%": 5_040_000, "g2=g": 240_000, "isotropic": 240_000, "mus+1%": 2_520_000},
    "mirror": {"g+1%": 2_520_000, "source+0.1dx": 240_000},
}


def golden_run(case):
    if ("golden", case) not in _RUNS:
        z = np.load(os.path.join(GOLDEN, f"scatter_layers_{case}.npz"))
        n = int(z["photons"])
        _RUNS["golden", case] = {"ab": [z[f"ab{a}"].astype(np.float64) for a in range(3)], "jm": [z[f"jm{a}"] for a in range(3)],
                                 "ctr": {"scatters": int(z["scatters"]), "absorbed": n, "escaped": 0, "faults": 0, "photons": n},
                                 "grid": None}
    return _RUNS["golden", case]


@pytest.mark.parametrize("case", CASES)
def test_golden_layers_pass(case):
    """The recorded layer sums of 2.016e7 photons pass the GPU test's assertions, with its caps."""
    run = golden_run(case)
    assert run["ctr"]["photons"] == AC.N_GPU_S
    st = AC.evaluate_s(run, AC.N_GPU_S // AC.BATCHES, AC.reference_s(case))
    AC.check_s(st, min_layers=AC.S_MIN_LAYERS[case])


@pytest.mark.parametrize("case,control", [(c, k) for c in FIRST for k in FIRST[c]])
def test_control(case, control):
    assert control in AC.S_CONTROLS
    wrong = AC.reference_s(case, control)
    runs = [(golden_run(case), AC.N_GPU_S // AC.BATCHES)]
    if FIRST[case][control] <= N_CPU_TOTAL:
        runs.append((cpu_run(case, "sdf"), N_CPU))
    for run, n_batch in runs:
        AC.check_s(AC.evaluate_s(run, n_batch, AC.reference_s(case)), min_layers=4, pool_cap=CPU_POOL_CAP)
        with pytest.raises(AssertionError):
            AC.check_s(AC.evaluate_s(run, n_batch, wrong), min_layers=4, pool_cap=CPU_POOL_CAP)


def test_control_mirror_one_side():
    """S-mirror: the tally with x reversed in the voxels above the source's y only. The source's x
    layer is not the grid's middle one, so the reversal breaks every orbit."""
    run = cpu_run("mirror", "sdf")
    AC.check_mirror(AC.mirror_stats(run["grid"]), min_orbits=20)
    jf = AC.S_NY // 2
    bad = run["grid"].copy()
    bad[:, jf:, :] = bad[:, jf:, ::-1]
    ms = AC.mirror_stats(bad)
    assert ms["max_z"] > ms["z_bound"] and ms["chi2"] > ms["chi2_hi"]
    assert ms["halves"][0]["chi2"] > ms["halves"][0]["chi2_hi"]
    with pytest.raises(AssertionError):
        AC.check_mirror(ms, min_orbits=20)
