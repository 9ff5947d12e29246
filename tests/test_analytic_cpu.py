"""Closed-form grids without a GPU: (a) tests/analytic_ref.py against itself and
against scipy's adaptive quadrature, (b) the CPU restatements of the three kernel families against
it, with the assertions tests/test_gpu_analytic.py makes of the HIP path, and (c) negative
controls: the same assertions must reject a reference that is slightly wrong.
"""
import ast
import math

import numpy as np
import pytest
from scipy import integrate

from oracle import pyoracle as O
from rsmcrt_amd import abi
from tests import analytic_cases as AC
from tests import analytic_ref as AR
from tests import mesh_ref as M
from tests import voxel_ref as V

RUN = {"sdf": O.run, "voxel": V.run, "mesh": M.run}
# photons per batch (x 24): A needs 7e6 for N p_v >= 100 in every voxel; B and C keep a test
# within 10 s of one core (the SDF restatement runs 0.33 M and 0.3 M photons/s on them)
N_BATCH = {"a": 300_000, "b": 80_000, "c": 100_000}
_RUNS = {}


def cpu_run(which, form):
    """(jmean per batch, absorb per batch, counters) of the restatement of `form`, run once."""
    if (which, form) not in _RUNS:
        sc, src = getattr(AC, "scene_" + which)(form)
        g = AC.grid()
        _RUNS[which, form] = AC.run_batches(
            lambda first, n: RUN[form](sc, g, src, n, seed=AC.SEED, first_photon=first, flags=abi.FLAG_PATHLENGTH),
            N_BATCH[which])
    return _RUNS[which, form]


# ---------------------------------------------------------------- (a) the reference itself ----
# The tolerances below are the agreement these checks reach, times five to ten for another libm;
# they are properties of the quadratures (32 Gauss-Legendre points per axis and panel), not of
# the engine.
TOL_CLOSURE = 2e-15      # reached: 2.2e-16
TOL_DIRECT = 1e-11       # reached: 1.9e-12 (the worst are the voxels next to the source's, 0.05 away from it)
TOL_ORDER = 1e-11        # 32 against 48 points: 1.8e-12
TOL_SCIPY = 5e-12        # reached: 4.5e-13 for the source's voxel over directions, 2e-14 for the Cartesian ones


def test_reference_imports_nothing_of_the_project():
    with open(AR.__file__) as f:
        tree = ast.parse(f.read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names <= {"__future__", "math", "numpy"}, names


def test_point_source_closure():
    """sum_V mua T(V) + P(escape) = 1, the escape integrated on its own over the six outer faces."""
    t, p = AC.reference_a()
    esc = AR.point_source_escape(*AC.faces(), AC.A_SRC, AC.A_MU)
    assert 0.05 < esc < 0.5 and abs(p.sum() + esc - 1.0) <= TOL_CLOSURE
    assert t.shape == (AC.NZ, AC.NY, AC.NX) and np.all(t > 0.0)


def test_point_source_against_direct_quadrature():
    """Every voxel but the source's: the pyramid sums against a tensor Gauss-Legendre integral of
    exp(-mu r) / (4 pi r^2) over the voxel itself."""
    t, _ = AC.reference_a()
    direct = AR.point_source_track_direct(*AC.faces(), AC.A_SRC, AC.A_MU)
    rel = np.abs(direct / t - 1.0)
    assert np.isnan(rel).sum() == 1
    print("largest relative difference", np.nanmax(rel))
    assert np.nanmax(rel) <= TOL_DIRECT
    finer = AR.point_source_track(*AC.faces(), AC.A_SRC, AC.A_MU, order=48)
    assert np.abs(finer / t - 1.0).max() <= TOL_ORDER


def _voxel_box(i, j, k):
    xe, ye, ze = AC.faces()
    return (xe[i], xe[i + 1]), (ye[j], ye[j + 1]), (ze[k], ze[k + 1])


def test_point_source_against_scipy():
    """A handful of voxels by adaptive quadrature: the source's voxel as an integral over directions
    of (1 - exp(-mu rho)) / (4 pi mu), rho the distance to the voxel's wall, in nested quads split at
    the kinks of rho (the azimuths of the voxel's vertical edges, the polar angles of its horizontal
    ones); a neighbour, a mid-range and a corner voxel in Cartesian
    coordinates."""
    t, _ = AC.reference_a()
    mu, s = AC.A_MU, AC.A_SRC
    xe, ye, ze = AC.faces()
    i, j, k = (int(np.searchsorted(e, c)) - 1 for e, c in zip((xe, ye, ze), s))
    box = _voxel_box(i, j, k)

    h_bot, h_top = s[2] - box[2][0], box[2][1] - s[2]

    def lateral(phi):  # the horizontal distance to the voxel's side walls along azimuth phi
        return min(((b[1] if dc > 0.0 else b[0]) - c) / dc
                   for b, c, dc in zip(box[:2], s[:2], (math.cos(phi), math.sin(phi))) if dc != 0.0)

    def phi_of(cost, r_lat):
        rho = min(r_lat / math.sqrt(1.0 - cost * cost) if abs(cost) < 1.0 else math.inf,
                  h_top / cost if cost > 0.0 else math.inf, h_bot / -cost if cost < 0.0 else math.inf)
        return -math.expm1(-mu * rho) / (4.0 * math.pi * mu)

    def over_cost(phi):  # rho has kinks where the exit changes from the bottom to a side wall and on to the top
        r_lat = lateral(phi)
        cuts = [-1.0, -h_bot / math.hypot(h_bot, r_lat), h_top / math.hypot(h_top, r_lat), 1.0]
        return sum(integrate.quad(phi_of, a, b, args=(r_lat,), epsabs=1e-16, epsrel=1e-13)[0] for a, b in zip(cuts, cuts[1:]))

    corners = sorted(math.atan2(y - s[1], x - s[0]) for x in box[0] for y in box[1])  # the kinks of lateral()
    corners.append(corners[0] + 2.0 * math.pi)
    total = sum(integrate.quad(over_cost, a, b, epsabs=1e-16, epsrel=1e-13)[0] for a, b in zip(corners, corners[1:]))
    print("source voxel", total, t[k, j, i], total / t[k, j, i] - 1.0)
    assert abs(total / t[k, j, i] - 1.0) <= TOL_SCIPY

    def f(z, y, x):
        r2 = (x - s[0]) ** 2 + (y - s[1]) ** 2 + (z - s[2]) ** 2
        return math.exp(-mu * math.sqrt(r2)) / (4.0 * math.pi * r2)

    for ii, jj, kk in ((i + 1, j, k), (1, 9, 7), (AC.NX - 1, 0, AC.NZ - 1)):
        (x0, x1), (y0, y1), (z0, z1) = _voxel_box(ii, jj, kk)
        v, _ = integrate.tplquad(f, x0, x1, y0, y1, z0, z1, epsabs=1e-14, epsrel=1e-10)
        print((ii, jj, kk), v, t[kk, jj, ii], v / t[kk, jj, ii] - 1.0)
        assert abs(v / t[kk, jj, ii] - 1.0) <= TOL_SCIPY


def test_beam_straight_through():
    """n = 1 inside: no interface acts, the beam is one straight leg. Its tracks sum to the chord
    through the grid, and the absorbed fraction is 1 - exp(-mu * (its length inside the slab))."""
    xe, ye, ze = AC.faces()
    d = np.array(AC.B_DIR) / np.linalg.norm(AC.B_DIR)
    o = np.array(AC.B_ORIGIN)
    t, p = AR.beam_slab(xe, ye, ze, o, d, AC.Z_HALF, 1.0, AC.B_MU)
    s_in, s_out = (AC.Z_HALF - o[2]) / d[2], (-AC.Z_HALF - o[2]) / d[2]
    s_exit = min(((e[-1] if dc > 0 else e[0]) - oc) / dc for e, oc, dc in zip((xe, ye, ze), o, d))
    assert s_in < s_out < s_exit  # (the beam leaves through the bottom face, below the slab)
    a = math.exp(-AC.B_MU * (s_out - s_in))
    assert p.sum() == pytest.approx(1.0 - a, rel=1e-13)
    assert t.sum() == pytest.approx(s_in + (1.0 - a) / AC.B_MU + a * (s_exit - s_out), rel=1e-13)
    assert np.all(p[t == 0.0] == 0.0) and 10 < np.count_nonzero(t) < 30


def test_beam_series_in_a_wide_slab():
    """On a grid far wider than the beam's walk every leg stays inside, and the absorbed fraction
    is the geometric series (1 - R)(1 - a) / (1 - R a), a = exp(-mu L), L one pass through the slab."""
    wide = np.array([-1e4, 1e4])
    ze = np.array([-AC.HALF[2], -AC.Z_HALF, AC.Z_HALF, AC.HALF[2]])
    t, p = AR.beam_slab(wide, wide, ze, AC.B_ORIGIN, AC.B_DIR, AC.Z_HALF, AC.B_N_IN, AC.B_MU)
    cos1 = abs(AC.B_DIR[2]) / math.sqrt(sum(c * c for c in AC.B_DIR))
    r, cos2 = AR.fresnel_unpolarised(cos1, 1.0, AC.B_N_IN)
    r_back, _ = AR.fresnel_unpolarised(cos2, AC.B_N_IN, 1.0)
    assert r_back == pytest.approx(r, rel=1e-12) and 0.03 < r < 0.08
    a = math.exp(-AC.B_MU * 2.0 * AC.Z_HALF / cos2)
    assert p[1, 0, 0] == pytest.approx((1.0 - r) * (1.0 - a) / (1.0 - r * a), rel=1e-12)
    assert p[0, 0, 0] == 0.0 and p[2, 0, 0] == 0.0 and t[0, 0, 0] > 0.0 and t[2, 0, 0] > 0.0


# ----------------------------------------------- (b) the restatements against the reference ----
@pytest.mark.parametrize("form", AC.FORMS)
def test_restatement_point_source(form):
    """Scene A at 7.2e6 photons: 960 voxels, none pooled."""
    jm, ab, ctr = cpu_run("a", form)
    st = AC.evaluate_ab("a", jm, ab, ctr, N_BATCH["a"], AC.reference_a())
    print(st)
    AC.check_ab(st)


@pytest.mark.parametrize("form", AC.FORMS)
def test_restatement_beam(form):
    """Scene B at 1.92e6 photons."""
    jm, ab, ctr = cpu_run("b", form)
    st = AC.evaluate_ab("b", jm, ab, ctr, N_BATCH["b"], AC.reference_b(form))
    print(st)
    AC.check_ab(st)
    assert ctr["fresnel"] > ctr["photons"] and ctr["reflections"] > 0
    big = AC.reference_b(form)[0] > 1e-3
    assert np.abs(jm.sum(axis=0)[big] / (st["n"] * AC.reference_b(form)[0][big]) - 1.0).max() < 0.01


@pytest.mark.parametrize("form", AC.FORMS)
def test_restatement_estimators(form):
    """Scene C at 2.4e6 photons."""
    jm, ab, ctr = cpu_run("c", form)
    st = AC.evaluate_c(jm, ab, ctr)
    print(st)
    AC.check_c(st)
    assert ctr["scatters"] > 4 * ctr["photons"] and ctr["fresnel"] > 0 and ctr["reflections"] > 0


def test_mesh_surface_in_a_voxel_wall_faults():
    """Why the mesh form's planes lie MESH_INSET inside the walls: with the planes in the walls every
    photon that enters the slab is a counted fault (the leg from the surface finds its cell on the
    other side of the wall), never a silent wrong tally."""
    from rsmcrt_amd import builders, scene
    ms = scene.MeshScene([scene.mono(0.0, AC.B_MU, 0.0, AC.B_N_IN), scene.mono(0.0, 0.0, 0.0, 1.0)], ambient=1)
    ms.add_surface(*builders.box_mesh((-10.0, -10.0, -AC.Z_HALF), (10.0, 10.0, AC.Z_HALF)), 0, 1)
    r = M.run(ms, AC.grid(), AC.scene_b("mesh")[1], 2000, seed=AC.SEED)
    assert r.counter("faults") + r.counter("escaped") == 2000 and r.counter("faults") > 1800
    assert r.counter("absorbed") == 0 and not r.absorb.any()


# ------------------------------------------------------------------ (c) negative controls ----
# A reference that is wrong on purpose must fail the assertions the right one passes, on the runs
# of (b), which have fewer photons than any GPU test. Each control names the groups of statistics
# it must trip here. The smallest photon count at which a control first trips a statistic, found
# by running the SDF restatement on the ladders A 2.4e4, 7.2e4, 2.4e5, 7.2e5, 2.4e6, 7.2e6;
# B 6e3, 2.4e4, 9.6e4, 4.8e5, 1.92e6; C 2.4e4, 7.2e4, 2.4e5, 7.2e5, 2.4e6 (the right reference
# passes every statistic on every rung):
#   A  mu + 1 %: 7.2e5 (counter and tracks; the counts from 2.4e6). Source moved by a tenth of an
#      edge along x, y or z, and axes x-y, x-z or y-z swapped: 2.4e4, the lowest rung (counts, tracks).
#   B  mu + 1 %: 9.6e4 (tracks; counts and counter from 4.8e5). Origin moved along x, y or z, any
#      two axes swapped, n = 1.45: 6e3, the lowest rung (counts, tracks, tallies off the support).
#      One polarisation: 6e3 (s: counter and tracks, p: tracks; all three groups from 9.6e4).
#   C  mua + 1 %: 2.4e5. Axes x-z or y-z swapped: 2.4e4, the lowest rung. (mua depends on z alone,
#      so an x-y swap leaves C's expectation as it is; A and B reject that one.)
def _moved(p, axis):
    q = list(p)
    q[axis] += 0.1 * AC.EDGES[axis]
    return tuple(q)


A_CONTROLS = {
    "mu+1%": (lambda: AC.reference_a(mu=1.01 * AC.A_MU), ("counts", "counter", "tracks")),
    "source+0.1dx": (lambda: AC.reference_a(src=_moved(AC.A_SRC, 0)), ("counts", "tracks")),
    "source+0.1dy": (lambda: AC.reference_a(src=_moved(AC.A_SRC, 1)), ("counts", "tracks")),
    "source+0.1dz": (lambda: AC.reference_a(src=_moved(AC.A_SRC, 2)), ("counts", "tracks")),
    "x-y-swapped": (lambda: AC.reference_a(swap="xy"), ("counts", "tracks")),
    "x-z-swapped": (lambda: AC.reference_a(swap="xz"), ("counts", "tracks")),
    "y-z-swapped": (lambda: AC.reference_a(swap="yz"), ("counts", "tracks")),
}
B_CONTROLS = {
    "mu+1%": (lambda: AC.reference_b(mu=1.01 * AC.B_MU), ("counts", "counter", "tracks")),
    "origin+0.1dx": (lambda: AC.reference_b(origin=_moved(AC.B_ORIGIN, 0)), ("counts", "tracks")),
    "origin+0.1dy": (lambda: AC.reference_b(origin=_moved(AC.B_ORIGIN, 1)), ("counts", "tracks")),
    "origin+0.1dz": (lambda: AC.reference_b(origin=_moved(AC.B_ORIGIN, 2)), ("counts", "tracks")),
    "x-y-swapped": (lambda: AC.reference_b(swap="xy"), ("counts", "tracks")),
    "x-z-swapped": (lambda: AC.reference_b(swap="xz"), ("counts", "tracks")),
    "y-z-swapped": (lambda: AC.reference_b(swap="yz"), ("counts", "tracks")),
    "n=1.45": (lambda: AC.reference_b(n_in=1.45), ("counts", "counter", "tracks")),
    "s-polarised": (lambda: AC.reference_b(polarisation="s"), ("counts", "counter", "tracks")),
    "p-polarised": (lambda: AC.reference_b(polarisation="p"), ("counts", "counter", "tracks")),
}


def _must_fail(st, groups):
    with pytest.raises(AssertionError):
        AC.check_ab(st)
    if "counts" in groups:
        with pytest.raises(AssertionError):
            AC.check_counts(st["counts"])
    if "counter" in groups:
        assert abs(st["z_absorbed"]) > st["z_bound"] and abs(st["z_escaped"]) > st["z_bound"]
    if "tracks" in groups:
        with pytest.raises(AssertionError):
            AC.check_batches(st["tracks"])


@pytest.mark.parametrize("control", list(A_CONTROLS))
def test_control_point_source(control):
    ref, groups = A_CONTROLS[control]
    jm, ab, ctr = cpu_run("a", "sdf")
    AC.check_ab(AC.evaluate_ab("a", jm, ab, ctr, N_BATCH["a"], AC.reference_a()))
    _must_fail(AC.evaluate_ab("a", jm, ab, ctr, N_BATCH["a"], ref()), groups)


@pytest.mark.parametrize("control", list(B_CONTROLS))
def test_control_beam(control):
    ref, groups = B_CONTROLS[control]
    jm, ab, ctr = cpu_run("b", "sdf")
    AC.check_ab(AC.evaluate_ab("b", jm, ab, ctr, N_BATCH["b"], AC.reference_b()))
    _must_fail(AC.evaluate_ab("b", jm, ab, ctr, N_BATCH["b"], ref()), groups)


@pytest.mark.parametrize("control", ["mua+1%", "x-z-swapped", "y-z-swapped"])
def test_control_estimators(control):
    jm, ab, ctr = cpu_run("c", "sdf")
    AC.check_c(AC.evaluate_c(jm, ab, ctr))
    m = AC.mua_c()
    wrong = 1.01 * m if control == "mua+1%" else AC.swapped(m, control[0] + control[2])
    with pytest.raises(AssertionError):
        AC.check_batches(AC.evaluate_c(jm, ab, ctr, mua=wrong))
