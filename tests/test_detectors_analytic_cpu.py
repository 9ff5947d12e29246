"""Closed-form detector bins without a GPU: (a) the detector expectations of
tests/analytic_ref.py against independent quadratures, (b) the CPU restatements of the three kernel
families against them, with the assertions tests/test_gpu_detectors_analytic.py makes of the HIP
path, and (c) negative controls: the same assertions must reject a reference that misreads one of
the hit rules. `python -m tests.test_detectors_analytic_cpu predict` prints the statistics of the
GPU-sized runs (PREDICTED in the GPU file), `... ladder` the photon counts at which each control
first fails.

Photons per case here (N_CPU): A 3e6 (1.6e7 in the SDF form, on which the controls are judged),
B 1e6, C 2e5, origins 1e6 and escape cells 5e5 each. The SDF restatement runs 1.3 M photons/s on A
and 0.25 M/s on B; the file takes 33 s of one core.
"""
import math
import sys

import numpy as np
import pytest
from scipy import integrate

from oracle import pyoracle as O
from rsmcrt_amd import abi, scene
from tests import analytic_cases as AC
from tests import analytic_ref as AR
from tests import mesh_ref as M
from tests import voxel_ref as V

RUN = {"sdf": O.run, "voxel": V.run, "mesh": M.run}
N_CPU = {"a": 3_000_000, "b": 1_000_000, "c": 200_000, "o": 1_000_000, "escape": 500_000}
N_CPU_A_SDF = 16_000_000   # the run the controls are judged on: a centre off by 0.1 w needs 1e7
PL = abi.FLAG_PATHLENGTH
_RUNS = {}


def n_cpu(which, form):
    return N_CPU_A_SDF if (which, form) == ("a", "sdf") else N_CPU[which]


def cpu_run(which, form, n=None, flags=PL):
    """(bins per detector, counters) of the restatement of `form` on detector set `which`."""
    n = n_cpu(which, form) if n is None else n
    key = (which, form, n, flags)
    if key not in _RUNS:
        sc, src = getattr(AC, "scene_" + which)(form)
        dets = AC.dets_b(form) if which == "b" else getattr(AC, "dets_" + which)()
        r = RUN[form](sc, AC.grid(), src, n, seed=AC.SEED, flags=flags, dets=dets)
        _RUNS[key] = ([r.detector(i).copy() for i in range(len(dets))], r.counters_dict())
    return _RUNS[key]


def cpu_origins(n=None, origins=AC.DO_ORIGINS):
    """totals[k, d] as the reference gets them: one run per origin."""
    n = N_CPU["o"] if n is None else n
    key = ("o", n, origins)
    if key not in _RUNS:
        sc, _ = AC.scene_a("sdf")
        dets = AC.dets_o()
        tot = np.zeros((len(origins), len(dets)))
        for k, o in enumerate(origins):
            r = O.run(sc, AC.grid(), scene.point_source(o), n, seed=AC.SEED, flags=PL, dets=dets)
            tot[k] = [r.detector(d).sum() for d in range(len(dets))]
        _RUNS[key] = tot
    return _RUNS[key]


# ---------------------------------------------------------------- (a) the reference itself ----
# Condition, not measurement: in every bin the error of the reference's N p is below 1 % of the
# bin's binomial standard error sqrt(N p (1 - p)) at N = AC.N_GPU. Measured, as the largest ratio of
# |difference| to that standard error over the bins: circle 3.1e-12, annulus 3.1e-12 (against
# dblquad over the discs in Cartesian plane coordinates), camera 2.3e-12, fibre 4.3e-3 (the
# enumeration's grid of 2.5e-7 in r places each edge to half a step; the first bin is 2.3e-3 wide).
REF_SHARE = 0.01


def _se(p, n=AC.N_GPU):
    return np.sqrt(np.asarray(p) / n)   # of p itself, (1 - p) ~ 1


def _disc_dblquad(src, mu, centre, normal, radius):
    """The probability of crossing within `radius` of `centre`, integrated in Cartesian
    coordinates (x, y) of the plane."""
    n, u, v = AR._plane_frame(normal)
    rel = np.asarray(centre) - np.asarray(src)
    h, cu, cv = float(rel @ n), float(rel @ u), float(rel @ v)

    def f(y, x):
        s2 = (cu + x) ** 2 + (cv + y) ** 2 + h * h
        return h * math.exp(-mu * math.sqrt(s2)) / (4.0 * math.pi * s2 ** 1.5)

    val, _ = integrate.dblquad(f, -radius, radius, lambda x: -math.sqrt(max(0.0, radius * radius - x * x)),
                               lambda x: math.sqrt(max(0.0, radius * radius - x * x)), epsabs=1e-13, epsrel=1e-11)
    return val


@pytest.mark.parametrize("which", ["circle", "annulus"])
def test_disc_bins_against_dblquad(which):
    if which == "circle":
        centre, edges = AC.DA_CENTRE, AR.circle_edges(AC.DA_RADIUS, AC.DA_NBINS)
    else:
        centre, edges = AC.DA_ANN_CENTRE, AR.annulus_edges(*AC.DA_ANN)
    p = AR.point_source_disc_bins(AC.A_SRC, AC.A_MU, centre, AC.DA_NORMAL, edges)
    cum = np.array([0.0 if e == 0.0 else _disc_dblquad(AC.A_SRC, AC.A_MU, centre, AC.DA_NORMAL, e) for e in edges])
    ratio = np.abs(np.diff(cum) - p) / _se(p)
    print(which, "largest |difference| / standard error", ratio.max())
    assert ratio.max() < REF_SHARE and np.all(p > 0.0)
    finer = AR.point_source_disc_bins(AC.A_SRC, AC.A_MU, centre, AC.DA_NORMAL, edges, order=48, panels=24)
    assert (np.abs(finer - p) / _se(p)).max() < REF_SHARE


def test_disc_bins_on_the_axis_and_behind():
    """A source on the disc's axis: the 1-D integral over r; a plane behind the source: zeros."""
    c = tuple(s + 0.35 * n for s, n in zip(AC.A_SRC, AC.DA_NORMAL))
    edges = AR.circle_edges(0.3, 5)
    p = AR.point_source_disc_bins(AC.A_SRC, AC.A_MU, c, AC.DA_NORMAL, edges)
    for i in range(len(p)):
        want, _ = integrate.quad(lambda r: 0.5 * r * 0.35 * math.exp(-AC.A_MU * math.hypot(r, 0.35)) / math.hypot(r, 0.35) ** 3,
                                 edges[i], edges[i + 1], epsabs=1e-15, epsrel=1e-13)
        assert p[i] == pytest.approx(want, rel=1e-11)
    assert not AR.point_source_disc_bins(AC.A_SRC, AC.A_MU, c, tuple(-n for n in AC.DA_NORMAL), edges).any()
    assert list(AR.circle_edges(0.3, 0)) == [0.0, 0.3] and len(AR.annulus_edges(0.1, 0.28, 9)) == 11


def test_rect_against_dblquad():
    p, xy = AR.point_source_rect(AC.A_SRC, 0.0, AC.DA_CAM_P1, AC.DA_CAM_E1, AC.DA_CAM_E2)
    pw, _ = AR.point_source_rect(AC.A_SRC, AC.A_MU, AC.DA_CAM_P1, AC.DA_CAM_E1, AC.DA_CAM_E2)
    p1, e1, e2, src = (np.array(a) for a in (AC.DA_CAM_P1, AC.DA_CAM_E1, AC.DA_CAM_E2, AC.A_SRC))
    nrm = np.cross(e2, e1)
    area = float(np.linalg.norm(nrm))
    h = abs(float((p1 - src) @ nrm)) / area
    for mu, got in ((0.0, p), (AC.A_MU, pw)):
        def f(b, a):
            s = float(np.linalg.norm(p1 + a * e1 + b * e2 - src))
            return area * h * math.exp(-mu * s) / (4.0 * math.pi * s ** 3)
        want, _ = integrate.dblquad(f, 0.0, 1.0, 0.0, 1.0, epsabs=1e-13, epsrel=1e-11)
        print("camera mu", mu, got, want, abs(got - want) / _se(got))
        assert abs(got - want) / _se(got) < REF_SHARE
    assert 0.3 * p < pw < 0.7 * p   # (the window, had the camera one, would halve its count)
    # the pixel comes from the source: x = src.z + p1.x = 0.15 -> int(0.15 / 0.11) + 1 = 2,
    # y = src.y + p1.y = -0.2 -> int(-1.8) + 1 = 0, below 1 -> nbins + 1 = 5
    assert xy == pytest.approx((0.15, -0.2)) and AR.camera_pixel(xy, AC.DA_CAM_NBINS, AC.DA_CAM_MAXVAL) == 1 + 5 * 4


def test_fibre_against_enumeration():
    """The 4f chain, step by step as check_hit_fibre takes it, on 200001 radii across the front
    aperture: the accepted radii are one interval from 0, its end and every change of bin agree with
    fibre_bins' edges to the grid's step, and the ring integrals between the enumerated edges agree
    with its probabilities."""
    f, h = AC._fibre_f(), AC.DA_FIBRE_H
    p, r_max, a, edges = AR.fibre_bins(AC.A_SRC, AC.A_MU, AC._fibre_front(), AC.DA_FIBRE_AXIS, f, AC.DA_FIBRE_NBINS)
    rs = np.linspace(0.0, f[2], 200001)
    step = rs[1]
    nb = AC.DA_FIBRE_NBINS + 1
    w = f[10] / 2.0 / AC.DA_FIBRE_NBINS
    ok, bins = np.zeros(len(rs), dtype=bool), np.zeros(len(rs), dtype=np.int64)
    for i, r in enumerate(rs):
        ok[i], rad = AR.fibre_chain(float(r), h, f)
        bins[i] = min(int(math.floor(rad / w + 0.5)) + 1, nb) - 1
    last = int(np.flatnonzero(ok)[-1])
    assert ok[:last + 1].all() and not ok[last + 1:].any()
    assert abs(rs[last] - r_max) <= step and r_max < f[2]
    assert np.all(np.diff(bins[:last + 1]) >= 0) and bins[0] == 0 and bins[last] == nb - 1
    change = np.flatnonzero(np.diff(bins[:last + 1]))
    mine = np.concatenate([[0.0], 0.5 * (rs[change] + rs[change + 1]), [0.5 * (rs[last] + rs[last + 1])]])
    assert np.abs(mine - edges).max() <= step
    want = [integrate.quad(lambda r: 0.5 * r * h * math.exp(-AC.A_MU * math.hypot(r, h)) / math.hypot(r, h) ** 3, lo, hi,
                           epsabs=1e-16, epsrel=1e-13)[0] for lo, hi in zip(mine, mine[1:])]
    ratio = np.abs(np.array(want) - p) / _se(p)
    print("fibre r_max", r_max, "a", a, "largest |difference| / standard error", ratio.max())
    assert ratio.max() < REF_SHARE
    # the limits, one at a time: here the acceptance angle binds; abs() at the pinhole would
    g1 = 1.0 / h - 1.0 / f[0]
    assert r_max == pytest.approx(math.tan(math.radians(f[9])) / abs(g1 - (1.0 + g1 * (f[6] + f[7])) / f[1]))
    _, r_abs, _, _ = AR.fibre_bins(AC.A_SRC, AC.A_MU, AC._fibre_front(), AC.DA_FIBRE_AXIS, f, AC.DA_FIBRE_NBINS, abs_at_pinhole=True)
    assert r_abs == pytest.approx(f[8] / abs(1.0 + g1 * f[6])) and r_abs < 0.5 * r_max


def test_beam_legs_match_beam_slab():
    """beam_slab_legs walks the legs beam_slab walks: the absorption of the legs inside the slab,
    q (1 - exp(-mu L)), sums to beam_slab's absorbed fraction."""
    legs = AR.beam_slab_legs(*AC.faces(), AC.B_ORIGIN, AC.B_DIR, AC.Z_HALF, AC.B_N_IN, mu_in=AC.B_MU)
    _, p = AC.reference_b("sdf")
    absorbed = sum(q * -math.expm1(-AC.B_MU * length) for _, _, q, length, inside in legs if inside)
    assert absorbed == pytest.approx(p.sum(), rel=1e-12) and len(legs) >= 8
    assert legs[0][2] == 1.0 and not legs[0][4]


@pytest.mark.parametrize("form", AC.FORMS)
def test_beam_landings(form):
    """D-B by the reference alone: every detector has its landings in different bins, all inside
    the grid (expected_b asserts it), and at the GPU tests' count the bins below MIN_EVENTS hold at
    most B_POOL_CAP of a detector's expectation."""
    ps, lands = AC.expected_b(form)
    for p, landed in zip(ps, lands):
        assert len({b for b, _, _, _ in landed}) == len(landed) >= 1
        small = p[(p > 0.0) & (AC.N_GPU * p < AC.MIN_EVENTS)]
        assert small.sum() / p.sum() <= AC.B_POOL_CAP and AC.N_GPU * p.max() >= AC.MIN_EVENTS
    assert sum(len(landed) for landed in lands) >= 7
    # the fourth detector: a leg that leaves the grid before it reaches the plane scores nothing
    assert len(lands[3]) == 1 and len(lands[2]) == 2


# ----------------------------------------------- (b) the restatements against the reference ----
@pytest.mark.parametrize("form", AC.FORMS)
def test_restatement_point_source_detectors(form):
    """D-A at 3e6 photons (SDF form: 1.6e7): circle, camera, annulus, fibre and the flipped circle."""
    bins, ctr = cpu_run("a", form)
    st = AC.evaluate_det(bins, AC.expected_a(), n_cpu("a", form), ctr["detector_hits"])
    print(st)
    AC.check_det(st)
    assert not bins[4].any() and ctr["photons"] == n_cpu("a", form)


@pytest.mark.parametrize("form", AC.FORMS)
def test_restatement_beam_detectors(form):
    """D-B at 1e6 photons (the pooled share is judged at the GPU's count, test_beam_landings)."""
    bins, ctr = cpu_run("b", form)
    st = AC.evaluate_det(bins, AC.expected_b(form)[0], N_CPU["b"], ctr["detector_hits"])
    print(st)
    AC.check_det(st)


@pytest.mark.parametrize("survival", [False, True], ids=["analogue", "survival-bias"])
@pytest.mark.parametrize("form", AC.FORMS)
def test_restatement_identity(form, survival):
    """D-C at 2e5 photons."""
    bins, ctr = cpu_run("c", form, flags=PL | (abi.FLAG_SURVIVAL_BIAS if survival else 0))
    print(bins, ctr["detector_hits"])
    AC.check_identity([b.sum() for b in bins], ctr, survival)
    assert all(len(b) == 1 for b in bins)


def test_restatement_origins():
    """D-O at 1e6 photons per origin."""
    st = AC.evaluate_origins(cpu_origins(), AC.expected_o(), N_CPU["o"])
    print(st)
    AC.check_origins(st)


def test_restatement_escape_cells():
    from oracle import escape_oracle as EO
    cfg, _, _ = AC.escape_case()
    S = EO.Sym(*AC.ESCAPE_GRID, (0.0, 0.0, 1.0), 0.0)
    es, _, _ = EO.escape_function(AC.scene_a("sdf")[0], AC.grid(), AC.dets_o(), S, N_CPU["escape"], seed=AC.SEED)
    AC.check_escape(es, N_CPU["escape"])


# ------------------------------------------------------------------ (c) negative controls ----
# A reference that misreads one rule must fail the assertions the right one passes, on the runs of
# (b). Beside each: the smallest photon count of the ladder 1e4, 3e4, 1e5, 3e5, 1e6, 3e6,
# 8e6, 1.6e7 (SDF restatement, the first N photons of the seed) at which check_det first fails and fails on every
# rung above (`python -m tests.test_detectors_analytic_cpu ladder`); the right reference passes
# on every rung.
A_CONTROLS = {
    "floor": 10_000,                # int(r / w) instead of nint: every edge half a bin out
    "no-clamp": 10_000,             # the last half bin is lost: counts where none are expected
    "no-window": 10_000,            # exp(-mu s) dropped: no `t <= pointSep`
    "annulus-shifted": 10_000,      # r1 <= r < r2 one bin further in
    "centre+0.1w": 8_000_000,       # the centre moved by a tenth of a bin width
    "normal-swapped": 10_000,       # two components of the normal exchanged
    "orientation-ignored": 10_000,  # the flipped circle counts as the first does
    "fibre-abs-pinhole": 10_000,    # abs() at the pinhole test
    "mu+1%": 8_000_000,             # mu off by 1 %: exp(-mu s) with s about 0.4
}
B_CONTROLS = {
    "mu+1%": 300_000,               # on D-B: what leaves the slab below carries exp(-mu L), L = 1.03
    "orientation-ignored": 10_000,  # the incoming beam crosses the upper detectors against their normal
}
LADDER = (10_000, 30_000, 100_000, 300_000, 1_000_000, 3_000_000, 8_000_000, 16_000_000)


@pytest.mark.parametrize("control", list(A_CONTROLS))
def test_control_point_source_detectors(control):
    bins, ctr = cpu_run("a", "sdf")
    AC.check_det(AC.evaluate_det(bins, AC.expected_a(), N_CPU_A_SDF, ctr["detector_hits"]))
    with pytest.raises(AssertionError):
        AC.check_det(AC.evaluate_det(bins, AC.expected_a(control), N_CPU_A_SDF, ctr["detector_hits"]))


@pytest.mark.parametrize("control", list(B_CONTROLS))
def test_control_beam_detectors(control):
    bins, ctr = cpu_run("b", "sdf")
    AC.check_det(AC.evaluate_det(bins, AC.expected_b("sdf")[0], N_CPU["b"], ctr["detector_hits"]))
    with pytest.raises(AssertionError), np.errstate(divide="ignore"):  # (orientation ignored: a bin with p = 1)
        AC.check_det(AC.evaluate_det(bins, AC.expected_b("sdf", control)[0], N_CPU["b"], ctr["detector_hits"]))


def test_control_origins_transposed():
    """totals[k, d] read with the [detector][origin] stride: first fails at 3e4 per origin, the lowest
    count at which every live total expects MIN_EVENTS (ladder 1e4, 3e4, 1e5, 3e5)."""
    tot = cpu_origins()
    AC.check_origins(AC.evaluate_origins(tot, AC.expected_o(), N_CPU["o"]))
    wrong = np.ascontiguousarray(tot.T).reshape(tot.shape)
    with pytest.raises(AssertionError):
        AC.check_origins(AC.evaluate_origins(wrong, AC.expected_o(), N_CPU["o"]))


# ------------------------------------------------------------------------ predictions ----
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _ladder():
    for which, controls, top in (("a", A_CONTROLS, N_CPU_A_SDF), ("b", B_CONTROLS, 1_000_000)):
        rungs = [n for n in LADDER if n <= top]
        runs = {n: cpu_run(which, "sdf", n) for n in rungs}
        exp = (lambda c: AC.expected_a(c)) if which == "a" else (lambda c: AC.expected_b("sdf", c)[0])
        for c in [None] + list(controls):
            fails = [_fails(lambda: AC.check_det(AC.evaluate_det(runs[n][0], exp(c), n, runs[n][1]["detector_hits"]))) for n in rungs]
            print(which, c, dict(zip(rungs, fails)))
    for n in LADDER[:4]:
        tot = cpu_origins(n)
        right = _fails(lambda: AC.check_origins(AC.evaluate_origins(tot, AC.expected_o(), n)))
        wrong = _fails(lambda: AC.check_origins(AC.evaluate_origins(np.ascontiguousarray(tot.T).reshape(tot.shape), AC.expected_o(), n)))
        print("origins", n, "right fails", right, "transposed fails", wrong)


def _predict(which):
    n = AC.N_GPU
    if which in ("a", "b"):
        for form in AC.FORMS:
            bins, ctr = cpu_run(which, form, n)
            exp = AC.expected_a() if which == "a" else AC.expected_b(form)[0]
            st = AC.evaluate_det(bins, exp, n, ctr["detector_hits"])
            AC.check_det(st, AC.B_POOL_CAP if which == "b" else None)
            print((which, form), {**AC.flat_det(st), "digest": AC.digest(bins)}, flush=True)
    elif which == "c":
        for form in AC.FORMS:
            for survival in (False, True):
                bins, ctr = cpu_run("c", form, AC.N_GPU_C, PL | (abi.FLAG_SURVIVAL_BIAS if survival else 0))
                AC.check_identity([b.sum() for b in bins], ctr, survival)
                print(("c", form, survival), {"bins": [float(b.sum()) for b in bins], "hits": ctr["detector_hits"]}, flush=True)
    elif which == "o":
        tot = cpu_origins(AC.N_GPU_O)
        st = AC.evaluate_origins(tot, AC.expected_o(), AC.N_GPU_O)
        AC.check_origins(st)
        print("origins", tot.tolist(), st["max_z"], flush=True)
        from oracle import escape_oracle as EO
        S = EO.Sym(*AC.ESCAPE_GRID, (0.0, 0.0, 1.0), 0.0)
        es, _, _ = EO.escape_function(AC.scene_a("sdf")[0], AC.grid(), AC.dets_o(), S, AC.N_GPU_E, seed=AC.SEED)
        st = AC.check_escape(es, AC.N_GPU_E)
        print("escape", [[float(es[d, i, j, k]) for d in range(3)] for i, j, k in AC.escape_case()[1]], st["max_z"], flush=True)


if __name__ == "__main__":
    np.set_printoptions(linewidth=200)
    if sys.argv[1] == "ladder":
        _ladder()
    else:
        for w in sys.argv[2:]:
            _predict(w)
