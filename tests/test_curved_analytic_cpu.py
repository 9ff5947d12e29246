"""Curved surfaces against closed forms, without a GPU (DESIGN.md §3.5 "Curved surfaces"): a glass
sphere in vacuum on analytic_cases.grid() (8 x 12 x 10, three unequal edges; the conditions hold on
it, so scene D needs no grid of its own). (a) tests/analytic_ref.py's tracer, casts and
centre-source solution against each other and against the geometric series, (b) the conditions on
the inputs, (c) the CPU restatements (oracle/ for the SDF forms, tests/mesh_ref.c for the
polyhedron) against them with the assertions tests/test_gpu_curved_analytic.py makes of the HIP
path, and (d) negative controls: the same assertions must reject a reference that is slightly
wrong. There is no voxel form: a label volume has no curved surface.

`python -m tests.test_curved_analytic_cpu predict [case ...]` prints the statistics of the
GPU-sized runs (PREDICTED in the GPU file); a case is centre-sdf, beam-mesh, tir-sdf-survival, det, ...,
with @N for another count per batch than 840,000.
"""
import math
import sys

import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, builders
from tests import analytic_cases as AC
from tests import analytic_ref as AR
from tests import mesh_ref as M

PL = abi.FLAG_PATHLENGTH
RUN = {"sdf": O.run, "table": O.run, "mesh": M.run}
# (the table form differs from the SDF form by tops that no photon meets: one case of it here, all
# three in the GPU-sized predictions)
CASES = [("centre", "sdf"), ("beam", "sdf"), ("beam", "table"), ("beam", "mesh"), ("tir", "sdf"), ("tir", "mesh")]
# photons per batch (x 24), the counts of tests/test_analytic_cpu.py: D-centre as A, the beams as B
N_BATCH = {"centre": 300_000, "beam": 80_000, "tir": 80_000}
N_DET = 1_000_000
_RUNS = {}


def cpu_run(case, form, n_batch=None, flags=PL):
    """(jmean per batch, absorb per batch, counters) of the restatement of `form`, run once."""
    n_batch = N_BATCH[case] if n_batch is None else n_batch
    key = (case, form, n_batch, flags)
    if key not in _RUNS:
        sc, src = AC.scene_d(case, form)
        g = AC.grid()
        _RUNS[key] = AC.run_batches(
            lambda first, n: RUN[form](sc, g, src, n, seed=AC.SEED, first_photon=first, flags=flags), n_batch)
    return _RUNS[key]


def cpu_det(form, n=N_DET):
    key = ("det", form, n)
    if key not in _RUNS:
        sc, src = AC.scene_d("beam", form)
        dets = AC.dets_d(form)
        r = RUN[form](sc, AC.grid(), src, n, seed=AC.SEED, flags=PL, dets=dets)
        _RUNS[key] = ([r.detector(i).copy() for i in range(len(dets))], r.counters_dict())
    return _RUNS[key]


def evaluate(case, form, jm, ab, ctr, n_batch, control=None):
    """evaluate_ab of a scene D run: D-centre in reduce_centre's layout (the cut voxels one pooled
    sum) without slop, as A; the beams per voxel with the derived slop."""
    if case == "centre":
        return AC.evaluate_ab("d", AC.reduce_centre(jm, control if control and control.endswith("-swapped") else None),
                              AC.reduce_centre(ab, control if control and control.endswith("-swapped") else None),
                              ctr, n_batch, AC.reference_centre(control), slop=0.0)
    return AC.evaluate_ab("d", jm, ab, ctr, n_batch, AC.reference_d(case, form, control), slop=AC.d_track_slop(case, form))


def exact_tir(form, jm, ab, ctr):
    """D-tir's exact statements. On the sphere nothing leaves it: no escape, every photon absorbed,
    no track in a voxel wholly outside radius R + 1e-6. On the polyhedron the reference decides
    (some facets transmit): there the zeros hold where the reference has none, which check_ab
    asserts (absorb and jmean off the support)."""
    if form == "mesh":
        return
    assert ctr["escaped"] == 0 and ctr["absorbed"] == ctr["photons"], ctr
    _, outside = AR.ball_voxels(*AC.faces(), AC.D_CENTRE, AC.D_R + 1e-6)
    assert outside.sum() >= 300 and not jm.sum(axis=0)[outside].any() and not ab.sum(axis=0)[outside].any()


# ------------------------------------------------------------- (a) the references themselves ----
def _inside_sequence(legs, paths):
    """The interior legs on the path that only reflects after entering, in order."""
    seq = [(leg, path) for leg, path in zip(legs, paths) if leg[4]]
    return sorted(seq, key=lambda lp: len(lp[1]))


@pytest.mark.parametrize("case", ["beam", "tir"])
def test_tracer_reproduces_the_geometric_series(case):
    """Every interior chord is 2 R cos(theta_t), every hit has one reflectance, interior leg k
    carries (1 - rho) rho^k exp(-mu k c) (from inside: exp(-mu s0) rho^k a^(k-1)), and the absorbed
    and escaped fractions are geometric series: to 1e-12."""
    tr, pa, legs, hits, paths = AC.trace_d(case)
    mu = AC.d_mu(case)
    if case == "beam":
        ser = AR.sphere_beam_series(AC.D_BEAM_B / AC.D_R, AC.D_R, AC.D_N, mu)
    else:
        ser = AR.sphere_beam_series(AC.D_TIR_SIN, AC.D_R, AC.D_N, mu, from_inside=True, first_run=legs[0][3])
        assert ser["rho"] == 1.0 and ser["escaped"] == 0.0 and AC.D_TIR_SIN > 1.0 / AC.D_N
        assert 0.45 < mu * ser["chord"] < 0.55 and 55 <= len(legs) <= 70
    inner = _inside_sequence(legs, paths)
    assert len(inner) >= 7
    for k, (leg, _) in enumerate(inner):
        if not (case == "tir" and k == 0):
            assert leg[3] == pytest.approx(ser["chord"], abs=1e-12)
        assert leg[2] == pytest.approx(ser["q"](k), rel=1e-12, abs=1e-26)
    for _, c1, _, inside, _ in hits:
        cos = math.sqrt(1.0 - (AC.D_BEAM_B / AC.D_R if case == "beam" else AC.D_TIR_SIN) ** 2)
        want = AR.fresnel_unpolarised(cos, 1.0, AC.D_N)[1] if inside and case == "beam" else cos
        assert c1 == pytest.approx(want, abs=1e-12)
    cut = sum(ser["q"](k) for k in range(len(inner), len(inner) + 3))  # what q_min leaves unfollowed
    assert pa.sum() == pytest.approx(ser["absorbed"], abs=1e-12 + cut)
    outer = sum(leg[2] * leg[3] for leg in legs if not leg[4])
    assert tr.sum() == pytest.approx(pa.sum() / mu + outer, rel=1e-12)
    assert np.all(pa[tr == 0.0] == 0.0)


def test_beam_legs_reproduces_beam_slab():
    """beam_slab is left as it is; the general tracer with a cast of the slab's two planes gives
    its grids on B's inputs (to rounding: the plane's hit point is not snapped onto the plane)."""
    zh = AC.Z_HALF

    def cast(o, d):
        best = None
        for zp in (-zh, zh):
            if d[2] != 0.0:
                s = (zp - o[2]) / d[2]
                if s > AR.CAST_EPS and (best is None or s < best[0]):
                    best = (s, np.array([0.0, 0.0, math.copysign(1.0, zp)]))
        return best

    t0, p0 = AC.reference_b()
    t1, p1, legs, _, _ = AR.beam_legs(*AC.faces(), AC.B_ORIGIN, AC.B_DIR, cast, AC.B_N_IN, 1.0, AC.B_MU, 1e-14)
    assert np.array_equal(t0 > 0.0, t1 > 0.0)
    assert np.abs(t1 - t0).max() < 1e-14 and np.abs(p1 - p0).max() < 1e-14
    assert len(legs) == len(AR.beam_slab_legs(*AC.faces(), AC.B_ORIGIN, AC.B_DIR, zh, AC.B_N_IN, mu_in=AC.B_MU))


def test_triangle_cast_approaches_the_sphere():
    """cast_triangles on finer icospheres approaches cast_sphere: the first three legs of D-beam
    (in, first interior leg, first exit) start and point within the facets' tilt of the sphere's."""
    o, d = np.array(AC.d_origin("beam")), np.array(AC.D_BEAM_DIR)

    def first_three(cast):
        _, _, legs, _, paths = AR.beam_legs(*AC.faces(), o, d, cast, AC.D_N, 1.0, AC.D_MU, 1e-3)
        pick = [next(lg for lg, p in zip(legs, paths) if len(p) == m and lg[4] == inside)
                for m, inside in ((0, False), (1, True), (2, False))]
        return np.array([np.concatenate([lg[0], lg[1]]) for lg in pick])

    want = first_three(AR.cast_sphere(AC.D_CENTRE, AC.D_R))
    err = {lv: float(np.abs(first_three(AR.cast_triangles(*builders.icosphere(lv, AC.D_R, AC.D_CENTRE))) - want).max())
           for lv in (2, 3, 5)}
    print(err)
    # a facet of level L spans 1.1 / 2^L rad; its normal is off the radial one by up to half of that
    assert err[5] < 0.6 / 2 ** 5 * 2.0 and err[5] < err[3] < 0.6 / 2 ** 3 * 2.0 and err[2] < 0.6 / 2 ** 2 * 2.0


def test_centre_source_closes_and_matches_direct_quadrature():
    """The three pyramid sums (mu, -mu, 0) against tensor Gauss-Legendre integrals over the voxels,
    the pooled expectation against a brute-force quadrature of g(r) / (4 pi r^2) over the cut voxels
    (subdivided: the integrand jumps on the surface, so that one is rough), and the totals."""
    c = AC.centre_d()
    xe, ye, ze = AC.faces()
    for mu in (AC.D_MU, -AC.D_MU, 0.0):
        t = AR.point_source_track(xe, ye, ze, AC.D_CENTRE, mu)
        direct = AR.point_source_track_direct(xe, ye, ze, AC.D_CENTRE, mu)
        assert np.nanmax(np.abs(direct / t - 1.0)) < 1e-10 and np.isnan(direct).sum() == 1
    assert float(AR.point_source_track(xe, ye, ze, AC.D_CENTRE, 0.0).sum()) > AC.D_R
    r0, mu, rad = c["r0"], AC.D_MU, AC.D_R
    assert r0 == pytest.approx(0.04) and c["p_escape"] == pytest.approx(0.96 * math.exp(-1.1) / (1.0 - 0.04 * math.exp(-2.2)), rel=1e-14)
    assert c["cut_track"] > 0.0 and c["cut_p_abs"] > 0.0
    # the interior track of the uncut voxels plus the cut ones' absorptions / mu is the whole interior track
    assert float(c["p_abs"][c["inside"]].sum()) + c["cut_p_abs"] == pytest.approx(1.0 - c["p_escape"], rel=1e-14)
    # midpoint quadrature over the cut voxels, 24^3 cells each
    dd = 1.0 - r0 * math.exp(-2.0 * mu * rad)
    m = (np.arange(24) + 0.5) / 24.0
    tot_t, tot_p = 0.0, 0.0
    for k, j, i in np.argwhere(c["cut"]):
        x = xe[i] + (xe[i + 1] - xe[i]) * m - AC.D_CENTRE[0]
        y = ye[j] + (ye[j + 1] - ye[j]) * m - AC.D_CENTRE[1]
        z = ze[k] + (ze[k + 1] - ze[k]) * m - AC.D_CENTRE[2]
        r = np.sqrt(z[:, None, None] ** 2 + y[None, :, None] ** 2 + x[None, None, :] ** 2)
        g_in = (np.exp(-mu * r) + r0 * np.exp(-mu * (2.0 * rad - r))) / dd
        w = (xe[i + 1] - xe[i]) * (ye[j + 1] - ye[j]) * (ze[k + 1] - ze[k]) / 24 ** 3
        dens = np.where(r < rad, g_in, c["p_escape"]) / (4.0 * math.pi * r * r)
        tot_t += float(dens.sum()) * w
        tot_p += float((mu * dens)[r < rad].sum()) * w
    print(tot_t, c["cut_track"], tot_p, c["cut_p_abs"])
    assert tot_t == pytest.approx(c["cut_track"], rel=2e-3) and tot_p == pytest.approx(c["cut_p_abs"], rel=2e-3)


# ------------------------------------------------------------------------ (b) conditions ----
def test_conditions():
    """Barycentric margins, hits off the voxel walls, D-centre's voxel counts and events, the pooled
    shares, the derived slop and its share of a voxel's track, the extra spheres' clearance."""
    fig = AC.d_conditions()
    for k, v in fig.items():
        print(k, v)
    for form in ("sdf", "mesh"):
        ps, lands = AC.expected_d(form)
        print(form, [p.sum() for p in ps])
        assert all(p.sum() * N_DET >= AC.MIN_EVENTS for p in ps)
    assert fig["tir", "sdf"]["p_abs"] > 1.0 - 1e-13 and fig["tir", "mesh"]["p_abs"] < 1.0 - 1e-4
    assert fig["tir", "sdf"]["min_cos"] < math.sqrt(1.0 - 1.0 / AC.D_N ** 2)


def test_table_form_takes_the_cooperative_eval():
    from tests import planprobe
    for case in ("centre", "beam", "tir"):
        sc, _ = AC.scene_d(case, "table")
        plan = planprobe.plan(sc, AC.grid())
        assert plan["status"] == abi.OK, plan["error"]
        assert plan["coop_lanes"] > 0 and plan["ctab"] == 1 and plan["lean_candidate"] == 0, plan
        plan = planprobe.plan(AC.scene_d(case, "sdf")[0], AC.grid())
        assert plan["coop_lanes"] == 0 and plan["lean_candidate"] == 1, plan


# ----------------------------------------------- (c) the restatements against the reference ----
@pytest.mark.parametrize("case,form", CASES, ids=[f"{c}-{f}" for c, f in CASES])
def test_restatement(case, form):
    jm, ab, ctr = cpu_run(case, form)
    st = evaluate(case, form, jm, ab, ctr, N_BATCH[case])
    print(st)
    AC.check_ab(st)
    if case == "tir":
        exact_tir(form, jm, ab, ctr)
    assert ctr["fresnel"] > 0 and ctr["reflections"] > 0 and ctr["scatters"] == 0, ctr


@pytest.mark.parametrize("form", ["sdf", "mesh"])
def test_restatement_survival_bias(form):
    """D-tir with FLAG_SURVIVAL_BIAS: absorb and jmean by batch means."""
    jm, ab, ctr = cpu_run("tir", form, flags=PL | abi.FLAG_SURVIVAL_BIAS)
    st = AC.evaluate_weighted(jm, ab, ctr, N_BATCH["tir"], AC.reference_d("tir", form), AC.d_track_slop("tir", form))
    print(st)
    AC.check_weighted(st)


@pytest.mark.parametrize("form", ["sdf", "table", "mesh"])
def test_restatement_detectors(form):
    """D-beam's two circles: Binomial in the landing bin, every other bin exactly 0."""
    bins, ctr = cpu_det(form)
    st = AC.evaluate_det(bins, AC.expected_d(form)[0], N_DET, ctr["detector_hits"])
    print(st)
    AC.check_det(st, AC.B_POOL_CAP)
    assert all(np.count_nonzero(b) == 1 and b[AC.D_DET_BIN] > 0 for b in bins)


# ------------------------------------------------------------------ (d) negative controls ----
# Each control names the cases whose assertions must reject it on the runs of (c). What each case
# cannot see: D-centre meets the surface at normal incidence, where both polarisations reflect
# alike, a normal's sign or a refraction about the unturned normal changes nothing, and n + 1 %
# moves r0 by 3 % of 0.04 (0.2 % of a voxel's track: below these runs' resolution); its reference
# under a tilted normal has no closed form. D-tir on the sphere transmits nothing, so the exit
# normal never acts, and total reflection knows no polarisation; n + 1 % leaves it total.
CONTROL_CASES = {
    "n+1%": ("beam",),
    "R+1%": ("centre", "beam", "tir"),
    "mu+1%": ("centre", "beam", "tir"),
    "s-polarised": ("beam",),
    "normal-tilted": ("beam", "tir"),
    "exit-normal-unturned": ("beam",),
    "x-y-swapped": ("centre", "beam", "tir"),
    "x-z-swapped": ("centre", "beam", "tir"),
    "y-z-swapped": ("centre", "beam", "tir"),
}
CONTROLS = [(c, case) for c in AC.D_CONTROLS for case in CONTROL_CASES[c]]


@pytest.mark.parametrize("control,case", CONTROLS, ids=[f"{c}-{k}" for c, k in CONTROLS])
def test_control(control, case):
    jm, ab, ctr = cpu_run(case, "sdf")
    AC.check_ab(evaluate(case, "sdf", jm, ab, ctr, N_BATCH[case]))
    with pytest.raises(AssertionError), np.errstate(divide="ignore", invalid="ignore"):
        AC.check_ab(evaluate(case, "sdf", jm, ab, ctr, N_BATCH[case], control))


@pytest.mark.parametrize("control", [c for c in AC.D_CONTROLS if not c.endswith("-swapped") and c != "mu+1%"])
def test_control_detectors(control):
    """The two circles see a direction error: every control that moves the doubly refracted or the
    reflected leg by more than half a bin, or changes its share, is rejected by check_det."""
    bins, ctr = cpu_det("sdf")
    AC.check_det(AC.evaluate_det(bins, AC.expected_d("sdf")[0], N_DET, ctr["detector_hits"]))
    with pytest.raises(AssertionError), np.errstate(divide="ignore", invalid="ignore"):
        AC.check_det(AC.evaluate_det(bins, AC.expected_d("sdf", control)[0], N_DET, ctr["detector_hits"]))


# ------------------------------------------------------------------------ predictions ----
def flat(st):
    """The figures of evaluate_ab that PREDICTED records."""
    return {"max_z": st["counts"]["max_z"], "chi2": st["counts"]["chi2"], "z_absorbed": st["z_absorbed"],
            "max_t": st["tracks"]["max_t"], "mean_t2": st["tracks"]["mean_t2"], "score": st["tracks"]["score"],
            "t_sum": st["tracks"]["t_sum"]}


def flat_weighted(st):
    c, t = st["counts"], st["tracks"]
    return {"ab_max_t": c["max_t"], "ab_mean_t2": c["mean_t2"], "ab_t_sum": c["t_sum"], "absorb_sum": st["absorb_sum"],
            "max_t": t["max_t"], "mean_t2": t["mean_t2"], "score": t["score"], "t_sum": t["t_sum"]}


def _predict(what):
    what, _, count = what.partition("@")     # "tir-sdf-survival@210000": photons per batch
    n_batch = int(count) if count else 840_000
    if what == "det":
        for form in ("sdf", "mesh"):
            bins, ctr = cpu_det(form, AC.N_GPU)
            st = AC.evaluate_det(bins, AC.expected_d(form)[0], AC.N_GPU, ctr["detector_hits"])
            AC.check_det(st, AC.B_POOL_CAP)
            print(("det", form), {**AC.flat_det(st), "digest": AC.digest(bins)}, flush=True)
        return
    case, form = what.split("-")[:2]
    survival = what.endswith("-survival")
    flags = PL | (abi.FLAG_SURVIVAL_BIAS if survival else 0)
    jm, ab, ctr = cpu_run(case, form, n_batch, flags)
    if survival:
        st = AC.evaluate_weighted(jm, ab, ctr, n_batch, AC.reference_d(case, form), AC.d_track_slop(case, form))
        print(st, flush=True)
        AC.check_weighted(st)
        print((case, form, True), flat_weighted(st), flush=True)
        return
    st = evaluate(case, form, jm, ab, ctr, n_batch)
    print(st, flush=True)
    AC.check_ab(st)
    if case == "tir":
        exact_tir(form, jm, ab, ctr)
    print((case, form), flat(st), flush=True)


if __name__ == "__main__":
    np.set_printoptions(linewidth=200)
    for w in sys.argv[2:]:
        _predict(w)
