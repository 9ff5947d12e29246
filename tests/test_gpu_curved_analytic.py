"""The HIP path on curved surfaces against closed forms that need neither the restatements nor the
reference (DESIGN.md §3.5 "Curved surfaces"): a glass sphere (n = 1.5, absorbing, not scattering)
in vacuum on analytic_cases.grid(), 8 x 12 x 10 with three unequal edges,

  D-centre  a point source at the sphere's centre: the radial law g(r) / (4 pi r^2) inside and
            outside, normal-incidence Fresnel, the inside-to-outside choice of the top whose
            normal is taken; a normal off the radius by an amount that varies over the sphere
            breaks the law outside (a tilt of all normals about one axis only turns the isotropic
            field about its centre: that one is D-beam's and D-tir's to catch),
  D-beam    an oblique pencil from outside: Snell and Fresnel about a tilted normal, both
            crossing branches, interior bounces; two circles across its doubly refracted and its
            reflected leg, whose one landing ring moves with a direction error of 1e-3 rad,
  D-tir     a pencil from inside beyond the critical angle: a star polygon of total reflections,
            no escape, no track outside the sphere, exactly,

through ws_kernel, transport_kernel, the cooperative EVAL with its table (nine more tops outside
the grid) and mesh_kernel (an icosphere, against the same polyhedron cast in numpy). There is no
voxel form: a label volume has no curved surface. The expectations are tests/analytic_ref.py
(beam_legs, cast_sphere, cast_triangles, centre_source_sphere), the scenes, conditions, slop and
statistics tests/analytic_cases.py; tests/test_curved_analytic_cpu.py checks the references against
each other, shows that the assertions reject a reference with n, R or mu off by 1 %, one
polarisation, a normal tilted by 5 mrad, an unturned exit normal or two axes swapped, and runs
them on the CPU restatements.

Statistics as in tests/test_gpu_analytic.py (24 batches of one seed, a family-wise false-alarm rate
of 1e-3 per test). The seeds are fixed and the integer tallies equal the restatements' bit for bit,
so each statistic is known beforehand from a CPU run of the same photons: PREDICTED.
"""
import numpy as np
import pytest

from rsmcrt_amd import abi
from rsmcrt_amd.engine import Engine
from tests import analytic_cases as AC
from tests import analytic_ref as AR
from tests import planprobe

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH

# path -> (scene form, environment, ws_kernel runs)
PATHS = {
    "ws": ("sdf", {}, True),
    "transport": ("sdf", {"SMCRT_LEAN": "0"}, False),
    "table": ("table", {}, False),
    "mesh": ("mesh", {}, False),
}

# Photons per batch (x 24): the 2e7 photons aimed at, on every path but one. Beside each: the time
# of the test's call seen on one MI355X in a run of this file, which takes 17 s for its 15 tests.
# The yardstick, the parent commit's test_gpu_analytic.py in the same session: 18 tests in 14.8 s,
# the slowest calls 3.04 s, 1.81 s, 1.81 s, 1.48 s; no call here may take more than 6.08 s.
# D-tir with survival bias on transport_kernel took 20.6 s at 840,000: the atomic fp64 deposit of
# 2e7 photons that all walk the same 39 voxels. It runs the count of the CPU suite's D-tir instead,
# 80,000, at which analytic_cases.d_conditions() still holds (the pooled shares stay below 2e-5).
N_BATCH = {
    ("centre", "ws"): 840_000,         # 0.44 s
    ("centre", "transport"): 840_000,  # 0.10 s
    ("centre", "table"): 840_000,      # 0.13 s
    ("beam", "ws"): 840_000,           # 0.91 s
    ("beam", "transport"): 840_000,    # 0.12 s
    ("beam", "table"): 840_000,        # 0.18 s
    ("beam", "mesh"): 840_000,         # 1.12 s
    ("tir", "ws"): 840_000,            # 1.11 s
    ("tir", "transport"): 840_000,     # 0.28 s
    ("tir", "table"): 840_000,         # 0.45 s
    ("tir", "mesh"): 840_000,          # 1.51 s
    ("tir", "transport", "survival"): 80_000,   # 3.41 s (20.6 s at 840,000)
    ("tir", "mesh", "survival"): 840_000,       # 2.97 s, 2.86 s
}
# the detector case, one launch: transport 1.22 s, mesh 0.09 s
N_DET = AC.N_GPU

# The statistics of the CPU restatements (oracle/ for the SDF forms, tests/mesh_ref.c) on the same
# photons, seed and batches, computed before the GPU ran them
# (`python -m tests.test_curved_analytic_cpu predict centre-sdf ... det`).
# The table form's tops are met by no photon: its tallies and statistics are the SDF form's.
# Bounds at these counts:
#   D-centre  max |z| 4.58, chi^2 in [11.8, 75.6] (34 voxels inside and the cut voxels' bin),
#             |z_absorbed| 3.59, max |t| 7.60, mean t^2 in [0.865, 1.325], score 974.8 (814 bins), |t_sum| 4.77
#   D-beam    max |z| 4.39 (mesh 4.45), chi^2 in [2.3, 44.8] (15 bins, 11 pooled voxels with 6e-6;
#             mesh [3.9, 51.3], 19 and 20 with 9e-6), max |t| 6.22, mean t^2 in [0.327, 2.693], score 75.6
#             (35 bins, 29 pooled voxels with 4e-6; mesh 6.31, [0.382, 2.510], 87.0, 43 and 45, 1e-5)
#   D-tir     max |z| 4.56 (mesh 4.59), chi^2 in [10.7, 72.6] (33 bins, 7 pooled voxels with 1e-5;
#             mesh [13.5, 79.9], 38 and 18), max |t| 6.25, mean t^2 in [0.350, 2.607], score 78.4
#             (37 bins, 3 pooled; mesh 6.45, [0.455, 2.236], 108.9, 59 and 39, 1e-6)
_CENTRE = {"max_z": 2.1240140737138864, "chi2": 26.559774139727203, "z_absorbed": -0.22526795290637283,
           "max_t": 3.3468691280316993, "mean_t2": 1.0489619584305143, "score": 781.7464518814056, "t_sum": 0.07953010586015362}
_BEAM = {"max_z": 2.2818041139929166, "chi2": 16.508222887376203, "z_absorbed": 2.2155233857881074,
         "max_t": 2.038680015158734, "mean_t2": 1.2261387221511637, "score": 39.79067498076967, "t_sum": -2.1074613720049835}
# (on the sphere every photon of D-tir is absorbed, which the test asserts outright: z_absorbed
# and the t of the absorb sum would only record the rounding of 1 - sum p = 9e-15)
_TIR = {"max_z": 2.6247066852469234, "chi2": 27.90478728672061,
        "max_t": 1.8504114834517111, "mean_t2": 1.5706676962040482, "score": 54.10873524201448, "t_sum": -1.7117413498049856}
PREDICTED = {
    ("centre", "sdf"): _CENTRE, ("centre", "table"): _CENTRE,
    ("beam", "sdf"): _BEAM, ("beam", "table"): _BEAM,
    ("beam", "mesh"): {"max_z": 1.5065179188597195, "chi2": 11.976570165025402, "z_absorbed": 1.9628814785186544,
                       "max_t": 2.0047200280680455, "mean_t2": 1.0336418343487148, "score": 41.17985153421315, "t_sum": -1.7071587635044323},
    ("tir", "sdf"): _TIR, ("tir", "table"): _TIR,
    ("tir", "mesh"): {"max_z": 1.8254366896711849, "chi2": 27.983222157514202, "z_absorbed": -0.21511397418699021,
                      "max_t": 1.8277086875112156, "mean_t2": 0.9873240369470305, "score": 54.2953965655486, "t_sum": -1.625457056513494},
    # at 24 x 80,000 photons (N_BATCH)
    ("tir", "sdf", True): {"ab_max_t": 2.319933879493988, "ab_mean_t2": 1.319034647628218,
                           "absorb_sum": 1920000.0, "max_t": 1.890711814732173, "mean_t2": 1.21192316808394,
                           "score": 36.385119187048524, "t_sum": 1.0834498115073778},
    ("tir", "mesh", True): {"ab_max_t": 1.8606085323505375, "ab_mean_t2": 0.6869838957721648, "ab_t_sum": -0.23887450149995296,
                            "absorb_sum": 20065671.0, "max_t": 1.8277086875112156, "mean_t2": 0.9873240369470305,
                            "score": 54.2953965655486, "t_sum": -1.625457056513494},
}
PREDICTED_DET = {
    ("det", "sdf"): {"hits": 3308509, "total0": 2431293.0, "max_z0": 1.9985954361266847, "chi20": 3.994383717306413,
                     "z_total0": -1.9985954361266847, "total1": 877216.0, "max_z1": 0.7408266855264761,
                     "chi21": 0.5488241779881443, "z_total1": -0.7408266855264761, "digest": (3308509.0, 25038554.0)},
    ("det", "mesh"): {"hits": 3352857, "total0": 2409228.0, "max_z0": 2.0713212075258425, "chi20": 4.290371544746314,
                      "z_total0": -2.0713212075258425, "total1": 943629.0, "max_z1": 0.27022423897877235,
                      "chi21": 0.07302113933165667, "z_total1": -0.27022423897877235, "digest": (3352857.0, 26521923.0)},
}


def n_batch_of(case, path, flags):
    key = (case, path, "survival") if flags & abi.FLAG_SURVIVAL_BIAS else (case, path)
    return N_BATCH[key]


def run_gpu(monkeypatch, case, path, flags=PL, dets=None):
    form, env, lean = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, src = AC.scene_d(case, form)
    if form == "table":
        plan = planprobe.plan(sc, AC.grid())
        assert plan["status"] == abi.OK and plan["coop_lanes"] > 0 and plan["ctab"] == 1, plan
    with Engine(sc, AC.grid(), *(() if dets is None else (dets,))) as eng:
        eng.kernel_times()
        if dets is None:
            n_batch = n_batch_of(case, path, flags)
            jm, ab, ctr = AC.run_batches(
                lambda first, n: eng.run(src, n, seed=AC.SEED, flags=flags, first_photon=first), n_batch)
            out = (jm, ab, ctr, n_batch)
        else:
            r = eng.run(src, N_DET, seed=AC.SEED, flags=flags)
            ctr = r.counters_dict()
            out = ([r.detector(i).copy() for i in range(len(dets))], ctr, N_DET)
        eng.check()
        kt = eng.kernel_times()
    if lean and dets is None and not flags & abi.FLAG_SURVIVAL_BIAS:
        assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, kt
    else:
        assert kt["lean_launches"] == 0, kt
    assert (ctr["sdf_evals"] > 0) == (form != "mesh"), ctr
    assert ctr["photons"] == (N_DET if dets is not None else n_batch_of(case, path, flags) * AC.BATCHES)
    assert ctr.get("faults", 0) == 0, ctr
    return out


def predicted(key, got, table=PREDICTED):
    """The statistics equal the restatement's: those of integer tallies to rounding, those of
    jmean (equal to 1e-12 per voxel; a t is a difference of 1e-3 of it over its error) to 1e-6."""
    want = table.get(key)
    print(key, got)
    assert want is not None, f"no prediction recorded for {key}"
    for k, v in want.items():
        if k == "digest":
            assert tuple(got[k]) == tuple(v), (k, got[k], v)
        else:
            assert got[k] == pytest.approx(v, rel=1e-6, abs=1e-6), (k, got[k], v)


def flat(st):
    """The figures of evaluate_ab that PREDICTED records."""
    return {"max_z": st["counts"]["max_z"], "chi2": st["counts"]["chi2"], "z_absorbed": st["z_absorbed"],
            "max_t": st["tracks"]["max_t"], "mean_t2": st["tracks"]["mean_t2"], "score": st["tracks"]["score"], "t_sum": st["tracks"]["t_sum"]}


def flat_weighted(st):
    c, t = st["counts"], st["tracks"]
    return {"ab_max_t": c["max_t"], "ab_mean_t2": c["mean_t2"], "ab_t_sum": c["t_sum"], "absorb_sum": st["absorb_sum"],
            "max_t": t["max_t"], "mean_t2": t["mean_t2"], "score": t["score"], "t_sum": t["t_sum"]}


@pytest.mark.parametrize("path", ["ws", "transport", "table"])
def test_point_source_at_the_centre(monkeypatch, path):
    """D-centre: r0 = ((n - 1) / (n + 1))^2, D = 1 - r0 exp(-2 mu R); a voxel wholly inside holds
    [T(mu) + r0 exp(-2 mu R) T(-mu)] / D of track and mu times that in absorptions, one wholly
    outside (1 - r0) exp(-mu R) / D * T(0) and no absorption, the 147 voxels the surface cuts one
    pooled sum that is exact by conservation. 34 + 779 + 1 bins, none below 100 events."""
    jm, ab, ctr, n_batch = run_gpu(monkeypatch, "centre", path)
    st = AC.evaluate_ab("d", AC.reduce_centre(jm), AC.reduce_centre(ab), ctr, n_batch, AC.reference_centre(), slop=0.0)
    print(st)
    AC.check_ab(st)
    assert st["counts"]["n_pooled"] == 0 and st["tracks"]["n_pooled"] == 0
    assert ctr["scatters"] == 0 and ctr["reflections"] > 0
    predicted(("centre", PATHS[path][0]), flat(st))


@pytest.mark.parametrize("path", list(PATHS))
def test_beam_through_the_sphere(monkeypatch, path):
    """D-beam: every leg with q >= 1e-14, reflected and refracted in vector form about the radial
    normal (the facet's, in the mesh form) with the unpolarised Fresnel reflectance, clipped against
    every voxel. Off the legs absorb and jmean are exactly zero."""
    form = PATHS[path][0]
    jm, ab, ctr, n_batch = run_gpu(monkeypatch, "beam", path)
    st = AC.evaluate_ab("d", jm, ab, ctr, n_batch, AC.reference_d("beam", form), slop=AC.d_track_slop("beam", form))
    print(st)
    AC.check_ab(st)
    predicted(("beam", form), flat(st))


@pytest.mark.parametrize("path", list(PATHS))
def test_total_internal_reflection(monkeypatch, path):
    """D-tir: sin(incidence) = 0.8 > 1 / n at every hit of the sphere. SDF forms: escaped is exactly
    0, absorbed exactly N, jmean and absorb exactly 0 in every voxel wholly outside radius
    R + 1e-6, and the star polygon's legs are pinned per voxel. Mesh form: some facets transmit;
    the polyhedron's own reference decides, and the zeros hold where it has none."""
    form = PATHS[path][0]
    jm, ab, ctr, n_batch = run_gpu(monkeypatch, "tir", path)
    st = AC.evaluate_ab("d", jm, ab, ctr, n_batch, AC.reference_d("tir", form), slop=AC.d_track_slop("tir", form))
    print(st)
    AC.check_ab(st)
    if form != "mesh":
        assert ctr["escaped"] == 0 and ctr["absorbed"] == n_batch * AC.BATCHES, ctr
        _, outside = AR.ball_voxels(*AC.faces(), AC.D_CENTRE, AC.D_R + 1e-6)
        assert outside.sum() >= 300 and not jm.sum(axis=0)[outside].any() and not ab.sum(axis=0)[outside].any()
    predicted(("tir", form), flat(st))


@pytest.mark.parametrize("path", ["transport", "mesh"])
def test_total_internal_reflection_with_survival_bias(monkeypatch, path):
    """D-tir with FLAG_SURVIVAL_BIAS: absorb holds fp64 weights; absorb and jmean by batch means."""
    form = PATHS[path][0]
    jm, ab, ctr, n_batch = run_gpu(monkeypatch, "tir", path, flags=PL | abi.FLAG_SURVIVAL_BIAS)
    st = AC.evaluate_weighted(jm, ab, ctr, n_batch, AC.reference_d("tir", form), AC.d_track_slop("tir", form))
    print(st)
    AC.check_weighted(st)
    predicted(("tir", form, True), flat_weighted(st))


@pytest.mark.parametrize("path", ["transport", "mesh"])
def test_beam_detectors(monkeypatch, path):
    """D-beam's two circles: Binomial(N, q) in the one ring where the doubly refracted and the
    reflected leg land, every other bin exactly 0 (a scene with detectors does not take the lean
    path)."""
    form = PATHS[path][0]
    bins, ctr, n = run_gpu(monkeypatch, "beam", path, dets=AC.dets_d(form))
    st = AC.evaluate_det(bins, AC.expected_d(form)[0], n, ctr["detector_hits"])
    print(st)
    AC.check_det(st, AC.B_POOL_CAP)
    assert all(np.count_nonzero(b) == 1 and b[AC.D_DET_BIN] > 0 for b in bins)
    predicted(("det", form), {**AC.flat_det(st), "digest": AC.digest(bins)}, PREDICTED_DET)
