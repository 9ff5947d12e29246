"""The HIP path against closed forms that need neither the restatements nor the reference
(DESIGN.md §3.5): the per-voxel absorb and jmean grids of

  A  an isotropic point source in a homogeneous absorber,
  B  an oblique pencil beam through an index-mismatched absorbing slab,
  C  any scattering scene: mua(v) * jmean[v] and absorb[v] estimate the same absorption,

on a grid with three different voxel edges and counts, through ws_kernel, transport_kernel,
voxel_kernel and mesh_kernel, and for A through every deposit regime. The expectations are
tests/analytic_ref.py (plain numpy), the scenes, statistics and bounds tests/analytic_cases.py;
tests/test_analytic_cpu.py checks the reference against itself, shows that the bounds reject a
reference that is wrong by 1 %, and runs the same assertions on the CPU restatements.

Each case is 24 batches of one seed over disjoint photon ranges. Asserted (analytic_cases.check_ab,
check_c), with a family-wise false-alarm rate of 1e-3 per test: the absorb counts as a multinomial
(max |z| over the voxels, sum z^2 against chi^2_V), exact zeros off the support, the absorbed and
escaped counters as a binomial, and the batch means of jmean per voxel and summed (max |t|, the
mean of t^2 between its quantiles, the t scores' chi^2, t of the sum; Student-t with 23 degrees
of freedom), with the pooling conditions on counts and tracks alike. The seeds are fixed and the
integer tallies equal the restatements' bit for bit, so each statistic is known beforehand from a
CPU run of the same photons: PREDICTED holds them, and the test asserts them too.
"""
import pytest

from rsmcrt_amd import abi
from rsmcrt_amd.engine import Engine
from tests import analytic_cases as AC

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH

# path -> (scene form, environment, ws_kernel runs)
PATHS = {
    "ws": ("sdf", {}, True),
    "transport": ("sdf", {"SMCRT_LEAN": "0"}, False),
    "voxel": ("voxel", {}, False),
    "mesh": ("mesh", {}, False),
}
# scene A's SDF form in the deposit regimes of test_gpu_parity.test_deposit_paths: ws_kernel files
# into buckets only (sceneplan.h launch_lean), the other regimes run transport_kernel
REGIMES = {
    "buckets": ({}, "buckets"),
    "sorted-fused-hist": ({"SMCRT_DEPOSIT": "sorted"}, "sorted"),
    "sorted-hist-kernel": ({"SMCRT_FUSED_HIST": "0"}, "sorted"),
    "atomics": ({"SMCRT_DEPOSIT": "atomic"}, "atomic"),
}

# Photons per batch (x 24): the 2e7 photons aimed at, on every path. Beside each: the time of the
# test's call seen on one MI355X in a run of this file, which takes 13 s for its 18 tests. The
# yardstick, the parent commit's test_gpu_voxel.py and test_gpu_mesh.py in the same session: 48
# tests in 13.5 s, the slowest calls 4.1 s (test_gpu_mesh.test_refusals), 1.3 s, 1.0 s, 0.7 s.
N_BATCH = {
    ("a", "ws"): 840_000,         # 0.35 s (sorted 0.07 s, atomics 0.32 s)
    ("a", "transport"): 840_000,  # 0.07 s
    ("a", "voxel"): 840_000,      # 0.07 s
    ("a", "mesh"): 840_000,       # 0.07 s
    ("b", "ws"): 840_000,         # 0.98 s
    ("b", "transport"): 840_000,  # 0.09 s
    ("b", "voxel"): 840_000,      # 0.08 s
    ("b", "mesh"): 840_000,       # 0.08 s
    ("c", "ws"): 840_000,         # 1.77 s
    ("c", "transport"): 840_000,  # 1.79 s, survival bias 2.99 s
    ("c", "voxel"): 840_000,      # 0.07 s, survival bias 0.61 s
    ("c", "mesh"): 840_000,       # 0.09 s, survival bias 0.63 s
}

# The statistics of the CPU restatements (oracle/, tests/voxel_ref.c, tests/mesh_ref.c) on the same
# photons, seed and batches, computed before the GPU ran them. Bounds at these counts:
#   A  max |z| 5.23, chi^2 in [803.7, 1133.8] (960 bins, none pooled), |z_absorbed| 3.59,
#      max |t| 7.67, mean t^2 in [0.884, 1.307], score 1133.8 (960 bins, none pooled), |t_sum| 4.77
#   B  max |z| 4.38, chi^2 in [2.0, 43.1] (13 bins and 8 pooled voxels, share 1.3e-5),
#      max |t| 6.26, mean t^2 in [0.353, 2.571], score 79.9 (37 bins and 9 pooled voxels, share 3e-6)
#   C  max |t| 7.18, mean t^2 in [0.898, 1.292], score 1120.0 (960 bins), |t_sum| 4.33
# A's three forms draw the same numbers and give the same tallies.
_A = {"max_z": 2.8988295772, "chi2": 924.03918782, "z_absorbed": -0.3797405343, "max_t": 3.2188950054,
      "mean_t2": 0.9799914569, "score": 868.42735588, "t_sum": 0.1483606393}
PREDICTED = {
    ("a", "sdf"): _A, ("a", "voxel"): _A, ("a", "mesh"): _A,
    ("b", "sdf"): {"max_z": 2.0779465426, "chi2": 12.833641437, "z_absorbed": 2.1654222855, "max_t": 2.0935609539,
                   "mean_t2": 1.1601681550, "score": 40.473291583, "t_sum": -2.1039736701},
    ("b", "voxel"): {"max_z": 2.0779465426, "chi2": 12.831627716, "z_absorbed": 2.1654222855, "max_t": 2.0935933530,
                     "mean_t2": 1.1600912094, "score": 40.470235062, "t_sum": -2.1039752661},
    ("b", "mesh"): {"max_z": 2.0776617473, "chi2": 12.849662260, "z_absorbed": 2.1649561071, "max_t": 2.0935617911,
                    "mean_t2": 1.1598643315, "score": 40.462764497, "t_sum": -2.1040955839},
    ("c", "sdf", False): {"max_t": 3.8856633787, "mean_t2": 1.1099886114, "score": 972.01217235, "t_sum": 0.8678670598,
                          "n_pooled": 0, "absorb_sum": 14428734.0},
    ("c", "voxel", False): {"max_t": 3.8856555010, "mean_t2": 1.1099456011, "score": 971.97414765, "t_sum": 0.8674659370,
                            "n_pooled": 0, "absorb_sum": 14428734.0},
    ("c", "mesh", False): {"max_t": 3.8853760014, "mean_t2": 1.1102245248, "score": 972.24516257, "t_sum": 0.8651049088,
                           "n_pooled": 0, "absorb_sum": 14428739.0},
    ("c", "sdf", True): {"max_t": 3.9384247858, "mean_t2": 1.2035972857, "score": 1053.7747561, "t_sum": -0.1223130853,
                         "n_pooled": 0, "absorb_sum": 14429565.650029},
    ("c", "voxel", True): {"max_t": 3.9384449876, "mean_t2": 1.2035546407, "score": 1053.7393712, "t_sum": -0.1222058333,
                           "n_pooled": 0, "absorb_sum": 14429564.970541},
    ("c", "mesh", True): {"max_t": 3.9350315284, "mean_t2": 1.2032718453, "score": 1053.4973007, "t_sum": -0.1215497623,
                          "n_pooled": 0, "absorb_sum": 14429566.226278},
}


def run_gpu(monkeypatch, which, path, flags=PL, env=(), regime=None):
    form, penv, lean = PATHS[path]
    for k, v in {**penv, **dict(env)}.items():
        monkeypatch.setenv(k, v)
    sc, src = getattr(AC, "scene_" + which)(form)
    n_batch = N_BATCH[which, path]
    with Engine(sc, AC.grid()) as eng:
        if regime is not None:
            assert eng.deposit_regime() == regime
        eng.kernel_times()
        jm, ab, ctr = AC.run_batches(
            lambda first, n: eng.run(src, n, seed=AC.SEED, flags=flags, first_photon=first), n_batch)
        eng.check()
        kt = eng.kernel_times()
    if lean and regime in (None, "buckets") and not flags & abi.FLAG_SURVIVAL_BIAS:
        assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, kt
    else:
        assert kt["lean_launches"] == 0, kt
    assert (ctr["sdf_evals"] > 0) == (form == "sdf"), ctr
    assert ctr["photons"] == n_batch * AC.BATCHES
    return jm, ab, ctr, n_batch


def predicted(key, got):
    """The statistics equal the restatement's: those of integer tallies to rounding, those of
    jmean (equal to 1e-12 per voxel; a t is a difference of 1e-3 of it over its error) to 1e-6."""
    want = PREDICTED.get(key)
    print(key, got)
    assert want is not None, f"no prediction recorded for {key}"
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-6, abs=1e-6), (k, got[k], v)


def flat(st):
    """The figures of evaluate_ab that PREDICTED records."""
    return {"max_z": st["counts"]["max_z"], "chi2": st["counts"]["chi2"], "z_absorbed": st["z_absorbed"],
            "max_t": st["tracks"]["max_t"], "mean_t2": st["tracks"]["mean_t2"], "score": st["tracks"]["score"], "t_sum": st["tracks"]["t_sum"]}


@pytest.mark.parametrize("case", list(REGIMES) + ["transport", "voxel", "mesh"])
def test_point_source_in_absorber(monkeypatch, case):
    """Scene A, mua = 2: absorb[v] is multinomial with p_v = mua T(V), T(V) the integral of
    exp(-mua r) / (4 pi r^2) over the voxel; no voxel is pooled (N p_v >= 100 everywhere)."""
    path = case if case in PATHS else "ws"
    env, regime = REGIMES.get(case, ({}, None))
    jm, ab, ctr, n_batch = run_gpu(monkeypatch, "a", path, env=env, regime=regime)
    st = AC.evaluate_ab("a", jm, ab, ctr, n_batch, AC.reference_a())
    print(st)
    AC.check_ab(st)
    predicted(("a", PATHS[path][0]), flat(st))


@pytest.mark.parametrize("path", list(PATHS))
def test_beam_through_slab(monkeypatch, path):
    """Scene B: every leg of the beam, reflected and refracted at the slab's two planes with the
    unpolarised Fresnel reflectance, clipped against every voxel. Off the beam absorb and jmean
    are exactly zero; the voxels of the rare legs (N p_v < 100) hold less than 1e-3 of the
    absorptions and are one pooled bin."""
    jm, ab, ctr, n_batch = run_gpu(monkeypatch, "b", path)
    st = AC.evaluate_ab("b", jm, ab, ctr, n_batch, AC.reference_b(PATHS[path][0]))
    print(st)
    AC.check_ab(st)
    predicted(("b", PATHS[path][0]), flat(st))


@pytest.mark.parametrize("path,survival", [(p, False) for p in PATHS] + [(p, True) for p in PATHS if p != "ws"],
                         ids=lambda v: v if isinstance(v, str) else ("survival-bias" if v else "analogue"))
def test_track_length_equals_collision_estimator(monkeypatch, path, survival):
    """Scene C: two scattering media with an index mismatch. Per batch and voxel
    mua(v) * jmean[v] - absorb[v] has expectation zero; with FLAG_SURVIVAL_BIAS absorb holds
    fp64 weights (the atomic path; ws_kernel does not take such runs, launch_lean)."""
    flags = PL | (abi.FLAG_SURVIVAL_BIAS if survival else 0)
    jm, ab, ctr, n_batch = run_gpu(monkeypatch, "c", path, flags=flags)
    st = AC.evaluate_c(jm, ab, ctr)
    print(st)
    AC.check_c(st)
    predicted(("c", PATHS[path][0], survival), {k: st[k] for k in ("max_t", "mean_t2", "score", "t_sum", "n_pooled", "absorb_sum")})
