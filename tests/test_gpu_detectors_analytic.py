"""The HIP path's detector bins against closed forms that need neither the restatements nor the
reference, through ws_kernel, transport_kernel, voxel_kernel and mesh_kernel:

  D-A  scene A (a point source in an absorber) with a tilted circle, a camera, an annulus, a fibre
       and the circle again with its normal flipped, which must read exactly zero;
  D-B  scene B (a pencil beam through a slab) with four circles on the beam's planes: each leg
       lands in one bin, every other bin is exactly zero;
  D-C  scene C (scattering): total(circle R) == total(circle r1) + total(annulus r1..R), exact in
       an analogue run, to 1e-12 with survival bias;
  D-O  per-origin totals of a batched launch, and the escape function's launch cells.

The expectations are tests/analytic_ref.py, the detector sets, statistics and bounds
tests/analytic_cases.py; tests/test_detectors_analytic_cpu.py checks the expectations against
independent quadratures, shows that the assertions reject each misread hit rule, and runs them on
the CPU restatements. Each case is one launch of one seed; a photon of A and B meets a detector at
most once, so the bins are multinomial and no batch variance is needed. Asserted per test, with a
family-wise false-alarm rate of 1e-3: per detector max |z| and sum z^2 of its bins and the
binomial of its total, exact zeros off the support, integer bins, detector_hits == the bins' sum.
The seeds are fixed and the integer bins equal the restatements' bit for bit, so each statistic
and a digest of the bins are known beforehand from a CPU run of the same photons: PREDICTED.
"""
import numpy as np
import pytest

from rsmcrt_amd import abi
from rsmcrt_amd.engine import Engine
from tests import analytic_cases as AC

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH

# path -> (scene form, environment, ws_kernel runs): a scene with detectors takes ws_kernel only
# when SMCRT_LEAN=1 forces it (sceneplan.cpp)
PATHS = {
    "ws": ("sdf", {"SMCRT_LEAN": "1"}, True),
    "transport": ("sdf", {"SMCRT_LEAN": "0"}, False),
    "voxel": ("voxel", {}, False),
    "mesh": ("mesh", {}, False),
}

# Photons per (case, path), one launch each. Beside each: the time of the test's call seen on one
# MI355X in two runs of this file, which took 9.6 s and 9.1 s for its 16 tests (the origins and
# escape test, 2e7 and 1.6e7 photons: 0.11 s). One to three seconds fall on three or four tests
# of a run, not the same ones in both (apparently the first use of a kernel instantiation); the
# launches themselves take the smaller figure. The yardstick, the parent commit's test_gpu_analytic.py in the
# same sessions: 18 tests in 13.1 s and 15.4 s, the slowest calls 3.03 s, 1.82 s, 1.80 s, 0.97 s and
# 4.31 s, 3.00 s, 1.79 s, 0.95 s.
N_PHOTONS = {
    ("a", "ws"): AC.N_GPU,           # 0.24 s, 0.24 s
    ("a", "transport"): AC.N_GPU,    # 0.06 s, 0.06 s
    ("a", "voxel"): AC.N_GPU,        # 0.07 s, 0.06 s
    ("a", "mesh"): AC.N_GPU,         # 1.07 s, 0.06 s
    ("b", "ws"): AC.N_GPU,           # 1.18 s, 0.08 s
    ("b", "transport"): AC.N_GPU,    # 1.59 s, 2.92 s
    ("b", "voxel"): AC.N_GPU,        # 0.07 s, 0.06 s
    ("b", "mesh"): AC.N_GPU,         # 0.07 s, 0.06 s
    # D-C is an identity, no bin needs a count: 2e6 (the restatement's prediction takes 8 s of CPU)
    ("c", "ws"): AC.N_GPU_C,         # 2.18 s, 0.09 s
    ("c", "transport"): AC.N_GPU_C,  # 0.09 s, 2.32 s; survival bias 0.18 s, 0.17 s
    ("c", "voxel"): AC.N_GPU_C,      # 0.02 s, 0.01 s; survival bias 0.06 s, 0.06 s
    ("c", "mesh"): AC.N_GPU_C,       # 0.02 s, 0.02 s; survival bias 0.06 s, 0.06 s
}

# The statistics of the CPU restatements (oracle/, tests/voxel_ref.c, tests/mesh_ref.c) on the same
# photons and seed, computed before the GPU ran them (`python -m tests.test_detectors_analytic_cpu
# predict a b c o`). "digest": (sum of all bins, sum of (i + 1) * bin i), exact integers.
# D-A's three forms draw the same numbers and give the same bins.
_A = {"hits": 3350855, "total0": 928436.0, "max_z0": 2.3224684665, "chi20": 7.3100575857,
      "z_total0": 0.42557819487, "total1": 1464298.0, "max_z1": 0.88704894769, "chi21": 0.78685583559,
      "z_total1": -0.88704894769, "total2": 909635.0, "max_z2": 1.5559332796, "chi22": 6.2670813346,
      "z_total2": 0.018552952373, "total3": 48486.0, "max_z3": 2.729310922, "chi23": 16.961280632,
      "z_total3": 0.069603526425, "total4": 0.0, "digest": (3350855.0, 89424527.0)}
PREDICTED = {
    ('a', 'sdf'): _A, ('a', 'voxel'): _A, ('a', 'mesh'): _A,
    ('b', 'sdf'): {"hits": 6394474, "total0": 856728.0, "max_z0": 0.54790187209, "chi20": 0.33148673861,
        "z_total0": -0.56597585634, "total1": 856728.0, "max_z1": 0.54790187209, "chi21": 0.33148673861,
        "z_total1": -0.56597585634, "total2": 2340543.0, "max_z2": 2.063612777, "chi22": 4.2590094404,
        "z_total2": -2.0637166092, "total3": 2340475.0, "max_z3": 2.063612777, "chi23": 4.2584976933,
        "z_total3": -2.063612777, "digest": (6394474.0, 150631954.0)},
    ('b', 'voxel'): {"hits": 6394474, "total0": 856728.0, "max_z0": 0.54790187209, "chi20": 0.33148673861,
        "z_total0": -0.56597585634, "total1": 856728.0, "max_z1": 0.54790187209, "chi21": 0.33148673861,
        "z_total1": -0.56597585634, "total2": 2340543.0, "max_z2": 2.063612777, "chi22": 4.2590094404,
        "z_total2": -2.0637166092, "total3": 2340475.0, "max_z3": 2.063612777, "chi23": 4.2584976933,
        "z_total3": -2.063612777, "digest": (6394474.0, 150631954.0)},
    ('b', 'mesh'): {"hits": 6394496, "total0": 856728.0, "max_z0": 0.54790187209, "chi20": 0.33182855723,
        "z_total0": -0.56609547852, "total1": 856728.0, "max_z1": 0.54790187209, "chi21": 0.33182855723,
        "z_total1": -0.56609547852, "total2": 2340554.0, "max_z2": 2.0629461242, "chi22": 4.2562632681,
        "z_total2": -2.0630505741, "total3": 2340486.0, "max_z3": 2.0629461242, "chi23": 4.2557467113,
        "z_total3": -2.0629461242, "digest": (6394496.0, 150632581.0)},
    ('c', 'sdf', False): {"bins": [162874.0, 49438.0, 113436.0], "hits": 325748},
    ('c', 'sdf', True): {"bins": [163112.7979646084, 49668.20110238391, 113444.59686232005], "hits": 423308},
    ('c', 'voxel', False): {"bins": [162874.0, 49438.0, 113436.0], "hits": 325748},
    ('c', 'voxel', True): {"bins": [163112.7979646084, 49668.20110238391, 113444.59686232005], "hits": 423308},
    ('c', 'mesh', False): {"bins": [162874.0, 49438.0, 113436.0], "hits": 325748},
    ('c', 'mesh', True): {"bins": [163112.77996694442, 49668.20110238391, 113444.57886465607], "hits": 423308},
}
# totals[k][d] at AC.N_GPU_O photons per origin
PREDICTED_ORIGINS = [
    [185713.0, 181007.0, 0.0],
    [685697.0, 594006.0, 0.0],
    [91268.0, 72409.0, 0.0],
    [0.0, 0.0, 158165.0],
    [16250.0, 21419.0, 0.0],
]
# escape_sym[d] (fp32) at each launch cell, AC.N_GPU_E photons per cell
PREDICTED_ESCAPE = [
    [0.008142000064253807, 0.007012499962002039, 0.0],
    [0.0, 0.0, 0.18634499609470367],
    [0.00810999982059002, 0.0063355001620948315, 0.0],
    [0.0, 0.0, 0.23119349777698517],
    [0.00975400023162365, 0.006411499809473753, 0.0],
    [0.0, 0.0, 0.21418499946594238],
    [0.0096859997138381, 0.005839500110596418, 0.0],
    [0.0, 0.0, 0.2708264887332916],
]


def run_gpu(monkeypatch, which, path, flags=PL):
    form, env, lean = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, src = getattr(AC, "scene_" + which)(form)
    dets = AC.dets_b(form) if which == "b" else getattr(AC, "dets_" + which)()
    n = N_PHOTONS[which, path]
    with Engine(sc, AC.grid(), dets) as eng:
        eng.kernel_times()
        r = eng.run(src, n, seed=AC.SEED, flags=flags)
        eng.check()
        kt = eng.kernel_times()
    if lean:
        assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, kt
    else:
        assert kt["lean_launches"] == 0, kt
    ctr = r.counters_dict()
    assert (ctr["sdf_evals"] > 0) == (form == "sdf"), ctr
    assert ctr["photons"] == n and ctr.get("faults", 0) == 0, ctr
    return [r.detector(i).copy() for i in range(len(dets))], ctr, n


def predicted(key, got):
    """Statistics of integer bins equal the restatement's to rounding; the digest exactly."""
    want = PREDICTED.get(key)
    print(key, got)
    assert want is not None, f"no prediction recorded for {key}"
    for k, v in want.items():
        if k == "digest":
            assert tuple(got[k]) == tuple(v), (k, got[k], v)
        else:
            assert got[k] == pytest.approx(v, rel=1e-6, abs=1e-6), (k, got[k], v)


@pytest.mark.parametrize("path", list(PATHS))
def test_point_source_detectors(monkeypatch, path):
    """D-A: the circle's and the annulus' bins are the ring integrals of h exp(-mu s) / (4 pi s^3)
    about a centre off the source's foot; the camera's one pixel (taken from the source's position)
    counts the rectangle's share of all directions; the fibre's bins are rings on the front lens
    cut at r_max of the signed thin-lens chain; the flipped circle reads zero. The camera's 25
    bins stand second, so every later detector's offset depends on them."""
    bins, ctr, n = run_gpu(monkeypatch, "a", path)
    st = AC.evaluate_det(bins, AC.expected_a(), n, ctr["detector_hits"])
    print(st)
    AC.check_det(st)
    assert not bins[4].any()
    predicted(("a", PATHS[path][0]), {**AC.flat_det(st), "digest": AC.digest(bins)})


@pytest.mark.parametrize("path", list(PATHS))
def test_beam_detectors(monkeypatch, path):
    """D-B: Binomial(N, q exp(-mu s)) in each leg's landing bin, exact zeros elsewhere (the legs
    that cross a plane against its normal, or leave the grid before they reach it, among them);
    the landings below 100 expected photons are pooled and hold less than 1e-3."""
    bins, ctr, n = run_gpu(monkeypatch, "b", path)
    st = AC.evaluate_det(bins, AC.expected_b(PATHS[path][0])[0], n, ctr["detector_hits"])
    print(st)
    AC.check_det(st, AC.B_POOL_CAP)
    predicted(("b", PATHS[path][0]), {**AC.flat_det(st), "digest": AC.digest(bins)})


@pytest.mark.parametrize("path,survival", [(p, False) for p in PATHS] + [(p, True) for p in PATHS if p != "ws"],
                         ids=lambda v: v if isinstance(v, str) else ("survival-bias" if v else "analogue"))
def test_circle_is_inner_circle_plus_annulus(monkeypatch, path, survival):
    """D-C: one plane inside the scattering slab; with FLAG_SURVIVAL_BIAS the bins hold fp64
    weights added atomically (ws_kernel does not take such runs, launch_lean)."""
    flags = PL | (abi.FLAG_SURVIVAL_BIAS if survival else 0)
    bins, ctr, n = run_gpu(monkeypatch, "c", path, flags=flags)
    tot = [float(b.sum()) for b in bins]
    print(tot, ctr["detector_hits"])
    AC.check_identity(tot, ctr, survival)
    want = PREDICTED.get(("c", PATHS[path][0], survival))
    assert want is not None
    assert ctr["detector_hits"] == want["hits"]
    if survival:
        np.testing.assert_allclose(tot, want["bins"], rtol=1e-12, atol=0.0)
    else:
        assert tot == want["bins"]


def test_origin_totals_and_escape_cells(monkeypatch):
    """D-O: totals[k, d] of a batched launch are Binomial(N, p_kd), with p_kd chosen so that a
    [detector][origin] stride cannot pass (five origins, three detectors, the flipped circle seen
    only from the origin behind the plane); and escape_sym[d, cell] = total / N at each launch
    cell of a 2 x 2 x 2 grid without symmetry. SDF form only (run_origins refuses the others)."""
    monkeypatch.setenv("SMCRT_LEAN", "0")
    sc, _ = AC.scene_a("sdf")
    cfg, idx, _ = AC.escape_case()
    with Engine(sc, AC.grid(), AC.dets_o()) as eng:
        eng.kernel_times()
        tot, res = eng.run_origins(AC.DO_ORIGINS, AC.N_GPU_O, seed=AC.SEED, flags=PL)
        eng.check()
        kt = eng.kernel_times()
        assert kt["lean_launches"] == 0, kt
        es, _, res_e = eng.escape(cfg, AC.N_GPU_E, seed=AC.SEED)
        eng.check()
        kt = eng.kernel_times()
        assert kt["lean_launches"] == 0, kt
    assert res.counter("photons") == AC.N_GPU_O * len(AC.DO_ORIGINS) and res.counter("faults") == 0
    assert res_e.counter("photons") == AC.N_GPU_E * len(idx) and res_e.counter("faults") == 0
    st = AC.evaluate_origins(tot, AC.expected_o(), AC.N_GPU_O)
    print(tot.tolist(), st)
    AC.check_origins(st)
    assert res.counter("detector_hits") == tot.sum()
    AC.check_escape(es, AC.N_GPU_E)
    assert PREDICTED_ORIGINS is not None and PREDICTED_ESCAPE is not None
    assert tot.tolist() == PREDICTED_ORIGINS
    assert [[float(es[d, i, j, k]) for d in range(3)] for i, j, k in idx] == PREDICTED_ESCAPE
