"""The HIP path against exact transport solutions of a scattering medium (DESIGN.md §3.5
"Scattering media"): in a homogeneous medium that is effectively infinite, the absorption sites
projected onto an axis are the scalar flux of a 1-D plane-geometry problem, whose Fourier
transform solves a tridiagonal system in the Legendre moments of the Henyey-Greenstein kernel
(tests/analytic_ref.py, scatter_cumulative: plain numpy, nothing of the project). So every voxel
layer of absorb and of jmean has an exact expectation along x, y and z:

  S-iso     an isotropic point source, g = 0.8, 0 and -0.5: both branches of scatter()'s cosine
            draw, back-scattering, the general rotation;
  S-beam    a pencil beam along -z and along +z, g = 0.8: one pole branch of scatter() each at
            every photon's first scattering;
  S-mirror  S-iso with the source on a voxel centre in x and z and a voxel face in y: besides the
            layers, the voxels of every mirror orbit about the source are equiprobable (the only
            per-voxel check: a sign or azimuth error that leaves the marginals intact);

through ws_kernel, transport_kernel, voxel_kernel and mesh_kernel, and S-iso g = 0.8 with
FLAG_SURVIVAL_BIAS (absorb holds weights and is tested by batch means like jmean). The scenes,
statistics and bounds are tests/analytic_cases.py; tests/test_scatter_analytic_cpu.py checks the
reference against itself and a numpy random walk, asserts the conditions on the grid (escapes,
populated layers, the reference's error), and shows that the assertions reject wrong references.

Each case is 24 batches of one seed over disjoint photon ranges. Asserted with a family-wise
false-alarm rate of 1e-3 per test (analytic_cases.check_s, check_mirror): per axis the absorb layer
sums as a multinomial and the batch means of the jmean layer sums against p / mua; the `scatters`
counter against a / (1 - a); absorbed == photons, escaped == 0 and faults == 0 outright. The
integer tallies equal the restatements' bit for bit, so each statistic is known beforehand from a
CPU run of the same photons: PREDICTED holds them, and the test asserts them too.
"""
import pytest

from rsmcrt_amd import abi
from rsmcrt_amd.engine import Engine
from tests import analytic_cases as AC

pytestmark = pytest.mark.gpu

PL = abi.FLAG_PATHLENGTH

# path -> (scene form, environment, ws_kernel runs), as in tests/test_gpu_analytic.py
PATHS = {
    "ws": ("sdf", {}, True),
    "transport": ("sdf", {"SMCRT_LEAN": "0"}, False),
    "voxel": ("voxel", {}, False),
    "mesh": ("mesh", {}, False),
}

# Photons per batch (x 24 = 2.016e7), on every path. The times of the tests' calls on one MI355X,
# in a run of this file that takes 17 s for its 27 tests (the first test of a case also computes
# its reference, 0.3 s for a point source and 1.2 s for a beam):
#   ws         3.27 s (beam -z, the engine 1.67 s of it), 2.20 s (iso g = 0.8), 1.43 s (g = 0),
#              1.27 s (beam +z), 0.96 s (g = -0.5), 0.85 s (mirror)
#   transport, voxel, mesh   0.10 to 0.16 s; with survival bias 0.66, 0.63 and 0.64 s
# The yardstick, test_gpu_analytic.py's scene-C calls in the same session: 3.03 s (transport with
# survival bias), 1.92 s (ws), 1.82 s (transport); a test here may take twice the slowest, 6.1 s.
N_BATCH = 840_000

# The statistics of the CPU restatements (oracle/, tests/voxel_ref.c, tests/mesh_ref.c) on the same
# photons, seed and batches, computed before the GPU ran them.
PREDICTED = {
    ("iso-g0.8", "sdf", False): {"z_scatters": 0.3422781197, "x_max_z": 1.933915319, "x_chi2": 16.32031391, "x_max_t": 3.23894909, "x_mean_t2": 1.322368035, "x_score": 25.49540054, "x_t_sum": 0.7751929405, "y_max_z": 1.767616821, "y_chi2": 24.87093735, "y_max_t": 1.772944444, "y_mean_t2": 0.7446237828, "y_score": 18.21366499, "y_t_sum": 0.7751895505, "z_max_z": 2.409711531, "z_chi2": 26.00528839, "z_max_t": 2.554236903, "z_mean_t2": 1.759888016, "z_score": 31.54898864, "z_t_sum": 0.7751913764},
    ("iso-g0.8", "voxel", False): {"z_scatters": 0.3422781197, "x_max_z": 1.933915319, "x_chi2": 16.3232574, "x_max_t": 3.238972105, "x_mean_t2": 1.322393449, "x_score": 25.49586591, "x_t_sum": 0.775192934, "y_max_z": 1.767616821, "y_chi2": 24.87093735, "y_max_t": 1.772933262, "y_mean_t2": 0.7446102347, "y_score": 18.21335294, "y_t_sum": 0.775189544, "z_max_z": 2.409711531, "z_chi2": 26.00528839, "z_max_t": 2.554229844, "z_mean_t2": 1.759890429, "z_score": 31.54905143, "z_t_sum": 0.7751913699},
    ("iso-g0.8", "mesh", False): {"z_scatters": 0.3422781197, "x_max_z": 1.933915319, "x_chi2": 16.32031391, "x_max_t": 3.23894909, "x_mean_t2": 1.322368035, "x_score": 25.49540054, "x_t_sum": 0.7751929405, "y_max_z": 1.767616821, "y_chi2": 24.87093735, "y_max_t": 1.772944444, "y_mean_t2": 0.7446237828, "y_score": 18.21366499, "y_t_sum": 0.7751895505, "z_max_z": 2.409711531, "z_chi2": 26.00528839, "z_max_t": 2.554236903, "z_mean_t2": 1.759888016, "z_score": 31.54898864, "z_t_sum": 0.7751913764},
    ("iso-g0", "sdf", False): {"z_scatters": 0.3422781197, "x_max_z": 2.03634233, "x_chi2": 11.9704202, "x_max_t": 2.181084176, "x_mean_t2": 0.5854518617, "x_score": 8.639143271, "x_t_sum": 0.7751854915, "y_max_z": 2.487554723, "y_chi2": 24.4137228, "y_max_t": 2.10385342, "y_mean_t2": 1.469717331, "y_score": 23.24815442, "y_t_sum": 0.775165888, "z_max_z": 1.340189428, "z_chi2": 5.836277789, "z_max_t": 2.459737256, "z_mean_t2": 1.476249108, "z_score": 17.3418196, "z_t_sum": 0.7751753991},
    ("iso-g0", "voxel", False): {"z_scatters": 0.3422781197, "x_max_z": 2.03634233, "x_chi2": 11.9704202, "x_max_t": 2.181071662, "x_mean_t2": 0.5854380747, "x_score": 8.638947113, "x_t_sum": 0.7751855065, "y_max_z": 2.487554723, "y_chi2": 24.4137228, "y_max_t": 2.103811217, "y_mean_t2": 1.469670194, "y_score": 23.24743984, "y_t_sum": 0.775165903, "z_max_z": 1.340189428, "z_chi2": 5.837532873, "z_max_t": 2.459763353, "z_mean_t2": 1.476285279, "z_score": 17.34221692, "z_t_sum": 0.7751754142},
    ("iso-g0", "mesh", False): {"z_scatters": 0.3422781197, "x_max_z": 2.03634233, "x_chi2": 11.9704202, "x_max_t": 2.181084176, "x_mean_t2": 0.5854518617, "x_score": 8.639143271, "x_t_sum": 0.7751854915, "y_max_z": 2.487554723, "y_chi2": 24.4137228, "y_max_t": 2.10385342, "y_mean_t2": 1.469717331, "y_score": 23.24815442, "y_t_sum": 0.775165888, "z_max_z": 1.340189428, "z_chi2": 5.836277789, "z_max_t": 2.459737256, "z_mean_t2": 1.476249108, "z_score": 17.3418196, "z_t_sum": 0.7751753991},
    ("iso-g-0.5", "sdf", False): {"z_scatters": 0.3422781197, "x_max_z": 2.03049171, "x_chi2": 15.16847728, "x_max_t": 2.37362917, "x_mean_t2": 0.8576381126, "x_score": 11.01479585, "x_t_sum": 0.7751733051, "y_max_z": 2.098083074, "y_chi2": 17.14065727, "y_max_t": 1.726152859, "y_mean_t2": 0.7716754533, "y_score": 11.65613427, "y_t_sum": 0.7751389934, "z_max_z": 2.274912359, "z_chi2": 11.66418539, "z_max_t": 1.676993808, "z_mean_t2": 0.701147498, "z_score": 7.940536118, "z_t_sum": 0.7751582106},
    ("iso-g-0.5", "voxel", False): {"z_scatters": 0.3422781197, "x_max_z": 2.03049171, "x_chi2": 15.16847728, "x_max_t": 2.37363353, "x_mean_t2": 0.8576438806, "x_score": 11.01486615, "x_t_sum": 0.7751732913, "y_max_z": 2.098083074, "y_chi2": 17.14065727, "y_max_t": 1.726147597, "y_mean_t2": 0.77164354, "y_score": 11.65566447, "y_t_sum": 0.7751389797, "z_max_z": 2.274912359, "z_chi2": 11.66418539, "z_max_t": 1.676985662, "z_mean_t2": 0.7011535812, "z_score": 7.940600854, "z_t_sum": 0.7751581969},
    ("iso-g-0.5", "mesh", False): {"z_scatters": 0.3422781197, "x_max_z": 2.03049171, "x_chi2": 15.16847728, "x_max_t": 2.37362917, "x_mean_t2": 0.8576381126, "x_score": 11.01479585, "x_t_sum": 0.7751733051, "y_max_z": 2.098083074, "y_chi2": 17.14065727, "y_max_t": 1.726152859, "y_mean_t2": 0.7716754533, "y_score": 11.65613427, "y_t_sum": 0.7751389934, "z_max_z": 2.274912359, "z_chi2": 11.66418539, "z_max_t": 1.676993808, "z_mean_t2": 0.701147498, "z_score": 7.940536118, "z_t_sum": 0.7751582106},
    ("beam-z-", "sdf", False): {"z_scatters": 1.457996181, "x_max_z": 1.938865197, "x_chi2": 14.46836872, "x_max_t": 1.509059256, "x_mean_t2": 0.6150695128, "x_score": 12.84828769, "x_t_sum": 0.02135664103, "y_max_z": 2.850813633, "y_chi2": 28.89410985, "y_max_t": 3.115121987, "y_mean_t2": 1.286046312, "y_score": 27.62798797, "y_t_sum": 0.02135371094, "z_max_z": 2.331635031, "z_chi2": 18.57612113, "z_max_t": 1.856668462, "z_mean_t2": 0.4715166265, "z_score": 7.840883971, "z_t_sum": 0.02142662959},
    ("beam-z-", "voxel", False): {"z_scatters": 1.457996181, "x_max_z": 1.938865197, "x_chi2": 14.50255542, "x_max_t": 1.509040404, "x_mean_t2": 0.6150769573, "x_score": 12.84844664, "x_t_sum": 0.02135663637, "y_max_z": 2.850813633, "y_chi2": 28.88733778, "y_max_t": 3.115158945, "y_mean_t2": 1.286065937, "y_score": 27.62834867, "y_t_sum": 0.02135370628, "z_max_z": 2.331635031, "z_chi2": 18.57046188, "z_max_t": 1.856662856, "z_mean_t2": 0.4715065876, "z_score": 7.840715666, "z_t_sum": 0.02142662493},
    ("beam-z-", "mesh", False): {"z_scatters": 1.457996181, "x_max_z": 1.938865197, "x_chi2": 14.46836872, "x_max_t": 1.509059256, "x_mean_t2": 0.6150695128, "x_score": 12.84828769, "x_t_sum": 0.02135664103, "y_max_z": 2.850813633, "y_chi2": 28.89410985, "y_max_t": 3.115121987, "y_mean_t2": 1.286046312, "y_score": 27.62798797, "y_t_sum": 0.02135371094, "z_max_z": 2.331635031, "z_chi2": 18.57612113, "z_max_t": 1.856668462, "z_mean_t2": 0.4715166265, "z_score": 7.840883971, "z_t_sum": 0.02142662959},
    ("beam-z+", "sdf", False): {"z_scatters": 1.457996181, "x_max_z": 2.137521024, "x_chi2": 19.79391032, "x_max_t": 1.70315393, "x_mean_t2": 0.6912553279, "x_score": 14.43104124, "x_t_sum": 0.02135707755, "y_max_z": 2.05082417, "y_chi2": 18.40277272, "y_max_t": 1.287910912, "y_mean_t2": 0.4604231144, "y_score": 10.60703781, "y_t_sum": 0.02135414747, "z_max_z": 1.977887473, "z_chi2": 10.08298579, "z_max_t": 2.641655888, "z_mean_t2": 1.02964277, "z_score": 17.92627501, "z_t_sum": 0.02142802847},
    ("beam-z+", "voxel", False): {"z_scatters": 1.457996181, "x_max_z": 2.137521024, "x_chi2": 19.79391032, "x_max_t": 1.703142639, "x_mean_t2": 0.6912474917, "x_score": 14.43088509, "x_t_sum": 0.02135707312, "y_max_z": 2.05082417, "y_chi2": 18.40277272, "y_max_t": 1.287885546, "y_mean_t2": 0.4604263069, "y_score": 10.60710928, "y_t_sum": 0.02135414303, "z_max_z": 1.977887473, "z_chi2": 10.08311864, "z_max_t": 2.641680381, "z_mean_t2": 1.029656642, "z_score": 17.9264968, "z_t_sum": 0.02142802403},
    ("beam-z+", "mesh", False): {"z_scatters": 1.457996181, "x_max_z": 2.137521024, "x_chi2": 19.79391032, "x_max_t": 1.70315393, "x_mean_t2": 0.6912553279, "x_score": 14.43104124, "x_t_sum": 0.02135707755, "y_max_z": 2.05082417, "y_chi2": 18.40277272, "y_max_t": 1.287910912, "y_mean_t2": 0.4604231144, "y_score": 10.60703781, "y_t_sum": 0.02135414747, "z_max_z": 1.977887473, "z_chi2": 10.08298579, "z_max_t": 2.641655888, "z_mean_t2": 1.02964277, "z_score": 17.92627501, "z_t_sum": 0.02142802847},
    ("mirror", "sdf", False): {"z_scatters": 0.3422781197, "x_max_z": 1.613120145, "x_chi2": 13.88243968, "x_max_t": 3.180858904, "x_mean_t2": 1.265855948, "x_score": 24.56842661, "x_t_sum": 0.7751929538, "y_max_z": 2.189351313, "y_chi2": 19.45002929, "y_max_t": 1.800062788, "y_mean_t2": 0.6869791336, "y_score": 16.24468427, "y_t_sum": 0.7751890555, "z_max_z": 3.069545356, "z_chi2": 29.67328089, "z_max_t": 2.988664982, "z_mean_t2": 1.804106898, "z_score": 31.99144917, "z_t_sum": 0.7751916682},
    ("mirror", "voxel", False): {"z_scatters": 0.3422781197, "x_max_z": 1.613120145, "x_chi2": 13.88243968, "x_max_t": 3.18088137, "x_mean_t2": 1.265877767, "x_score": 24.56882538, "x_t_sum": 0.7751929622, "y_max_z": 2.189351313, "y_chi2": 19.45002929, "y_max_t": 1.800048304, "y_mean_t2": 0.6869833903, "y_score": 16.24477772, "y_t_sum": 0.7751890639, "z_max_z": 3.069545356, "z_chi2": 29.67328089, "z_max_t": 2.988642194, "z_mean_t2": 1.804105435, "z_score": 31.99146378, "z_t_sum": 0.7751916767},
    ("mirror", "mesh", False): {"z_scatters": 0.3422781197, "x_max_z": 1.613120145, "x_chi2": 13.88243968, "x_max_t": 3.180858904, "x_mean_t2": 1.265855948, "x_score": 24.56842661, "x_t_sum": 0.7751929538, "y_max_z": 2.189351313, "y_chi2": 19.45002929, "y_max_t": 1.800062788, "y_mean_t2": 0.6869791336, "y_score": 16.24468427, "y_t_sum": 0.7751890555, "z_max_z": 3.069545356, "z_chi2": 29.67328089, "z_max_t": 2.988664982, "z_mean_t2": 1.804106898, "z_score": 31.99144917, "z_t_sum": 0.7751916682},
    ("iso-g0.8", "sdf", True): {"x_ab_max_t": 2.108024906, "x_ab_mean_t2": 1.190311983, "x_ab_t_sum": 0.9255433034, "x_max_t": 2.129007591, "x_mean_t2": 1.288401526, "x_score": 26.08820007, "x_t_sum": 0.04430415375, "y_ab_max_t": 2.057114609, "y_ab_mean_t2": 0.8474485736, "y_ab_t_sum": 0.9254137477, "y_max_t": 1.950074614, "y_mean_t2": 0.7896558512, "y_score": 19.32099467, "y_t_sum": 0.04429727075, "z_ab_max_t": 2.147843318, "z_ab_mean_t2": 1.261979385, "z_ab_t_sum": 0.9255053662, "z_max_t": 2.111081763, "z_mean_t2": 1.073500181, "z_score": 19.79342982, "z_t_sum": 0.04430151258},
    ("iso-g0.8", "voxel", True): {"x_ab_max_t": 2.108663229, "x_ab_mean_t2": 1.19043172, "x_ab_t_sum": 0.9255433034, "x_max_t": 2.129040521, "x_mean_t2": 1.288511723, "x_score": 26.09034238, "x_t_sum": 0.04430414158, "y_ab_max_t": 2.057648412, "y_ab_mean_t2": 0.8475971374, "y_ab_t_sum": 0.9254137477, "y_max_t": 1.950210044, "y_mean_t2": 0.7896896255, "y_score": 19.32176156, "y_t_sum": 0.04429725857, "z_ab_max_t": 2.147832325, "z_ab_mean_t2": 1.26197327, "z_ab_t_sum": 0.9255053662, "z_max_t": 2.111114942, "z_mean_t2": 1.073567131, "z_score": 19.79460959, "z_t_sum": 0.0443015004},
    ("iso-g0.8", "mesh", True): {"x_ab_max_t": 2.108024906, "x_ab_mean_t2": 1.190311983, "x_ab_t_sum": 0.9255433034, "x_max_t": 2.129007591, "x_mean_t2": 1.288401526, "x_score": 26.08820007, "x_t_sum": 0.04430415375, "y_ab_max_t": 2.057114609, "y_ab_mean_t2": 0.8474485736, "y_ab_t_sum": 0.9254137477, "y_max_t": 1.950074614, "y_mean_t2": 0.7896558512, "y_score": 19.32099467, "y_t_sum": 0.04429727075, "z_ab_max_t": 2.147843318, "z_ab_mean_t2": 1.261979385, "z_ab_t_sum": 0.9255053662, "z_max_t": 2.111081763, "z_mean_t2": 1.073500181, "z_score": 19.79342982, "z_t_sum": 0.04430151258},
    ("mirror", "sdf", "orbits"): {"orbits": 226, "m_max_z": 3.650998053, "m_chi2": 1209.077675, "x_half_chi2": 3.922330507, "y_half_chi2": 5.971436323, "z_half_chi2": 20.47278639},
    ("mirror", "voxel", "orbits"): {"orbits": 226, "m_max_z": 3.650998053, "m_chi2": 1209.077675, "x_half_chi2": 3.922330507, "y_half_chi2": 5.971436323, "z_half_chi2": 20.47278639},
    ("mirror", "mesh", "orbits"): {"orbits": 226, "m_max_z": 3.650998053, "m_chi2": 1209.077675, "x_half_chi2": 3.922330507, "y_half_chi2": 5.971436323, "z_half_chi2": 20.47278639},
}


def run_gpu(monkeypatch, case, path, flags=PL):
    form, penv, lean = PATHS[path]
    for k, v in penv.items():
        monkeypatch.setenv(k, v)
    sc, src = AC.scene_s(case, form)
    with Engine(sc, AC.grid_s()) as eng:
        eng.kernel_times()
        run = AC.run_layers(lambda first, n: eng.run(src, n, seed=AC.SEED, flags=flags, first_photon=first),
                            N_BATCH, keep_grid=case == "mirror")
        eng.check()
        kt = eng.kernel_times()
    if lean and not flags & abi.FLAG_SURVIVAL_BIAS:
        assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, kt
    else:
        assert kt["lean_launches"] == 0, kt
    ctr = run["ctr"]
    assert (ctr["sdf_evals"] > 0) == (form == "sdf"), ctr
    assert ctr["photons"] == N_BATCH * AC.BATCHES and ctr["escaped"] == 0 and ctr.get("faults", 0) == 0, ctr
    return run


def predicted(key, got):
    """The statistics equal the restatement's: those of integer tallies to rounding, those of
    jmean (equal to 1e-12 per voxel; a t is a difference of 1e-3 of it over its error) to 1e-6."""
    want = PREDICTED.get(key)
    print(key, got)
    assert want is not None, f"no prediction recorded for {key}"
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-6, abs=1e-6), (k, got[k], v)


def check(case, path, run, weighted=False):
    st = AC.evaluate_s(run, N_BATCH, AC.reference_s(case), weighted=weighted)
    print(st)
    AC.check_s(st, min_layers=AC.S_MIN_LAYERS[case])
    predicted((case, PATHS[path][0], weighted), AC.flat_s(st))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", ["iso-g0.8", "iso-g0", "iso-g-0.5"])
def test_point_source_layers(monkeypatch, case, path):
    """S-iso: the layers of absorb and jmean along x, y and z of an isotropic point source at a
    generic position in the medium (mus, mua) = (7, 3)."""
    check(case, path, run_gpu(monkeypatch, case, path))


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", ["beam-z-", "beam-z+"])
def test_beam_layers(monkeypatch, case, path):
    """S-beam: a pencil beam along the z axis, whose first scattering takes a pole branch of
    scatter(): the transverse layers (direction cosine 0 to the axis) and the axial ones (+-1)."""
    check(case, path, run_gpu(monkeypatch, case, path))


@pytest.mark.parametrize("path", list(PATHS))
def test_mirror_orbits(monkeypatch, path):
    """S-mirror: the layers as above, and the homogeneity of every mirror orbit of voxels."""
    run = run_gpu(monkeypatch, "mirror", path)
    check("mirror", path, run)
    ms = AC.mirror_stats(run["grid"])
    print(ms)
    AC.check_mirror(ms)
    predicted(("mirror", PATHS[path][0], "orbits"), AC.flat_mirror(ms))


@pytest.mark.parametrize("path", [p for p in PATHS if p != "ws"])
def test_point_source_layers_survival_bias(monkeypatch, path):
    """S-iso, g = 0.8, with FLAG_SURVIVAL_BIAS: absorb holds fp64 weights (ws_kernel does not take
    such runs), so its layers are batch means against N_b p like the tracks."""
    check("iso-g0.8", path, run_gpu(monkeypatch, "iso-g0.8", path, flags=PL | abi.FLAG_SURVIVAL_BIAS), weighted=True)
