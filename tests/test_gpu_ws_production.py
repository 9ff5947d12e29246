"""The lean path's two instantiations by run kind (ws.h, the template parameter TK).

A production run (no FLAG_TEST_KERNEL) takes the ws_kernel whose photon waves hold no inline event
code and no RNG state: every interaction that draws, every tauint2 entry and every emission goes
to the event waves, the photon's draws live in its event slot, and an emission whose slot is
still busy waits for it. A FLAG_TEST_KERNEL run keeps the instantiation with the events (and the
moments) in the photon waves.

Every case is compared with the CPU restatement (oracle/) as tests/test_gpu_parity.py compares
them: counters (rng_draws, scatters, absorbed, ...), nscatt, the photon records (pos, dir, cell,
draws, status, nscatt, ...) and absorb bit for bit, jmean at rtol 1e-12 (only the order of its
fp64 sums differs). lean_launches > 0 shows that ws_kernel ran.
"""
import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.engine import Engine
from tests.test_gpu_parity import SEED, compare

pytestmark = pytest.mark.gpu

N_M1 = 20000
GRIDS = {
    "32": (32, 32, 32),      # power-of-two spacing: grid mode 2
    "48": (48, 48, 48),      # a spacing that is no power of two
    "64x32x16": (64, 32, 16),
}
_ORACLE = {}  # the oracle's M1 result per grid, shared by the cases on that grid


def _m1_scene():
    return builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0)


def _grid(name):
    nx, ny, nz = GRIDS[name]
    return scene.grid(nx, ny, nz, 1, 1, 1)


def _m1_oracle(name):
    if name not in _ORACLE:
        _ORACLE[name] = O.run(_m1_scene(), _grid(name), scene.point_source(), N_M1, seed=SEED,
                              flags=abi.FLAG_PATHLENGTH, records=True)
    return _ORACLE[name]


def _run(monkeypatch, sc, g, src, n, flags, env, lean=True):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with Engine(sc, g) as eng:
        eng.kernel_times()
        res = eng.run(src, n, seed=SEED, flags=flags, records=True)
        eng.check()  # (raises if a watchdog fired)
        kt = eng.kernel_times()
    if lean:
        assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, kt
    else:
        assert kt["lean_launches"] == 0, kt
    return res


@pytest.mark.parametrize("grid,env", [("32", {}), ("48", {}), ("64x32x16", {}), ("64x32x16", {"SMCRT_WS_SLOTS": "2"})],
                         ids=["32", "48", "64x32x16", "64x32x16-two-slots"])
def test_production_run_exact(monkeypatch, grid, env):
    """M1's scene, photons [0, 20000) of seed 123456789, on three grids and with two slots."""
    cpu = _m1_oracle(grid)
    gpu = _run(monkeypatch, _m1_scene(), _grid(grid), scene.point_source(), N_M1, abi.FLAG_PATHLENGTH, env)
    compare(gpu, cpu)
    assert gpu.counter("rng_draws") == cpu.counter("rng_draws") > 0
    assert cpu.counter("scatters") > N_M1 and cpu.counter("absorbed") > 0
    assert gpu.counter("faults") == cpu.counter("faults") == 0


def test_production_run_against_transport_kernel(monkeypatch):
    """The second reference: the same photons through transport_kernel (SMCRT_LEAN=0)."""
    cpu = _m1_oracle("32")
    lean = _run(monkeypatch, _m1_scene(), _grid("32"), scene.point_source(), N_M1, abi.FLAG_PATHLENGTH, {})
    full = _run(monkeypatch, _m1_scene(), _grid("32"), scene.point_source(), N_M1, abi.FLAG_PATHLENGTH,
                {"SMCRT_LEAN": "0"}, lean=False)
    compare(full, cpu)
    compare(lean, full)


@pytest.mark.parametrize("n", [5000, 200000])
def test_emission_waits_for_its_slot(monkeypatch, n):
    """A nearly transparent sphere on a 256 x 16 x 16 grid with two slots: most photons fly straight
    out, in a few long segments that are walked across up to 128 thin voxels each while the photon
    itself is already finished, so the lane's next photon finds its slot P.seq busy and its emission
    waits for the walker (ws.h "Production runs"). The run must stay exact, without a fault and
    without a watchdog expiry (Engine.check).

    5,000 photons are ten blocks of 512 photon lanes, so hardly a lane takes a second photon: a
    -DSMCRT_DIAG build counts no waiting emission on that input ([diag-ws] "emissions waiting for
    a slot"). 200,000 photons are more than the 131,072 photon lanes of 256 blocks, so the lanes
    that finish first fetch again while their walks run; the same build counts the waits of that
    input (profiles/r08_tk/ab_tk.txt), and of M1 itself (17,686 lane-trips per launch)."""
    sc = builders.setup_sphere(0.01, 0.0001, 0.9, 1.0, 1.0)
    g = scene.grid(256, 16, 16, 1, 1, 1)
    src = scene.point_source()
    cpu = O.run(sc, g, src, n, seed=SEED, flags=abi.FLAG_PATHLENGTH, records=True)
    # at least two segments per photon, so the second slot is in use; and nearly all fly out
    print(f"segments/photon {cpu.counter('grid_updates') / n:.2f}, scatters {cpu.counter('scatters')}, "
          f"escaped {cpu.counter('escaped')}")
    assert cpu.counter("grid_updates") >= 2 * n
    assert cpu.counter("escaped") > 0.9 * n
    gpu = _run(monkeypatch, sc, g, src, n, abi.FLAG_PATHLENGTH, {"SMCRT_WS_SLOTS": "2"})
    compare(gpu, cpu)
    assert gpu.counter("faults") == cpu.counter("faults") == 0


@pytest.mark.parametrize("kind", ["plain", "fresnel"])
def test_test_kernel_run_on_the_lean_path(monkeypatch, kind):
    """FLAG_TEST_KERNEL on the lean path, plain and XF instantiation: the moments, which only the
    photon waves' inline scatter adds, and the counters are the oracle's."""
    if kind == "plain":
        sc = builders.setup_scat_test(10.0)
    else:
        sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.33, 1.0)  # n = 1.33 in n = 1: Fresnel interfaces
    g = scene.grid(32, 32, 32, 1, 1, 1)
    n = 5000
    flags = abi.FLAG_PATHLENGTH | abi.FLAG_TEST_KERNEL
    cpu = O.run(sc, g, scene.point_source(), n, seed=SEED, flags=flags, records=True)
    gpu = _run(monkeypatch, sc, g, scene.point_source(), n, flags, {})
    compare(gpu, cpu)
    assert np.any(cpu.moments != 0.0)
    assert cpu.counter("scatters") > 0
    if kind == "fresnel":
        assert cpu.counter("fresnel") > 0
