"""The hand-out of ws_kernel's photon waves takes any free slot of the photon (ws.h).

A photon keeps the slot it pushed last and pushes its next segment into the lowest free one, so
its segments' slots follow no fixed order. Nothing that is computed depends on the slot, so every
case is the oracle's and transport_kernel's (SMCRT_LEAN=0) as tests/test_gpu_parity.py compares
them: counters, photon records (the final cells and the draws among them), absorb and emission
bit for bit, jmean at rtol 1e-12. lean_hazards stays 0, and Engine.out_of_order_handouts, the
count of hand-outs that took another slot than a rotation would have, shows that the policy ran.

N_M1, the photons of the M1 case. On that case 4 photons counted 56 such hand-outs, 8 counted 112,
16 counted 169 and 32 counted 334 (of 1,817 segments), one run each. 8 is the smallest power of two
that reached 100, but the count is a schedule statistic that differs from run to run, and 112
leaves no room for that, so the case takes 32, the smallest with a factor of three over the 100
it asserts. With so few photons no photon lane takes a second photon, so two more cases run
262,144 photons (2,520,830 counted, 14,932,296 segments): more than the 131,072 photon lanes of
256 blocks, so that lanes emit into a free slot while segments of their previous photon are
still being walked.
"""
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.engine import Engine
from tests.test_gpu_parity import SEED, compare

pytestmark = pytest.mark.gpu

N_M1 = 32
N_REUSE = 262144
_TJ_SRC = scene.uniform_source((-0.25, 0.0, 0.99999), (0.5, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0))


def _m1():
    return (builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0), scene.grid(64, 64, 64, 1, 1, 1), scene.point_source(), N_M1,
            abi.FLAG_PATHLENGTH, ())


def _m1_reuse():
    return _m1()[:3] + (N_REUSE,) + _m1()[4:]


def _m0():
    return (builders.setup_scat_test(10.0), scene.grid(40, 40, 40, 1, 1, 1), scene.point_source(), 8192,
            abi.FLAG_PATHLENGTH, ())


def _m0_test_kernel():  # the TK = true units
    return (builders.setup_scat_test(10.0), scene.grid(40, 40, 40, 1, 1, 1), scene.point_source(), 8192,
            abi.FLAG_PATHLENGTH | abi.FLAG_TEST_KERNEL, ())


def _tran_jacques():  # the XF instantiation: an event's inputs and results travel in a free slot
    return (builders.setup_tran_and_jacques(), scene.grid(32, 32, 32, 1, 1, 1), _TJ_SRC, 8192, abi.FLAG_PATHLENGTH, ())


def _skin():  # detectors: record_hits in the photon waves (the XF instantiation, SMCRT_LEAN=1)
    dets = (scene.circle_dect((0.0, 0.0, 0.0499), (0.0, 0.0, 1.0), 1, 0.05, 50),
            scene.annulus_dect((0.0, 0.0, 0.0499), (0.0, 0.0, 1.0), 1, 0.005, 0.02, 25))
    return (builders.skin_layers(), scene.grid(48, 48, 48, 0.05, 0.05, 0.05),
            scene.pencil_source((0.0, 0.0, 0.0499), (0.0, 0.0, -1.0)), 8192, abi.FLAG_PATHLENGTH, dets)


CASES = {
    "m1": (_m1, {}),
    "m1-two-slots": (_m1, {"SMCRT_WS_SLOTS": "2"}),
    "m1-lane-reuse": (_m1_reuse, {}),
    "m1-lane-reuse-two-slots": (_m1_reuse, {"SMCRT_WS_SLOTS": "2"}),
    "m0": (_m0, {}),
    "m0-two-slots": (_m0, {"SMCRT_WS_SLOTS": "2"}),
    "tran-jacques": (_tran_jacques, {}),
    "skin-detectors": (_skin, {"SMCRT_LEAN": "1"}),
    "m0-test-kernel": (_m0_test_kernel, {}),
}
_REF = {}  # per scene: the oracle's result and transport_kernel's, shared by its cases


def _run(monkeypatch, make, env):
    sc, g, src, n, flags, dets = make()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with Engine(sc, g, list(dets)) as eng:
        eng.kernel_times()
        res = eng.run(src, n, seed=SEED, flags=flags, records=True)
        eng.check()
        kt = eng.kernel_times()
        ooo = eng.out_of_order_handouts()
    return res, kt, ooo


def _refs(monkeypatch, make):
    if make.__name__ not in _REF:
        sc, g, src, n, flags, dets = make()
        cpu = O.run(sc, g, src, n, seed=SEED, flags=flags, dets=list(dets), records=True)
        with monkeypatch.context() as m:
            full, kt, ooo = _run(m, make, {"SMCRT_LEAN": "0"})
        assert kt["lean_launches"] == 0 and ooo == 0, (kt, ooo)
        _REF[make.__name__] = (cpu, full)
    return _REF[make.__name__]


@pytest.mark.parametrize("case", list(CASES))
def test_any_free_slot_exact(monkeypatch, case):
    make, env = CASES[case]
    cpu, full = _refs(monkeypatch, make)
    gpu, kt, ooo = _run(monkeypatch, make, env)
    print(f"{case}: out-of-order hand-outs {ooo} of {cpu.counter('grid_updates')} segments")
    assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, kt
    compare(gpu, cpu)
    compare(full, cpu)
    compare(gpu, full)
    assert gpu.counter("faults") == cpu.counter("faults")
    assert 0 <= ooo <= cpu.counter("grid_updates")
    if case.startswith(("m1", "m0")):
        assert ooo > 0
    if case == "m1":
        assert ooo >= 100
    if case == "tran-jacques":
        assert cpu.counter("fresnel") > 0
    if case == "skin-detectors":
        assert cpu.counter("detector_hits") > 0
    if case == "m0-test-kernel":
        assert (cpu.moments != 0.0).any()


def test_records_final_cells_and_draws(monkeypatch):
    """Records on: a photon's cells are those of the segment it handed out last, whichever slot that
    took and whichever of its segments finished last; the draws are the oracle's."""
    make, env = CASES["m0"]
    cpu, _ = _refs(monkeypatch, make)
    gpu, kt, ooo = _run(monkeypatch, make, env)
    assert kt["lean_hazards"] == 0 and ooo > 0
    for f in ("cell", "draws", "status", "pos"):
        assert (gpu.records[f] == cpu.records[f]).all(), f
    assert (gpu.absorb == cpu.absorb).all()


def test_absorbed_photons_cells(monkeypatch):
    """An absorbing sphere (mua = 10): most photons are absorbed while deferred segments of theirs are
    still being walked, and recordWeight needs the cells of the one handed out last."""
    def absorbing():
        return (builders.setup_sphere(10.0, 10.0, 0.9, 1.0, 1.0), scene.grid(64, 64, 64, 1, 1, 1), scene.point_source(),
                8192, abi.FLAG_PATHLENGTH, ())
    cpu, full = _refs(monkeypatch, absorbing)
    gpu, kt, ooo = _run(monkeypatch, absorbing, {})
    assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0 and ooo > 0, (kt, ooo)
    assert cpu.counter("absorbed") > 8192 // 2
    compare(gpu, cpu)
    compare(gpu, full)
