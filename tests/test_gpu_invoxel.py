"""The lean path's in-voxel segments (ws.h, invoxel.h): a segment that provably ends inside its
start voxel is deposited by its photon wave instead of going to a walker wave.

Every case runs with the fast path on (SMCRT_WS_INVOXEL=1) and off (SMCRT_WS_INVOXEL=0) and against
the CPU restatement (oracle/): counters, photon records, absorb, emission and detector bins bit
for bit, jmean at rtol 1e-12 (only the order of its fp64 sums differs), as
tests/test_gpu_parity.py compares them. Each case also shows that it ran the intended path:
lean launches without hazards, and the count of in-voxel segments (Engine.invoxel_segments) is
0 with the knob off and positive with it on.
"""
import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, builders, scene
from rsmcrt_amd.engine import Engine
from tests.test_gpu_parity import RTOL, SEED, compare

pytestmark = pytest.mark.gpu

_ORACLE = {}  # the oracle's result per scene, shared by the cases that run the same photons


def _m1():
    return (builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0), scene.grid(128, 128, 128, 1, 1, 1), scene.point_source(),
            20000, abi.FLAG_PATHLENGTH, ())


def _skin(with_dets):
    dets = (scene.circle_dect((0.0, 0.0, 0.0499), (0.0, 0.0, 1.0), 1, 0.05, 50),
            scene.annulus_dect((0.0, 0.0, 0.0499), (0.0, 0.0, 1.0), 1, 0.005, 0.02, 25)) if with_dets else ()
    # a pencil beam exactly along -z from x = y = 0, the mid-planes of the 48^3 grid: zero direction
    # components, and starts on a face whose cell is rounded separately ("outside their own cell")
    return (builders.skin_layers(), scene.grid(48, 48, 48, 0.05, 0.05, 0.05),
            scene.pencil_source((0.0, 0.0, 0.0499), (0.0, 0.0, -1.0)), 10000, abi.FLAG_PATHLENGTH, dets)


CASES = {
    # M1's scene and grid, photons [0, 20000) of seed 123456789
    "m1": (_m1, {}),
    "m1-two-slots": (_m1, {"SMCRT_WS_SLOTS": "2"}),
    # a spacing that is not a power of two
    "scat-test-67": (lambda: (builders.setup_scat_test(10.0), scene.grid(67, 67, 67, 1, 1, 1), scene.point_source(), 8000,
                              abi.FLAG_PATHLENGTH, ()), {}),
    # an anisotropic grid, 48 x 40 x 56 cells over half-extents 0.16 x 0.09 x 0.13
    "anisotropic": (lambda: (builders.setup_sphere(100.0, 1.0, 0.9, 1.0, 0.08, bounding=(0.32, 0.18, 0.26)),
                             scene.grid(48, 40, 56, 0.16, 0.09, 0.13), scene.point_source(), 8000, abi.FLAG_PATHLENGTH,
                             ()), {}),
    "skin-pencil": (lambda: _skin(False), {}),
    # mua = 10: many photons are absorbed right after an in-voxel segment while an earlier
    # multi-voxel segment is still being walked (recordWeight needs the newest cells)
    "absorbing": (lambda: (builders.setup_sphere(10.0, 10.0, 0.9, 1.0, 1.0), scene.grid(64, 64, 64, 1, 1, 1),
                           scene.point_source(), 20000, abi.FLAG_PATHLENGTH, ()), {}),
    # the XF instantiation: the Tran & Jacques sphere (Fresnel), the skin scene with two detectors
    "fresnel": (lambda: (builders.setup_tran_and_jacques(), scene.grid(48, 48, 48, 1, 1, 1),
                         scene.uniform_source((-0.25, 0.0, 0.99999), (0.5, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0)),
                         20000, abi.FLAG_PATHLENGTH, ()), {}),
    "skin-detectors": (lambda: _skin(True), {"SMCRT_LEAN": "1"}),
    # test_kernel semantics (moments) on the g = 0 sphere
    "moments": (lambda: (builders.setup_scat_test(10.0), scene.grid(48, 48, 48, 1, 1, 1), scene.point_source(), 20000,
                         abi.FLAG_PATHLENGTH | abi.FLAG_TEST_KERNEL, ()), {}),
}


def _oracle(make):
    key = make.__name__ if make.__name__ != "<lambda>" else id(make)
    if key not in _ORACLE:
        sc, g, src, n, flags, dets = make()
        _ORACLE[key] = O.run(sc, g, src, n, seed=SEED, flags=flags, dets=list(dets), records=True)
    return _ORACLE[key]


def _run(monkeypatch, make, env, knob):
    sc, g, src, n, flags, dets = make()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SMCRT_WS_INVOXEL", knob)
    with Engine(sc, g, list(dets)) as eng:
        eng.kernel_times()
        res = eng.run(src, n, seed=SEED, flags=flags, records=True)
        kt = eng.kernel_times()
        taken = eng.invoxel_segments()
    assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, kt
    return res, taken


@pytest.mark.parametrize("case", list(CASES))
def test_invoxel_segments_exact(monkeypatch, case):
    make, env = CASES[case]
    on, taken_on = _run(monkeypatch, make, env, "1")
    off, taken_off = _run(monkeypatch, make, env, "0")
    cpu = _oracle(make)
    print(f"{case}: in-voxel segments {taken_on} of {cpu.counter('grid_updates')} grid updates, "
          f"{cpu.counter('deposits')} deposits")
    assert taken_off == 0
    assert 0 < taken_on <= cpu.counter("grid_updates")
    compare(on, cpu)
    compare(off, cpu)
    compare(on, off)
    assert on.counter("faults") == cpu.counter("faults")
    if case.startswith("m1"):
        # the restatement alone finds 65.7 % one-record segments on exactly these photons; the
        # predicate's 2^-41 margin cannot move that by a visible amount
        assert taken_on > cpu.counter("grid_updates") // 2
    if case == "absorbing":
        assert cpu.counter("absorbed") > 20000 // 2
    if case in ("fresnel", "skin-detectors", "skin-pencil"):
        assert cpu.counter("fresnel") > 0
    if case == "skin-detectors":
        assert cpu.counter("detector_hits") > 0


def test_invoxel_default_by_instantiation(monkeypatch):
    """Without SMCRT_WS_INVOXEL the plain instantiation (M1's) takes in-voxel segments, and the XF
    instantiation (Fresnel interfaces or detectors), which measured slower with them, does not."""
    monkeypatch.delenv("SMCRT_WS_INVOXEL", raising=False)
    for case, want in (("m1", True), ("fresnel", False)):
        sc, g, src, _, flags, dets = CASES[case][0]()
        with Engine(sc, g, list(dets)) as eng:
            eng.kernel_times()
            eng.run(src, 2000, seed=SEED, flags=flags)
            kt = eng.kernel_times()
            taken = eng.invoxel_segments()
        assert kt["lean_launches"] > 0 and kt["lean_hazards"] == 0, (case, kt)
        assert (taken > 0) == want, (case, taken)


def test_invoxel_deposits_flushed_at_launch_end(monkeypatch):
    """Two asynchronous launches (FLAG_ASYNC_FOLD | FLAG_OVERLAP) on disjoint photon ranges, then a
    fence: the tallies are the oracle's for the union, so every photon lane's pending in-voxel
    sum reached jmean when its wave left."""
    import torch
    sc = builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0)
    g = scene.grid(64, 64, 64, 1, 1, 1)
    src = scene.point_source()
    n = 10000
    nv = 64 ** 3
    dev = torch.device("cuda", 0)
    jm = torch.zeros(nv, dtype=torch.float64, device=dev)
    ab = torch.zeros(nv, dtype=torch.float64, device=dev)
    ctr = torch.zeros(abi.NCOUNTERS, dtype=torch.int64, device=dev)
    dt = abi.DeviceTallies()
    dt.jmean, dt.absorb, dt.counters = jm.data_ptr(), ab.data_ptr(), ctr.data_ptr()
    stream = torch.cuda.current_stream()
    fl = abi.FLAG_PATHLENGTH | abi.FLAG_ASYNC_FOLD | abi.FLAG_OVERLAP
    monkeypatch.setenv("SMCRT_WS_INVOXEL", "1")
    with Engine(sc, g) as eng:
        eng.kernel_times()
        for i in range(2):
            eng.run_device(src, Engine.config(n, seed=SEED, flags=fl, first_photon=i * n), dt, stream.cuda_stream)
        eng.fence(stream.cuda_stream)
        torch.cuda.synchronize()
        eng.check()
        kt = eng.kernel_times()
        taken = eng.invoxel_segments()
    assert kt["lean_launches"] == 2 and kt["lean_hazards"] == 0, kt
    cpu = O.run(sc, g, src, 2 * n, seed=SEED, flags=abi.FLAG_PATHLENGTH)
    assert 0 < taken <= cpu.counter("grid_updates")
    np.testing.assert_allclose(jm.cpu().numpy().reshape(cpu.jmean.shape), cpu.jmean, rtol=RTOL, atol=1e-300)
    assert np.array_equal(ab.cpu().numpy().reshape(cpu.absorb.shape), cpu.absorb)
    c = ctr.cpu().numpy()
    got = {k: int(c[abi.CTR[k]]) for k in abi.COUNTER_NAMES if k not in abi.ENGINE_COUNTERS}
    assert got == cpu.counters_dict()
