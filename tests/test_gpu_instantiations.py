"""Every transport-kernel instantiation, jmean deposit regime and axis-length edge against the
oracle, on the GPU.

tests/plan_cases.py lists the cases: one per compiled transport_kernel / ws_kernel (45), the
photon counts of one lane and one lane past a wave, the deposit regimes at the tile counts
where one hands over to the next, each axis on both sides of the lean path's cell-packing
bound, and grids with axes of 1, 2 and 3 voxels. The device-free plan (tests/planprobe.py) says
which kernel and regime a case selects; the run must launch that kernel family and equal the
oracle under test_gpu_parity.compare: counters, photon records, absorb and emission bit for
bit, jmean at 1e-12.
"""
import time

import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi
from rsmcrt_amd.engine import Engine
from tests import plan_cases, planprobe
from tests.test_gpu_parity import SEED, compare

pytestmark = pytest.mark.gpu

_oracle_runs = {}


def oracle(case):
    """The oracle's run of a case. The small cases that differ only in knobs (segment slots,
    SMCRT_LEAN) share one run, which nothing modifies; the large grids are run where needed."""
    sc, g, src = case.scene(), case.scene_grid(), case.source()
    if case.group in ("deposit", "axis-bound"):
        return O.run(sc, g, src, case.n, seed=SEED, flags=case.flags, records=True)
    key = (case.make_scene.__name__, case.grid, case.make_source.__name__, case.n, case.flags)
    if key not in _oracle_runs:
        _oracle_runs[key] = O.run(sc, g, src, case.n, seed=SEED, flags=case.flags, records=True)
    return _oracle_runs[key]


def check_inputs(case, cpu):
    """What a case needs of its inputs to test what it is there for (conditions on the oracle's
    run, not tolerances)."""
    assert cpu.counter("photons") == case.n and cpu.counter("faults") == 0
    if case.kernel[0] == "ws_kernel" and case.plan["xf"]:
        assert cpu.counter("fresnel") > 0 and cpu.counter("reflections") > 0  # (the XF program points ran)
    if case.group == "deposit":  # every tile, the first and the last, receives deposits
        flat = cpu.jmean.ravel()
        touched = np.maximum.reduceat(flat, np.arange(0, flat.size, plan_cases.TILE_VOXELS)) > 0.0
        assert touched.size == plan_cases.tiles_of(case.grid) and touched.all(), np.flatnonzero(~touched)
        assert cpu.counter("deposits") > 5e6
    if case.group == "axis-bound":  # the packed cell index of the long axis uses its top bit
        assert cpu.records["cell"][:, case.axis].max() > 1 << 19
        assert cpu.counter("deposits") > 5e6


@pytest.mark.parametrize("case", plan_cases.CASES, ids=[c.id for c in plan_cases.CASES])
def test_case(case, monkeypatch):
    """One case of tests/plan_cases.py: the plan it states, the kernel family the plan implies
    (lean_launches), no lean hazard, and the oracle's photons and tallies.

    Measured on an MI355X no case takes 5 s: the slowest are the axis-*-at-limit cases (2.5-2.8 s,
    2.3-2.6 s of it transport_kernel walking 2^20 voxels per segment in one lane),
    dep-sorted-4096 (2.6 s) and dep-atomics-4112 (2.5 s; 67 M voxels: engine 1.3-1.5 s, oracle
    0.35 s, compare 0.75 s); the other deposit cases take 1.6-1.9 s, everything else under 1 s."""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    sc, g, src = case.scene(), case.scene_grid(), case.source()
    plan = planprobe.plan(sc, g, env=case.env)
    assert plan["status"] == abi.OK, plan["error"]
    assert plan_cases.plan_fields(plan) == case.plan
    assert plan_cases.kernel_of(plan, case.xsrc, case.flags) == case.kernel
    assert plan_cases.regime_of(plan) == case.regime
    t0 = time.perf_counter()
    with Engine(sc, g) as eng:
        eng.kernel_times()
        gpu = eng.run(src, case.n, seed=SEED, flags=case.flags, records=True)
        kt = eng.kernel_times()
    t1 = time.perf_counter()
    assert (kt["lean_launches"] > 0) == case.lean, (plan, kt)
    if case.lean:
        assert kt["lean_hazards"] == 0, kt
    cpu = oracle(case)
    t2 = time.perf_counter()
    check_inputs(case, cpu)
    compare(gpu, cpu)
    t3 = time.perf_counter()
    print(f"{case.id}: engine {t1 - t0:.2f} s, oracle {t2 - t1:.2f} s, compare {t3 - t2:.2f} s")
