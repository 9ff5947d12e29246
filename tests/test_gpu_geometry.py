"""Every SDF kind, CSG op and modifier on every path that evaluates the SDF array, against the
oracle, on the GPU.

tests/geom_cases.py lists the cases: the ten primitives through the lean path's serial fold,
transport_kernel's, the cooperative EVAL's LDS table and the culled EVAL; the culled EVAL's
straight-line groups, mixed lists, a reflection and a scaled top; the four CSG ops and the seven
modifiers as tops of 2-, 12- and 24-top scenes; transport_kernel's sphere/box pair branches in
every order and transform combination; and the far-field march with tori, segments, capsules
and boxes as far tops and with a sphere as the near top. The device-free plan
(tests/planprobe.py) says which path a case selects; the run must launch that kernel family
and equal the oracle under test_gpu_parity.compare: counters, photon records, absorb and
emission bit for bit, jmean at 1e-12. tests/test_geometry_matrix.py checks the table, the
plans and the inputs without a GPU.
"""
import time

import pytest

from rsmcrt_amd import abi
from rsmcrt_amd.engine import Engine
from tests import geom_cases, planprobe
from tests.test_geometry_matrix import check_inputs, oracle
from tests.test_gpu_parity import SEED, compare

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", geom_cases.CASES, ids=[c.id for c in geom_cases.CASES])
def test_case(case, monkeypatch):
    """One case of tests/geom_cases.py: the plan it states, the kernel family (lean_launches),
    no lean hazard, the far-field march's step count where the case is about it, and the oracle's
    photons and tallies.

    Measured on an MI355X the 104 cases take 10.3 s together; the slowest calls are sphere-lean
    (0.32 s, the first use of the device) and csg-union-global (0.20 s), the engine's share
    0.01 to 0.14 s per case."""
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    sc, g, src = case.scene(), case.scene_grid(), case.source()
    plan = planprobe.plan(sc, g, env=case.env)
    assert plan["status"] == abi.OK, plan["error"]
    assert geom_cases.plan_fields(plan) == case.plan
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
    if case.far == "on":
        assert kt["far_steps"] > 0, kt
    elif case.far == "off":
        assert kt["far_steps"] == 0, kt
    print(f"{case.id}: engine {t1 - t0:.2f} s, oracle {t2 - t1:.2f} s, compare {t3 - t2:.2f} s, "
          f"far_steps {kt['far_steps']}")
