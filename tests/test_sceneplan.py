"""The device-free scene plan (rsmcrt_amd/csrc/sceneplan.h), observed without a GPU.

tests/sceneplan_probe.cpp calls the library's own read_knobs() and plan_scene() and prints the
plan (tests/planprobe.py builds and runs it). The expected values follow from the rules in
sceneplan.cpp: which kernel instantiation, deposition path and limits a scene gets, what each
SMCRT_* knob changes, and the validation errors with their texts.
"""
import glob
import os
import re

import numpy as np
import pytest

import bench
from rsmcrt_amd import abi, builders, scene
from tests import plan_cases, planprobe
from tests.test_abi import _nested
from tests.test_far_bound import fm_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GiB = 1 << 30


def sphere():
    return builders.setup_sphere(10.0, 0.1, 0.9, 1.0, 1.0), scene.grid(48, 48, 48, 1, 1, 1)


def skin():
    dets = [scene.circle_dect((0.0, 0.0, 0.0499), (0.0, 0.0, 1.0), 1, 0.05, 50),
            scene.annulus_dect((0.0, 0.0, 0.0499), (0.0, 0.0, 1.0), 1, 0.005, 0.02, 25)]
    return builders.skin_layers(), scene.grid(50, 50, 50, 0.05, 0.05, 0.05), dets


def spheres(n_tops):
    return builders.setup_sphere_scene(builders.random_sphere_list(n_tops - 1)), scene.grid(32, 32, 32, 1, 1, 1)


@pytest.fixture(scope="module")
def m2():
    sc, g, _, _, _, _ = bench.workload("m2", 32)
    return sc, g, planprobe.plan(sc, g)


def test_one_sphere_takes_the_lean_path():
    sc, g = sphere()
    p = planprobe.plan(sc, g)
    assert p["status"] == abi.OK
    assert (p["grid_mode"], p["coop_lanes"], p["nested"], p["lean_candidate"], p["ws_slots"]) == (1, 0, 0, 1, 3)
    assert p["bucketed"] == 1 and p["n_tiles"] == 7 and p["lds_faces"] == 1 and p["fresnel"] == 0
    assert p["inv2"] == [0.5, 0.5, 0.5] and p["fm_err"] == 0.0
    assert p["n_prog"] == 2 and p["prog_size"] == 2 + 3
    assert planprobe.plan(sc, g, env={"SMCRT_LEAN": "0"})["lean_candidate"] == 0
    assert planprobe.plan(sc, g, env={"SMCRT_WS_SLOTS": "2"})["ws_slots"] == 2
    q = planprobe.plan(sc, g, env={"SMCRT_DEBUG_LEAN_MARGIN": "all", "SMCRT_POOL_CAP": "100000"})
    assert q["lean_debug"] == 2 and q["pool_cap_chunks"] == 100000 // 16384


def test_grid_modes():
    sc, _ = sphere()
    p = planprobe.plan(sc, scene.grid(128, 128, 128, 1, 1, 1))
    assert p["grid_mode"] == 2 and p["fe"] == [-6, -6, -6]  # a face is k * 2/128
    assert planprobe.plan(sc, scene.grid(48, 48, 48, 0.05, 0.05, 0.05))["grid_mode"] == 0


def test_detector_scenes_are_lean_only_when_forced():
    sc, g, dets = skin()
    p = planprobe.plan(sc, g, dets)
    assert p["lean_candidate"] == 0 and p["fresnel"] == 1
    assert planprobe.plan(sc, g, dets, env={"SMCRT_LEAN": "1"})["lean_candidate"] == 1
    sizes = scene.det_sizes(dets)
    assert p["det_total"] == sum(sizes) and p["h_det_off"] == [0, sizes[0], sum(sizes)]
    cam = scene.camera((-0.05, -0.05, 0.0499), (0.05, -0.05, 0.0499), (-0.05, 0.05, 0.0499), 1, 4, 100.0)
    p = planprobe.plan(sc, g, dets + [cam])
    assert scene.det_sizes([cam]) == [cam.nbins ** 2]  # a camera owns nbins x nbins doubles
    assert p["det_total"] == sum(sizes) + cam.nbins ** 2 and p["h_det_off"][-2:] == [sum(sizes), p["det_total"]]


def test_coop_threshold():
    assert planprobe.plan(*spheres(7))["coop_lanes"] == 0
    assert planprobe.plan(*spheres(8))["coop_lanes"] == 2
    assert planprobe.plan(*spheres(8), env={"SMCRT_COOP_MIN_TOPS": "9"})["coop_lanes"] == 0
    assert planprobe.plan(*spheres(8), env={"SMCRT_COOP_LANES": "5"})["coop_lanes"] == 5


def test_m2_plan_and_its_knobs(m2):
    sc, g, p = m2
    assert sc.n_top == 41
    assert (p["coop_lanes"], p["ctab"], p["cull"], p["lean_candidate"]) == (10, 1, 1, 0)
    assert p["fm_err"] > 0.0
    assert planprobe.plan(sc, g, env={"SMCRT_COOP_TAB": "0"})["ctab"] == 0
    assert planprobe.plan(sc, g, env={"SMCRT_CULL": "0"})["cull"] == 0
    q = planprobe.plan(sc, g, env={"SMCRT_FAR_MARCH": "0"})
    assert q["fm_err"] == 0.0 and q["fm_step"] == 0.0


@pytest.mark.parametrize("workload", ["m2", "m4"])
def test_far_march_bounds_are_the_ones_test_far_bound_checks(workload, m2):
    """fm_err and fm_step of the host, bit for bit, against tests/test_far_bound.py::fm_bounds,
    the restatement whose slack that test measures."""
    if workload == "m2":
        sc, g, p = m2
    else:
        sc, g, _, _, _, _ = bench.workload("m4", 32)
        p = planprobe.plan(sc, g)
    fm_err, fm_step = fm_bounds(sc, g)
    assert p["fm_err"] == float(fm_err) and p["fm_step"] == float(fm_step)
    assert p["fm_err"] > 0.0


def test_deposit_paths():
    sc, g = sphere()
    assert planprobe.plan(sc, g, env={"SMCRT_DEPOSIT": "sorted"})["bucketed"] == 0
    p = planprobe.plan(sc, g, env={"SMCRT_FUSED_HIST": "0"})
    assert p["bucketed"] == 0 and p["hist_tiles"] == 0 and p["lean_candidate"] == 0
    p = planprobe.plan(sc, g, env={"SMCRT_DEPOSIT": "sorted"})
    assert p["hist_tiles"] == p["n_tiles"] == 7 and p["force_atomic"] == 0
    assert planprobe.plan(sc, g, env={"SMCRT_DEPOSIT": "atomic"})["force_atomic"] == 1
    # 264 * 256 * 256 voxels are 1056 tiles of 2^14: binned, but past the 1024 direct tiles
    p = planprobe.plan(sc, scene.grid(264, 256, 256, 1, 1, 1))
    assert p["n_tiles"] == 1056 and p["bucketed"] == 0 and p["lean_candidate"] == 0


def test_plan_table_covers_every_instantiation():
    """tests/plan_cases.py: its matrix is the 24 ws_kernel and 21 transport_kernel instantiations
    of kinst.hip, once each, beside the five deposit-regime sizes, the six axis-bound and the
    eight tiny-grid cases."""
    assert plan_cases.check_table() == {"ws_kernel": 24, "transport_kernel": 21, "deposit": 5, "axis-bound": 6,
                                        "tiny": 8}


@pytest.mark.parametrize("case", plan_cases.CASES, ids=[c.id for c in plan_cases.CASES])
def test_plan_table(case):
    """Every case of tests/plan_cases.py gets the plan it states, and with it the kernel
    instantiation and the deposit regime that tests/test_gpu_instantiations.py runs it for: a
    changed threshold (MAX_FACE_BYTES, the tile limits, the lean axis bound) fails here instead
    of leaving a kernel without its GPU case."""
    p = planprobe.plan(case.scene(), case.scene_grid(), env=case.env)
    assert p["status"] == abi.OK, p["error"]
    assert plan_cases.plan_fields(p) == case.plan
    assert plan_cases.kernel_of(p, case.xsrc, case.flags) == case.kernel
    assert plan_cases.regime_of(p) == case.regime
    assert p["n_tiles"] == (plan_cases.tiles_of(case.grid) if plan_cases.tiles_of(case.grid) <= 4096 else 0)


def _check_choices(sc, g, p, dets=(), env=None, kind="sdf"):
    """The probe's launch choice against plan_cases.choice_of for both values of xsrc and every
    run state of plan_cases.RUN_STATES, and the grid keys: equal exactly where the restatement
    says two launches share a grid."""
    # (the library's lean_ok is the plan's lean_candidate, unless the lane-scratch allocation failed: "no-lean")
    states = [(x, st[1], st[2] and p["lean_candidate"]) + st[3:] for x in (0, 1) for st in plan_cases.RUN_STATES]
    got = planprobe.choices(sc, g, states, dets, env, kind)
    want = [plan_cases.choice_of(p, x, fl, dets, lean_ok, paths, phasor, n_scr, kind, env)
            for x, fl, lean_ok, paths, phasor, n_scr in states]
    for st, c, w in zip(states, got, want):
        assert {k: v for k, v in c.items() if k != "grid_key"} == {k: v for k, v in w.items() if k != "grid"}, st
    for i in range(len(states)):
        for j in range(i):
            assert (got[i]["grid_key"] == got[j]["grid_key"]) == (want[i]["grid"] == want[j]["grid"]), (states[i], states[j])
    return got


@pytest.mark.parametrize("case", plan_cases.CASES, ids=[c.id for c in plan_cases.CASES])
def test_launch_choice_table(case):
    """sceneplan.h launch_choice, which the occupancy query and the launch both read, against the
    independent restatement of tests/plan_cases.py for every case of the table."""
    sc, g = case.scene(), case.scene_grid()
    p = planprobe.plan(sc, g, env=case.env)
    got = _check_choices(sc, g, p, env=case.env)
    plain = got[[case.xsrc == x and st[0] == "plain" for x in (0, 1) for st in plan_cases.RUN_STATES].index(True)]
    assert (plain["family"] == "ws_kernel") == case.lean


@pytest.mark.parametrize("kind", ["voxel", "mesh"])
@pytest.mark.parametrize("gm", [2, 1, 0])
def test_launch_choice_voxel_and_mesh(kind, gm):
    case = plan_cases.BY_ID[f"ws-F1-G{gm}-xf0-s3"]
    sc, g = case.scene(), case.scene_grid()
    p = planprobe.plan(sc, g)
    assert p["grid_mode"] == gm
    got = _check_choices(sc, g, p, kind=kind)
    assert {c["family"] for c in got} == {kind + "_kernel"} and {c["grid_key"] for c in got} == {0, 1}


def test_launch_choice_with_detectors_and_the_invoxel_knob():
    """Detectors make a scene XF and give transport_kernel its start-point rows; SMCRT_WS_INVOXEL
    overrides the in-voxel coordinate either way."""
    sc, g, dets = skin()
    for env in ({}, {"SMCRT_LEAN": "1"}, {"SMCRT_LEAN": "1", "SMCRT_WS_INVOXEL": "1"}):
        got = _check_choices(sc, g, planprobe.plan(sc, g, dets, env=env), dets, env)
        assert (got[0]["family"], got[0]["xf"], got[0]["iv"]) == (("ws_kernel", 1, int("SMCRT_WS_INVOXEL" in env))
                                                                  if env else ("transport_kernel", 0, 0))
    sc, g = sphere()
    for env, iv in (({}, 1), ({"SMCRT_WS_INVOXEL": "0"}, 0)):
        got = _check_choices(sc, g, planprobe.plan(sc, g, env=env), env=env)
        assert (got[0]["family"], got[0]["xf"], got[0]["iv"]) == ("ws_kernel", 0, iv)


def test_design_coverage_table_cites_the_cases():
    """DESIGN.md §3.3b names, for each instantiation and deposit regime, the test id that runs
    it: every matrix and deposit case of the table is cited there by its id."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        doc = f.read()
    cases = plan_cases.group("matrix") + plan_cases.group("deposit")
    missing = [c.id for c in cases if f"`test_case[{c.id}]`" not in doc]
    assert not missing, missing
    cited = set(re.findall(r"`test_case\[((?:ws|tr|dep)-[A-Za-z0-9-]+)\]`", doc))
    assert cited <= set(plan_cases.BY_ID), sorted(cited - set(plan_cases.BY_ID))


def test_nested_scenes_never_run_lean():
    p = planprobe.plan(_nested(3), scene.grid(8, 8, 8, 1, 1, 1))
    assert p["status"] == abi.OK and p["nested"] == 1 and p["lean_candidate"] == 0
    p = planprobe.plan(_nested(33), scene.grid(8, 8, 8, 1, 1, 1))
    assert p["status"] == abi.ERR_UNSUPPORTED and "nested" in p["error"]


def test_validation_errors_keep_their_texts():
    g = scene.grid(8, 8, 8, 1, 1, 1)
    sc = _nested(3)
    nodes = sc.node_array()
    i = next(k for k, nd in enumerate(nodes) if nd.kind == abi.SDF_MODEL)
    nodes[i].op = 99
    p = planprobe.plan(sc, g, nodes=nodes)
    assert (p["status"], p["error"]) == (abi.ERR_INVALID_ARG, f"model node {i}: bad CSG op")
    o = scene.mono(1.0, 0.1, 0.0, 1.0)
    sc = scene.Scene([scene.onion(scene.sphere(0.5, o, 1), 0.1), scene.box((2.0, 2.0, 2.0), o, 2)])
    nodes = sc.node_array()
    nodes[0].n_children = 2
    p = planprobe.plan(sc, g, nodes=nodes)
    assert (p["status"], p["error"]) == (abi.ERR_INVALID_ARG, "modifier node 0: needs exactly one child")
    sc, _ = sphere()
    p = planprobe.plan(sc, g, top=[0, len(sc.nodes)])
    assert (p["status"], p["error"]) == (abi.ERR_INVALID_ARG, "top index out of range")
    det = scene.circle_dect((0.0, 0.0, 0.5), (0.0, 0.0, 1.0), 1, 0.5, 10)
    det.nbins = 0
    p = planprobe.plan(sc, g, [det])
    assert (p["status"], p["error"]) == (abi.ERR_INVALID_ARG, "bad detector 0")


def test_slot_depth_rule():
    """sceneplan.h slot_depth: two slots for lean and far-march scenes, MAX_SLOTS (4) for other
    scenes while a slot's pool is at most the deep-slot size (24 GiB, or 60 % of the device's
    memory over four slots if that is more), two past it; SMCRT_SLOTS is clamped to 2 .. 4."""
    sd = planprobe.slot_depth
    assert sd(True, 1 * GiB, 288 * GiB) == 2
    assert sd(False, 1 * GiB, 288 * GiB) == 4
    assert sd(False, 24 * GiB, 0) == 4 and sd(False, 24 * GiB + 8, 0) == 2
    assert sd(False, 40 * GiB, 288 * GiB) == 4 and sd(False, 44 * GiB, 288 * GiB) == 2  # 0.6 * 288 / 4 = 43.2
    assert sd(False, 2 * GiB, 288 * GiB, env={"SMCRT_DEEP_SLOT_GIB": "1"}) == 2
    assert sd(False, 1 * GiB, 288 * GiB, env={"SMCRT_DEEP_SLOT_GIB": "1"}) == 4
    assert [sd(False, GiB, 0, env={"SMCRT_SLOTS": v}) for v in ("1", "2", "3", "4", "9")] == [2, 2, 3, 4, 4]
    assert sd(True, GiB, 0, env={"SMCRT_SLOTS": "4"}) == 4
    assert sd(False, 25 * GiB, 0, env={"SMCRT_SLOTS": "4"}) == 2


def test_every_knob_is_documented():
    """Every SMCRT_* name the engine passes to getenv is named in INTEGRATION.md."""
    names = set()
    for path in glob.glob(os.path.join(ROOT, "rsmcrt_amd", "csrc", "*")):
        with open(path, errors="replace") as f:
            names.update(re.findall(r'getenv\("(SMCRT_[A-Z_]+)"\)', f.read()))
    assert len(names) >= 27, sorted(names)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    missing = sorted(n for n in names if not re.search(r"\b" + n + r"\b", doc))
    assert not missing, missing
