"""Displacement expressions (smcrt.h SMCRT_DISP_EXPR) on the GPU, against the unchanged oracle.

The oracle knows only the built-in sine and the primitives, so every scene here has a twin
the oracle understands whose SDF values are the same bit for bit: the sine product written as an
expression (the same operations in the same order, tests/test_displacement_expr.py), and
formula-defined SDFs (scene.implicit: a zero-normal plane, whose d is +-0, displaced by the
formula) that restate a primitive's own arithmetic (geometry.h sdf_shape_s). Each GPU run must
equal the oracle's run of the twin under test_gpu_parity.compare: counters, photon records,
absorb and emission bit for bit, jmean at 1e-12. A few thousand photons on the 32^3 grid of
tests/geom_cases.py; each test takes a few seconds at most.
"""
import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, scene
from rsmcrt_amd.engine import Engine
from rsmcrt_amd.scene import Scene
from tests import geom_cases
from tests.geom_cases import SUBJECT, lattice, medium, place
from tests.test_displacement_expr import sine_expr, with_expressions
from tests.test_geometry_matrix import check_inputs, oracle
from tests.test_gpu_parity import SEED, compare

pytestmark = pytest.mark.gpu


def run(sc, case):
    with Engine(sc, case.scene_grid()) as eng:
        eng.kernel_times()
        gpu = eng.run(case.source(), case.n, seed=SEED, flags=case.flags, records=True)
        return gpu, eng.kernel_times()


@pytest.mark.parametrize("path", ["serial", "global", "culled"])
def test_sine_by_expression_on_every_nested_eval_path(path, monkeypatch):
    """The scenes of mod-displacement-serial / -global / -culled with displacement_sine replaced
    by the equivalent expression: the run equals the oracle's run of the sine scene."""
    case = geom_cases.BY_ID[f"mod-displacement-{path}"]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    sc = with_expressions(case.scene())
    gpu, kt = run(sc, case)
    assert kt["lean_launches"] == 0, kt
    cpu = oracle(case)
    check_inputs(case, cpu)
    compare(gpu, cpu)


def _translation(nd):
    """A translate-only node's p = pos + t as three sub-expressions."""
    t = nd.transform
    assert [t[k] for k in (0, 1, 2, 4, 5, 6, 8, 9, 10)] == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    return f"(x+{t[3]!r})", f"(y+{t[7]!r})", f"(z+{t[11]!r})"


def sphere_formula(nd):  # geometry.h SMCRT_SDF_SPHERE
    X, Y, Z = _translation(nd)
    return f"sqrt({X}*{X}+{Y}*{Y}+{Z}*{Z}) - {nd.param[0]!r}"


def torus_formula(nd):  # geometry.h SMCRT_SDF_TORUS: q = (len(p.x, 0, p.z) - R, p.y, 0); len(q) - r
    X, Y, Z = _translation(nd)
    A = f"(sqrt({X}*{X}+0*0+{Z}*{Z})-{nd.param[0]!r})"
    return f"sqrt({A}*{A}+{Y}*{Y}+0*0) - {nd.param[1]!r}"


@pytest.mark.parametrize("kind,formula,size", [(abi.SDF_SPHERE, sphere_formula, 26), (abi.SDF_TORUS, torus_formula, 60)],
                         ids=["sphere", "torus"])
def test_formula_defined_sdf_equals_the_primitive(kind, formula, size):
    """scene.implicit of a primitive's own formula against the oracle's run of the primitive
    scene (prim_scene(kind, 1): one translate-only copy and the medium box). The torus program
    is near the size limit."""
    case = geom_cases.BY_ID[f"{geom_cases.PRIMITIVES[kind]}-serial"]
    prim = case.scene()
    nd = prim.nodes[prim.top[0]]
    assert nd.kind == kind
    sub = scene.implicit(formula(nd), SUBJECT, 1)
    assert sub.param[1] == size
    sc = Scene([sub, medium(2)])
    gpu, kt = run(sc, case)
    assert kt["lean_launches"] == 0, kt
    cpu = oracle(case)
    check_inputs(case, cpu)
    compare(gpu, cpu)


def _three_tops(as_expressions):
    c = lattice()
    sph = scene.sphere(0.17, SUBJECT, 1, place(c[0], 0, False))
    bx = scene.box((0.3, 0.24, 0.36), SUBJECT, 2, place(c[1], 1, True))
    cp = scene.capsule((-0.1, -0.02, 0.0), (0.1, 0.05, 0.04), 0.1, SUBJECT, 3, place(c[2], 2, False))
    a1, f1, a2, f2 = 0.02, (9.0, 7.0, 5.0), 0.015, (11.0, 6.0, 8.0)
    if as_expressions:
        nd = sph.node()
        tops = [scene.implicit(sphere_formula(nd), SUBJECT, 1), scene.displacement(bx, sine_expr(a1, *f1)),
                scene.displacement_sine(cp, a2, f2)]
    else:
        tops = [sph, scene.displacement_sine(bx, a1, f1), scene.displacement_sine(cp, a2, f2)]
    return Scene(tops + [medium(4)])


def test_several_programs_in_one_scene():
    """An implicit sphere, a sine-by-expression box and a built-in-sine capsule: two different
    programs and the built-in side by side must not alias."""
    case = geom_cases.BY_ID["mod-displacement-serial"]  # (its grid, source, n and flags)
    sc = _three_tops(True)
    progs = [bytes(n)[abi.SdfNode.transform.offset:abi.SdfNode.k.offset] for n in sc.nodes
             if n.kind == abi.SDF_DISPLACEMENT and n.param[0] == abi.DISP_EXPR]
    assert len(progs) == 2 and progs[0] != progs[1]
    gpu, kt = run(sc, case)
    assert kt["lean_launches"] == 0, kt
    cpu = O.run(_three_tops(False), case.scene_grid(), case.source(), case.n, seed=SEED, flags=case.flags, records=True)
    assert cpu.counter("photons") == case.n and cpu.counter("faults") == 0
    assert cpu.counter("fresnel") >= 50 and cpu.counter("reflections") >= 10
    compare(gpu, cpu)


def test_classify_with_an_expression():
    """Engine.classify of 4096 points within 0.08 of a displaced box's surface: the layer is
    predicted from the oracle's value of the undisplaced box plus smcrt_displacement_eval's
    f, added in numpy (the same d + f), and every point must agree."""
    expr = "0.04*cos(11*x)*min(abs(y),0.3) - 0.02*floor(3*z)"
    bx = scene.box((0.48, 0.36, 0.6), SUBJECT, 1, place((0.1, -0.05, 0.2), 0, False))
    mod = scene.displacement(bx, expr)
    sc = Scene([mod, medium(2)])
    plain = Scene([bx, medium(2)])
    rng = np.random.Generator(np.random.Philox(4096))
    cand = rng.uniform(-0.6, 0.8, size=(100000, 3))
    ds0 = O.sdf_eval(plain, cand, which=0) + scene.displacement_eval(mod, cand)
    near = np.flatnonzero(np.abs(ds0) < 0.08)[:4096]
    assert len(near) == 4096
    pts, ds0 = cand[near], ds0[near]
    ds1 = O.sdf_eval(plain, pts, which=1)
    assert (ds1 < 0.0).all()  # inside the medium box
    want = np.where((ds0 < 0.0) & (ds0 >= ds1), 1, 2).astype(np.int32)  # maxloc(ds, mask = ds < 0)
    with Engine(sc, scene.grid(32, 32, 32, 1.0, 1.0, 1.0)) as eng:
        lay, _ = eng.classify(pts)
    assert np.array_equal(lay, want), int((lay != want).sum())
    assert 1000 < int((want == 1).sum()) < 3096
