"""Displacement expressions (smcrt.h SMCRT_DISP_EXPR) without a GPU: the compiler, the host run
of the interpreter the kernels use (smcrt_displacement_eval), describe, the limits, and the
check smcrt_scene_create makes of a stored program before any device call.

Values are compared with ==, never with a tolerance: + - * / sqrt floor abs min max are
exactly rounded (or exact) fp64 operations that numpy performs too, in the order written; sin
and cos are the engine's own, which the oracle restates (pyoracle.sincos, valid on [0, 4 pi]).
"""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, engine, scene
from rsmcrt_amd.scene import Modifier, Scene
from tests import geom_cases, planprobe

N_POINTS = 1000
CODE_OFFSET = abi.SdfNode.param.offset + 3 * 8  # param[3..10]: the 64 code bytes


@pytest.fixture(autouse=True)
def _library(lib_path):
    engine.load_library(lib_path)


def points():
    return np.random.Generator(np.random.Philox(20251019)).uniform(-1.0, 1.0, (N_POINTS, 3))


def child():
    return scene.sphere(0.3, geom_cases.SUBJECT, 1)


def evaluate(expr, pts):
    return scene.displacement_eval(scene.displacement(child(), expr), pts)


def dmin(a, b):  # geometry.h dmin / dmax
    return np.where(a < b, a, b)


def dmax(a, b):
    return np.where(a > b, a, b)


EXACT = [  # expression, the same formula in numpy fp64
    ("x + y * z - x / y", lambda x, y, z: x + y * z - x / y),
    ("x * y + z", lambda x, y, z: x * y + z),
    ("x - y - z", lambda x, y, z: (x - y) - z),
    ("x / y / z", lambda x, y, z: (x / y) / z),
    ("x - (y - z)", lambda x, y, z: x - (y - z)),
    ("x / (y / z)", lambda x, y, z: x / (y / z)),
    ("-x*y", lambda x, y, z: -x * y),
    ("2*-x", lambda x, y, z: 2 * -x),
    ("- -x - -2.5", lambda x, y, z: x - -2.5),
    ("((x + y) * (z - (x * (y + 2)))) / ((x - 3) * (y + (z - 4)))",
     lambda x, y, z: ((x + y) * (z - (x * (y + 2)))) / ((x - 3) * (y + (z - 4)))),
    ("1e-3 * x + .5 - 2.5E+1 * y", lambda x, y, z: 1e-3 * x + .5 - 2.5E+1 * y),
    ("pi * x + y / pi", lambda x, y, z: np.pi * x + y / np.pi),
    ("abs(x) + sqrt(abs(y)) * floor(3*z)", lambda x, y, z: np.abs(x) + np.sqrt(np.abs(y)) * np.floor(3 * z)),
    ("sqrt(x*x + y*y + z*z) - 0.3", lambda x, y, z: np.sqrt(x * x + y * y + z * z) - 0.3),
    ("min(x, y) - max(y, z) * min(max(x, -0.25), 0.25)",
     lambda x, y, z: dmin(x, y) - dmax(y, z) * dmin(dmax(x, -0.25), 0.25)),
    ("floor(x / 1e-3) * 1e-3 + floor(-y)", lambda x, y, z: np.floor(x / 1e-3) * 1e-3 + np.floor(-y)),
    (" x\t+\n( y ) ", lambda x, y, z: x + y),
]
TRIG = ["sin(12.5*x)", "cos(12.5*y)", "0.5*sin(3*x + 4*y - 5*z)*cos(pi*z)", "((0.03*sin(9.0*x))*sin(7.0*y))*sin(5.0*z)"]


@pytest.mark.parametrize("expr,formula", EXACT, ids=[e for e, _ in EXACT])
def test_exactly_rounded_operations(expr, formula):
    pts = points()
    got = evaluate(expr, pts)
    want = formula(pts[:, 0], pts[:, 1], pts[:, 2])
    assert np.isfinite(want).all()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]


def oracle_sin(t):
    """sin(t) for |t| <= 4 pi from the oracle's sincos on [0, 4 pi]: sin(-t) = -sin(t)."""
    assert np.abs(t).max() <= 4.0 * np.pi
    return np.array([-O.sincos(-v)[0] if v < 0.0 else O.sincos(v)[0] for v in t])


def oracle_cos(t):
    assert np.abs(t).max() <= 4.0 * np.pi
    return np.array([O.sincos(abs(v))[1] for v in t])


def test_sin_and_cos_are_the_oracles():
    pts = points()
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    for k in (12.5, 1.0, 1e-3):  # |k x| up to 12.5 < 4 pi
        assert np.array_equal(evaluate(f"sin({k!r}*x)", pts), oracle_sin(k * x)), k
        assert np.array_equal(evaluate(f"cos({k!r}*y)", pts), oracle_cos(k * y)), k
    assert np.array_equal(evaluate("0.5*sin(3*x + 4*y - 5*z)*cos(pi*z)", pts),
                          0.5 * oracle_sin(3 * x + 4 * y - 5 * z) * oracle_cos(np.pi * z))


def sine_expr(a, fx, fy, fz):
    """The built-in SMCRT_DISP_SINE (geometry.h modifier_value) as an expression."""
    return f"(({a!r}*sin({fx!r}*x))*sin({fy!r}*y))*sin({fz!r}*z)"


def test_sine_product_from_oracle_values():
    pts = points()
    a, fx, fy, fz = 0.1 * 0.3, 9.0, 7.0, 5.0
    want = ((a * oracle_sin(fx * pts[:, 0])) * oracle_sin(fy * pts[:, 1])) * oracle_sin(fz * pts[:, 2])
    assert np.array_equal(evaluate(sine_expr(a, fx, fy, fz), pts), want)
    # and d + f is what the oracle's built-in displacement adds to its child
    sine = Scene([scene.displacement_sine(child(), a, (fx, fy, fz))])
    assert np.array_equal(O.sdf_eval(sine, pts), O.sdf_eval(Scene([child()]), pts) + want)


@pytest.mark.parametrize("expr", [e for e, _ in EXACT] + TRIG)
def test_describe_round_trip(expr):
    m = scene.displacement(child(), expr)
    text = scene.displacement_describe(m)
    again = scene.displacement(child(), text)
    assert again.words == m.words, text
    assert scene.displacement_describe(again) == text


def test_node_words_and_encoding():
    """The node is self-contained: what Scene writes is what smcrt_displacement_compile made,
    in the fields smcrt.h documents, and no double of it is a NaN or an infinity."""
    m = scene.displacement(child(), "0.25*x - min(y, -1.5)*pi")
    sc = Scene([m, geom_cases.medium(2)])
    nd = sc.node_array()[sc.top[0]]
    assert nd.kind == abi.SDF_DISPLACEMENT and nd.param[0] == abi.DISP_EXPR == 2
    assert nd.n_children == 1 and nd.layer == 1 and nd.mus == geom_cases.SUBJECT.mus
    assert (nd.param[1], nd.param[2]) == (9.0, 3.0)
    assert list(nd.transform)[:3] == [0.25, -1.5, np.pi] and not any(list(nd.transform)[3:])
    code = bytes((C.c_ubyte * 64).from_address(C.addressof(nd) + CODE_OFFSET))
    assert list(code[:9]) == [16, 1, 6, 2, 17, 8, 18, 6, 5] and not any(code[9:])  # c0 x * y c1 min c2 * -
    assert nd.param[11] == 0.0
    assert np.isfinite(np.array(list(nd.transform) + list(nd.param))).all()


def compile_status(expr):
    L = engine.load_library()
    nd = abi.SdfNode()
    nd.layer = 77
    st = L.smcrt_displacement_compile(expr.encode(), C.byref(nd))
    return st, L.smcrt_last_error().decode(), nd


INSTR_64 = "-x" + "+x" * 31                   # 32 pushes, one negation, 31 additions
INSTR_65 = "x" + "+x" * 32                    # 33 pushes, 32 additions
CONSTS_12 = "+".join(f"{i}.5" for i in range(12))
CONSTS_13 = "+".join(f"{i}.5" for i in range(13))
DEPTH_8 = "x+(x+(x+(x+(x+(x+(x+x))))))"
DEPTH_9 = "x+(x+(x+(x+(x+(x+(x+(x+x)))))))"


@pytest.mark.parametrize("expr,column", [("", 1), ("x +", 4), ("foo(x)", 1), ("min(x)", 6), ("(x + y", 7), ("x + y)", 6),
                                         ("sin(x, y)", 6), ("x y", 3), ("2 * pow(x, 2)", 5), ("1e999", 1),
                                         (INSTR_65, None), (CONSTS_13, None), (DEPTH_9, None)],
                         ids=["empty", "dangling-operator", "unknown-function", "min-one-argument", "unclosed", "unopened",
                              "sin-two-arguments", "juxtaposed", "pow", "infinite-literal", "65-instructions",
                              "13-constants", "stack-9"])
def test_rejections(expr, column):
    st, msg, nd = compile_status(expr)
    assert st == abi.ERR_INVALID_ARG, (st, msg)
    found = re.search(r"column (\d+)", msg)
    assert found, msg
    assert 1 <= int(found.group(1)) <= len(expr) + 1
    if column is not None:
        assert int(found.group(1)) == column, msg
    assert nd.kind == 0 and nd.layer == 77  # the node is untouched
    with pytest.raises(ValueError, match=r"column \d+"):
        scene.displacement(child(), expr)


def test_limits_are_reached():
    """64 instructions, 12 distinct constants and 8 stack values compile and evaluate."""
    pts = points()
    x = pts[:, 0]
    st, msg, nd = compile_status(INSTR_64)
    assert st == abi.OK and nd.param[1] == 64.0 and nd.layer == 77, msg
    want = -x
    for _ in range(31):
        want = want + x
    assert np.array_equal(evaluate(INSTR_64, pts), want)
    st, msg, nd = compile_status(CONSTS_12)
    assert st == abi.OK and nd.param[2] == 12.0, msg
    assert evaluate(CONSTS_12, pts[:1])[0] == sum(i + 0.5 for i in range(12))
    assert compile_status("+".join(["1.5"] * 20) + "+" + CONSTS_12[4:])[0] == abi.OK  # repeated constants share a slot
    want = x
    for _ in range(7):
        want = x + want
    assert np.array_equal(evaluate(DEPTH_8, pts), want)


def _create(nodes, sc, g):
    L = engine.load_library()
    h = C.c_void_p()
    st = L.smcrt_scene_create(nodes, len(sc.nodes), sc.top_array(), sc.n_top, C.byref(g), None, 0, 0, C.byref(h))
    msg = L.smcrt_last_error()
    if st == abi.OK:
        L.smcrt_scene_destroy(h)
    return st, msg


def test_stored_program_is_verified_before_the_device():
    """smcrt_scene_create re-verifies the words of a displacement node: a hand-corrupted program
    is INVALID_ARG before any device call (so this needs no GPU); the intact node is accepted."""
    sc = Scene([scene.displacement(child(), "0.02*sin(9*x)"), geom_cases.medium(2)])  # c0 c1 x * sin *
    g = scene.grid(8, 8, 8, 1, 1, 1)
    assert _create(sc.node_array(), sc, g)[0] in (abi.OK, abi.ERR_NO_DEVICE)

    def corrupted(change):
        nodes = sc.node_array()
        nd = nodes[sc.top[0]]
        change(nd, (C.c_ubyte * 64).from_address(C.addressof(nd) + CODE_OFFSET))
        return nodes

    def setp(i, v):
        return lambda nd, code: nd.param.__setitem__(i, v)

    def setc(i, v):
        return lambda nd, code: code.__setitem__(i, v)

    cases = {"bad opcode": setc(2, 63), "opcode past the constants' range": setc(2, 28), "opcode 255": setc(0, 255),
             "length past the node": setp(1, 65.0), "huge length": setp(1, 1e9), "zero length": setp(1, 0.0),
             "fractional length": setp(1, 7.5), "NaN length": setp(1, float("nan")),
             "length short of the code": setp(1, 5.0), "length beyond the code": setp(1, 7.0),
             "constant index out of range": setc(0, 16 + 2), "constant count past the node": setp(2, 13.0),
             "stack underflow": setc(0, 4), "two values left": setc(5, 1)}
    for name, change in cases.items():
        nodes = corrupted(change)
        st, msg = _create(nodes, sc, g)
        assert st == abi.ERR_INVALID_ARG, (name, st, msg)
        assert b"displacement node 0" in msg, (name, msg)
        p = planprobe.plan(sc, g, nodes=nodes)  # the same answer from the device-free plan
        assert p["status"] == abi.ERR_INVALID_ARG, (name, p)
    # an unknown function number is still rejected
    assert _create(corrupted(setp(0, 3.0)), sc, g)[0] == abi.ERR_INVALID_ARG


def with_expressions(sc):
    """`sc` with every built-in sine displacement replaced by the equivalent expression."""
    def conv(s):
        if isinstance(s, Modifier) and s.kind == abi.SDF_DISPLACEMENT and s.param[0] == abi.DISP_SINE:
            return scene.displacement(s.child, sine_expr(*s.param[1:5]))
        return s
    out = Scene([conv(s) for s in sc.sdfs])
    assert [n.kind for n in out.nodes] == [n.kind for n in sc.nodes] and out.top == sc.top
    assert sum(n.kind == abi.SDF_DISPLACEMENT and n.param[0] == abi.DISP_EXPR for n in out.nodes) >= 1
    return out


@pytest.mark.parametrize("copies,path", [(1, "serial"), (11, "global"), (3, "culled")])
def test_plan_is_the_sine_scenes(copies, path):
    case = geom_cases.BY_ID[f"mod-displacement-{path}"]
    sine = geom_cases.modifier_scene(abi.SDF_DISPLACEMENT, copies)
    g = case.scene_grid()
    want = planprobe.plan(sine, g, env=case.env)
    got = planprobe.plan(with_expressions(sine), g, env=case.env)
    assert want["status"] == got["status"] == abi.OK, (want["error"], got["error"])
    assert geom_cases.plan_fields(got) == geom_cases.plan_fields(want) == case.plan


def test_pickle_and_node_bytes():
    import pickle
    m = scene.implicit("sqrt(x*x + y*y + z*z) - 0.25", geom_cases.SUBJECT, 3)
    again = pickle.loads(pickle.dumps(m))
    assert bytes(Scene([again]).node_array()) == bytes(Scene([m]).node_array())
    pts = points()
    want = np.sqrt(pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1] + pts[:, 2] * pts[:, 2]) - 0.25
    # the zero-normal plane's d is +-0, so the oracle-free host value of the top is f itself
    assert np.array_equal(scene.displacement_eval(again, pts), want)
