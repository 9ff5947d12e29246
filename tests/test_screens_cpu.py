"""Field screens and the optical-path option (include/smcrt.h "field screens") without a GPU: the
header, abi.py and the Fortran module agree; the entry points are exported and refuse bad input
before any device call; smcrt_screen_hit, the text the kernel runs, against the rule restated
in numpy; output.write_screen."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rsmcrt_amd import abi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smcrt.h")
FORTRAN = os.path.join(ROOT, "bindings", "fortran", "smcrt_mod.f90")
FUNCTIONS = ["smcrt_scene_set_screens", "smcrt_scene_screen_info", "smcrt_scene_read_screens",
             "smcrt_scene_reset_screens", "smcrt_screen_hit"]
FIELDS = ["origin", "eu", "ev", "nu", "nv", "sides", "reserved"]


# ---- 1. exports, layout, Fortran text -------------------------------------------------------------
def test_exports_and_version(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for fn in FUNCTIONS:
        assert fn in exported, fn
        assert fn in abi.EXPORTED_SYMBOLS, fn
    from rsmcrt_amd import engine
    assert engine.load_library(lib_path).smcrt_abi_version() == 5  # (additive: the version stays)
    assert abi.PHASOR_OPTICAL_PATH == 1


def test_header_and_abi_agree(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("option %d\\n", (int)SMCRT_PHASOR_OPTICAL_PATH);',
             'printf("version %d\\n", (int)SMCRT_ABI_VERSION);',
             'printf("size %zu\\n", sizeof(smcrt_screen));',
             'printf("cfgsize %zu\\n", sizeof(smcrt_phasor_config));']
    lines += [f'printf("{f} %zu\\n", offsetof(smcrt_screen, {f}));' for f in FIELDS]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["option"]) == abi.PHASOR_OPTICAL_PATH == 1
    assert int(got["version"]) == abi.SMCRT_ABI_VERSION == 5
    assert int(got["size"]) == C.sizeof(abi.Screen) == 88
    assert int(got["cfgsize"]) == C.sizeof(abi.PhasorConfig) == 16
    assert [n for n, _ in abi.Screen._fields_] == FIELDS
    for f in FIELDS:
        assert int(got[f]) == getattr(abi.Screen, f).offset, f


def test_fortran_module_agrees():
    """bindings/fortran/smcrt_mod.f90 by text: the option's value, the bind(C) type field for
    field, an interface per entry point, and the module's ABI version unchanged."""
    low = re.sub(r"&\s*\n\s*", " ", open(FORTRAN).read().lower())
    assert re.search(r"smcrt_phasor_optical_path\s*=\s*1\b", low)
    assert re.search(r"smcrt_mod_abi_version\s*=\s*5\b", low)
    m = re.search(r"type,\s*bind\(c\)\s*::\s*smcrt_screen\b(.*?)end type smcrt_screen", low, re.S)
    assert m, "smcrt_screen is missing"
    decl = [l.split("!")[0].strip() for l in m.group(1).splitlines() if l.split("!")[0].strip()]
    # nine doubles in three vectors of 3, then four int32 (as the C struct and abi.Screen)
    assert len(decl) == 2 and decl[0].startswith("real(c_double)") and decl[1].startswith("integer(c_int32_t)")
    parts = [p.strip() for d in decl for p in re.split(r",(?![^()]*\))", d.split("::")[1])]
    names = [re.match(r"(\w+)", p).group(1) for p in parts]
    assert names == FIELDS
    assert all(re.match(r"\w+\(3\)", p) for p in parts[:3]) and not any("(" in p.split("=")[0] for p in parts[3:])
    for fn in FUNCTIONS:
        assert re.search(rf'function {fn}\(.*?\)\s*bind\(c,\s*name="{fn}"\)', low), fn
        assert f"end function {fn}" in low, fn


# ---- 2. refusals before the device ----------------------------------------------------------------
def good():
    return scene.screen((-0.5, -0.5, 0.25), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 4, 3)


def _bad_screens():
    out = []
    for field in ("origin", "eu", "ev"):
        for v in (float("nan"), float("inf"), -float("inf")):
            s = good()
            getattr(s, field)[1] = v
            out.append((f"{field} {v}", s))
    s = good(); s.eu[0] = 0.0; out.append(("eu zero", s))
    s = good(); s.ev[1] = 0.0; out.append(("ev zero", s))
    s = good(); s.ev[0] = 1e-9; out.append(("not orthogonal", s))
    s = good(); s.ev[0], s.ev[1] = 2.0, 0.0; out.append(("parallel edges", s))
    for f in ("nu", "nv"):
        for v in (0, -1, 4097):
            s = good(); setattr(s, f, v); out.append((f"{f} {v}", s))
    for v in (2, -2):
        s = good(); s.sides = v; out.append((f"sides {v}", s))
    s = good(); s.reserved = 1; out.append(("reserved", s))
    return out


def test_errors_before_the_device(lib_path):
    """Each invalid screen is INVALID_ARG naming its index, decided with a NULL scene, so before any
    device call; a valid list then fails only for the scene; the phasor configuration refuses
    unknown bits of `reserved` the same way."""
    from rsmcrt_amd import engine
    L = engine.load_library(lib_path)
    for what, bad in _bad_screens():
        for pos in (0, 2):  # the first offending screen is named
            arr = (abi.Screen * 3)(good(), good(), good())
            arr[pos] = bad
            assert L.smcrt_scene_set_screens(None, arr, 3) == abi.ERR_INVALID_ARG, what
            assert f"screen {pos}:".encode() in L.smcrt_last_error(), (what, L.smcrt_last_error())
    arr = (abi.Screen * 17)(*[good() for _ in range(17)])
    for n in (17, -1):
        assert L.smcrt_scene_set_screens(None, arr, n) == abi.ERR_INVALID_ARG
        assert b"screens" in L.smcrt_last_error() and b"NULL" not in L.smcrt_last_error()
    for n in (1, 16):  # valid lists: only the scene is wrong
        assert L.smcrt_scene_set_screens(None, arr, n) == abi.ERR_INVALID_ARG
        assert b"screen " not in L.smcrt_last_error() and b"NULL" in L.smcrt_last_error()
    assert L.smcrt_scene_set_screens(None, None, 0) == abi.ERR_INVALID_ARG  # (off, on no scene)
    out = (C.c_double * 2)()
    assert L.smcrt_scene_read_screens(None, out) == abi.ERR_INVALID_ARG
    assert L.smcrt_scene_reset_screens(None) == abi.ERR_INVALID_ARG
    n, nd = C.c_int32(), C.c_int64()
    assert L.smcrt_scene_screen_info(None, C.byref(n), C.byref(nd)) == abi.ERR_INVALID_ARG
    # smcrt_screen_hit validates its screen too
    t, px = C.c_double(), C.c_int32()
    p = (C.c_double * 3)(0.0, 0.0, 1.0)
    d = (C.c_double * 3)(0.0, 0.0, -1.0)
    bad = good(); bad.nu = 0
    assert L.smcrt_screen_hit(C.byref(bad), p, d, 2.0, C.byref(t), C.byref(px)) == abi.ERR_INVALID_ARG
    assert L.smcrt_screen_hit(None, p, d, 2.0, C.byref(t), C.byref(px)) == abi.ERR_INVALID_ARG
    # the phasor configuration: bit 0 of reserved is the option, any other bit is refused
    cfg = abi.PhasorConfig()
    for r in (2, 3, 4, -2, 1 << 30):
        cfg.reserved = r
        assert L.smcrt_scene_set_phasor(None, C.byref(cfg)) == abi.ERR_INVALID_ARG
        assert b"reserved" in L.smcrt_last_error(), r
    cfg.reserved = abi.PHASOR_OPTICAL_PATH  # (fails only for the scene)
    assert L.smcrt_scene_set_phasor(None, C.byref(cfg)) == abi.ERR_INVALID_ARG
    assert b"reserved" not in L.smcrt_last_error() and b"NULL" in L.smcrt_last_error()


# ---- 3. smcrt_screen_hit against numpy --------------------------------------------------------------
def np_rule(s, start, d, sep):
    """The hit rule of smcrt.h, operation for operation, on arrays of legs: hit, t, u * nu, v * nv."""
    o, eu, ev = (np.array(list(v)) for v in (s.origin, s.eu, s.ev))

    def dot(a, b):
        return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]

    c = np.array([eu[1] * ev[2] - eu[2] * ev[1], eu[2] * ev[0] - eu[0] * ev[2], eu[0] * ev[1] - eu[1] * ev[0]])
    N = c / np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
    den = dot(d, N)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = dot(o - start, N) / den
        w = (start + t[:, None] * d) - o
        u, v = dot(w, eu) / dot(eu, eu), dot(w, ev) / dot(ev, ev)
    hit = (den != 0.0) & (t > 0.0) & (t <= sep) & (u >= 0.0) & (u < 1.0) & (v >= 0.0) & (v < 1.0)
    if s.sides > 0:
        hit &= den > 0.0
    if s.sides < 0:
        hit &= den < 0.0
    return hit, t, u * s.nu, v * s.nv


def c_rule(lib_path, s, start, d, sep):
    """smcrt_screen_hit on each leg (through a handle of its own, so that plain addresses can be
    passed: 4 * 10^5 calls)."""
    fn = C.CDLL(lib_path).smcrt_screen_hit
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    start, d = np.ascontiguousarray(start), np.ascontiguousarray(d)
    n = len(sep)
    hit, t, px = np.zeros(n, dtype=np.int32), np.full(n, np.nan), np.full(n, -7, dtype=np.int32)
    ps, pd, pt, pp, scr = start.ctypes.data, d.ctypes.data, t.ctypes.data, px.ctypes.data, C.addressof(s)
    for i in range(n):
        hit[i] = fn(scr, ps + 24 * i, pd + 24 * i, sep[i], pt + 8 * i, pp + 4 * i)
    return hit, t, px


def tilted():
    eu = np.array([0.6, 0.3, -0.2])
    ev = np.cross(np.array([0.1, -0.5, 0.7]), eu)
    ev -= eu * (ev @ eu) / (eu @ eu)
    return scene.screen((-0.3, 0.1, -0.2), eu, 0.8 * ev / np.linalg.norm(ev), 5, 7)


SCREENS = {"1x1": lambda: scene.screen((-0.5, -0.5, 0.1), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1, 1),
           "4x3": lambda: scene.screen((-0.5, -0.4, 0.25), (1.0, 0.0, 0.0), (0.0, 0.8, 0.0), 4, 3),
           "tilted": tilted,
           "4096x1": lambda: scene.screen((-0.5, -0.5, -0.3), (0.0, 1.0, 0.0), (0.0, 0.0, 0.7), 4096, 1)}
MARGIN = 1e-9


@pytest.mark.parametrize("name", list(SCREENS))
@pytest.mark.parametrize("sides", [0, 1, -1])
def test_screen_hit_random_legs(lib_path, name, sides):
    """About 10^5 random legs per screen, split over the three `sides`: t to 1e-14, the same
    hit / miss and the same pixel for every leg further than 1e-9 from a pixel edge."""
    s = SCREENS[name]()
    s.sides = sides
    n = 34000
    rng = np.random.default_rng(100 + sides)
    start = rng.uniform(-1.0, 1.0, size=(n, 3))
    # a third of the legs in any direction, the others aimed at the rectangle enlarged by half its
    # size on every side, with lengths up to twice the distance
    o, eu, ev = (np.array(list(v)) for v in (s.origin, s.eu, s.ev))
    target = o + rng.uniform(-0.5, 1.5, size=(n, 1)) * eu + rng.uniform(-0.5, 1.5, size=(n, 1)) * ev
    d = np.where(np.arange(n)[:, None] % 3 == 0, rng.normal(size=(n, 3)), target - start)
    dist = np.linalg.norm(d, axis=1)
    d /= dist[:, None]
    sep = np.where(np.arange(n) % 3 == 0, rng.uniform(0.0, 3.0, size=n), dist * rng.uniform(0.0, 2.0, size=n))
    hit, t, un, vn = np_rule(s, start, d, sep)
    near = (np.abs(un - np.rint(un)) <= MARGIN) | (np.abs(vn - np.rint(vn)) <= MARGIN) | (np.abs(t - sep) <= MARGIN)
    assert np.count_nonzero(near) < 1e-3 * n  # (the numpy side alone: the margin exempts almost nothing)
    assert 0.02 * n < np.count_nonzero(hit) < 0.9 * n
    got_hit, got_t, got_px = c_rule(lib_path, s, start, d, sep)
    ok = ~near
    assert np.array_equal(got_hit[ok] == 1, hit[ok]) and np.all((got_hit == 0) | (got_hit == 1))
    both = ok & hit
    np.testing.assert_allclose(got_t[both], t[both], rtol=1e-14, atol=0.0)
    want_px = np.minimum(un.astype(np.int64), s.nu - 1) + s.nu * np.minimum(vn.astype(np.int64), s.nv - 1)
    assert np.array_equal(got_px[both], want_px[both])
    assert np.all(np.isnan(got_t[got_hit == 0])) and np.all(got_px[got_hit == 0] == -7)  # (a miss writes nothing)
    if s.nu * s.nv > 1:
        assert len(np.unique(got_px[both])) > 1


def test_screen_hit_constructed(lib_path):
    """A leg that ends exactly on the plane hits (t == sep) and the leg that starts there misses;
    parallel legs, legs that stop short and legs past the rectangle miss; all three `sides`."""
    rows = []  # (sides, start, dir, sep, hit, t, pixel)
    x, y, zs = 0.3, -0.1, 0.25  # pixel: u = 0.8 -> iu 3 of 4, v = 0.375 -> iv 1 of 3
    down, up = (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)
    for sides in (0, 1, -1):
        d_ok, u_ok = sides <= 0, sides >= 0  # N = +z: a leg going down has dir . N < 0
        rows += [(sides, (x, y, 1.0), down, 0.75, d_ok, 0.75, 3 + 4 * 1),   # ends exactly on the plane
                 (sides, (x, y, zs), down, 0.75, False, None, None),        # the follow-on leg: t == 0
                 (sides, (x, y, 1.0), down, 2.0, d_ok, 0.75, 7),
                 (sides, (x, y, 1.0), down, 0.5, False, None, None),        # stops short
                 (sides, (x, y, 1.0), down, 0.75 - 2.0 ** -50, False, None, None),
                 (sides, (x, y, -1.0), up, 1.25, u_ok, 1.25, 7),            # from below, ends on the plane
                 (sides, (x, y, zs), up, 1.0, False, None, None),
                 (sides, (x, y, 1.0), up, 5.0, False, None, None),          # flying away: t < 0
                 (sides, (x, y, 0.5), (1.0, 0.0, 0.0), 5.0, False, None, None),  # parallel
                 (sides, (x, y, zs), (0.0, 1.0, 0.0), 5.0, False, None, None),   # parallel, in the plane
                 (sides, (0.5, y, 1.0), down, 2.0, False, None, None),      # u == 1: outside
                 (sides, (-0.5, y, 1.0), down, 2.0, d_ok, 0.75, 4),         # u == 0: inside, iu 0
                 (sides, (x, 0.4, 1.0), down, 2.0, False, None, None),      # v == 1: outside
                 (sides, (x, -0.4, 1.0), down, 2.0, d_ok, 0.75, 3),         # v == 0: inside, iv 0
                 (sides, (0.7, y, 1.0), down, 2.0, False, None, None),
                 (sides, (x, -0.9, 1.0), down, 2.0, False, None, None)]
    for sides, start, d, sep, hit, t, px in rows:
        s = SCREENS["4x3"]()
        s.sides = sides
        gh, gt, gp = c_rule(lib_path, s, np.array([start]), np.array([d]), np.array([sep]))
        assert bool(gh[0]) == hit, (sides, start, d, sep)
        if hit:
            assert gt[0] == t and gp[0] == px, (sides, start, d, sep, gt[0], gp[0])
        nh = np_rule(s, np.array([start]), np.array([d], dtype=float), np.array([sep]))[0]
        assert bool(nh[0]) == hit  # (the numpy restatement agrees on the constructed cases too)


# ---- 4. write_screen --------------------------------------------------------------------------------
def test_write_screen(lib_path, tmp_path):
    """abs(field)**2 as fp32 through the NRRD writer with nz = 1, under phasor/<outfile>."""
    from rsmcrt_amd import output
    rng = np.random.default_rng(12)
    f = rng.normal(size=(3, 5)) + 1j * rng.normal(size=(3, 5))
    name = output.write_screen(tmp_path, "screen0.nrrd", f)
    assert os.path.samefile(name, tmp_path / "phasor" / "screen0.nrrd")
    want = output.write_data(tmp_path / "want.nrrd", (np.abs(f) ** 2).astype(np.float32).reshape(1, 3, 5))
    raw = open(name, "rb").read()
    assert raw == open(want, "rb").read()
    data = np.frombuffer(raw[-3 * 5 * 4:], dtype="<f4").reshape(3, 5)
    assert np.array_equal(data, (np.abs(f) ** 2).astype(np.float32))  # (raw, little-endian, u fastest)
    with pytest.raises(ValueError):
        output.write_screen(tmp_path, "x.nrrd", np.zeros((3, 5)))
    with pytest.raises(ValueError):
        output.write_screen(tmp_path, "x.nrrd", np.zeros((1, 3, 5), dtype=complex))
