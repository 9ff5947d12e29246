"""The phasor tally (include/smcrt.h "phasor tally") without a GPU: the header, abi.py and the
Fortran module agree on the new names, the flag and the struct; the entry points are exported
and answer before any device call where they can; output.write_phasor writes what the
reference's commented-out line would."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rsmcrt_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smcrt.h")
FORTRAN = os.path.join(ROOT, "bindings", "fortran", "smcrt_mod.f90")
FUNCTIONS = ["smcrt_scene_set_phasor", "smcrt_scene_read_phasor", "smcrt_scene_reset_phasor"]
FIELDS = ["fixed_k", "reserved", "wavenumber"]


def test_exports_and_version(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for fn in FUNCTIONS:
        assert fn in exported, fn
        assert fn in abi.EXPORTED_SYMBOLS, fn
    from rsmcrt_amd import engine
    assert engine.load_library(lib_path).smcrt_abi_version() == 5  # (additive: the version stays)
    assert abi.FLAG_PHASOR == 1 << 9


def test_header_and_abi_agree(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("flag %u\\n", (unsigned)SMCRT_FLAG_PHASOR);',
             'printf("version %d\\n", (int)SMCRT_ABI_VERSION);',
             'printf("size %zu\\n", sizeof(smcrt_phasor_config));']
    lines += [f'printf("{f} %zu\\n", offsetof(smcrt_phasor_config, {f}));' for f in FIELDS]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["flag"]) == abi.FLAG_PHASOR == 512
    assert int(got["version"]) == abi.SMCRT_ABI_VERSION == 5
    assert int(got["size"]) == C.sizeof(abi.PhasorConfig) == 16
    for f in FIELDS:
        assert int(got[f]) == getattr(abi.PhasorConfig, f).offset, f
    # the flag shares no bit with another run flag
    others = [v for k, v in vars(abi).items() if k.startswith("FLAG_") and k != "FLAG_PHASOR"]
    assert all(isinstance(v, int) and not v & abi.FLAG_PHASOR for v in others) and len(others) >= 9


def test_fortran_module_agrees():
    """bindings/fortran/smcrt_mod.f90 (text: the suite does not need a Fortran compiler for this):
    the flag's value, the bind(C) type field for field, an interface per entry point, and the
    module's ABI version unchanged."""
    txt = open(FORTRAN).read()
    low = re.sub(r"&\s*\n\s*", " ", txt.lower())
    assert re.search(r"smcrt_flag_phasor\s*=\s*512\b", low)
    assert re.search(r"smcrt_mod_abi_version\s*=\s*5\b", low)
    m = re.search(r"type,\s*bind\(c\)\s*::\s*smcrt_phasor_config(.*?)end type smcrt_phasor_config", low, re.S)
    assert m, "smcrt_phasor_config is missing"
    decl = [l.split("!")[0].strip() for l in m.group(1).splitlines() if l.split("!")[0].strip()]
    # field order and kinds: two int32, then a double (as the C struct and abi.PhasorConfig)
    assert len(decl) == 2 and decl[0].startswith("integer(c_int32_t)") and decl[1].startswith("real(c_double)")
    names = [re.match(r"\s*(\w+)", part).group(1) for d in decl for part in d.split("::")[1].split(",")]
    assert names == FIELDS == [n for n, _ in abi.PhasorConfig._fields_]
    for fn in FUNCTIONS:
        assert re.search(rf'function {fn}\(.*?\)\s*bind\(c,\s*name="{fn}"\)', low), fn
        assert f"end function {fn}" in low, fn


FC = os.environ.get("AMDFLANG", "/opt/rocm/bin/amdflang")


@pytest.mark.skipif(not os.path.exists(FC), reason="no Fortran compiler in this image")
def test_fortran_module_compiles_and_calls(lib_path, tmp_path):
    """The module compiles, the type has the C struct's size, and the three interfaces link and
    answer a NULL scene with SMCRT_ERR_INVALID_ARG."""
    prog = """program phasor_sizes
    use iso_c_binding
    use smcrt_mod
    implicit none
    type(smcrt_phasor_config), target :: cfg
    complex(c_double_complex) :: grid(2)
    grid = (0._c_double, 0._c_double)
    cfg%fixed_k = 1
    cfg%wavenumber = 2._c_double
    print '(a,i0)', 'size ', c_sizeof(cfg)
    print '(a,i0)', 'flag ', SMCRT_FLAG_PHASOR
    print '(a,i0)', 'set ', smcrt_scene_set_phasor(c_null_ptr, c_loc(cfg))
    print '(a,i0)', 'off ', smcrt_scene_set_phasor(c_null_ptr, c_null_ptr)
    print '(a,i0)', 'read ', smcrt_scene_read_phasor(c_null_ptr, grid)
    print '(a,i0)', 'reset ', smcrt_scene_reset_phasor(c_null_ptr)
end program phasor_sizes
"""
    (tmp_path / "smcrt_mod.f90").write_text(open(FORTRAN).read())
    (tmp_path / "phasor_sizes.f90").write_text(prog)
    libdir = os.path.dirname(lib_path)
    subprocess.run([FC, "-O2", "-c", "smcrt_mod.f90"], cwd=tmp_path, check=True)
    subprocess.run([FC, "-o", "phasor_sizes", "phasor_sizes.f90", "smcrt_mod.o", f"-L{libdir}", "-lsmcrt",
                    f"-Wl,-rpath,{libdir}"], cwd=tmp_path, check=True)
    out = subprocess.run([str(tmp_path / "phasor_sizes")], capture_output=True, text=True, check=True).stdout
    got = dict(l.split() for l in out.splitlines())
    assert int(got["size"]) == C.sizeof(abi.PhasorConfig) and int(got["flag"]) == abi.FLAG_PHASOR
    assert [int(got[k]) for k in ("set", "off", "read", "reset")] == [abi.ERR_INVALID_ARG] * 4


def test_errors_before_the_device(lib_path):
    """NULL scenes and a bad fixed wavenumber are INVALID_ARG with a message, decided without a
    device; the drivers' refusals of the flag need a scene and are in tests/test_gpu_phasor.py."""
    from rsmcrt_amd import engine
    L = engine.load_library(lib_path)
    cfg = abi.PhasorConfig()
    assert L.smcrt_scene_set_phasor(None, C.byref(cfg)) == abi.ERR_INVALID_ARG
    assert L.smcrt_scene_set_phasor(None, None) == abi.ERR_INVALID_ARG
    out = (C.c_double * 2)()
    assert L.smcrt_scene_read_phasor(None, out) == abi.ERR_INVALID_ARG
    assert L.smcrt_scene_reset_phasor(None) == abi.ERR_INVALID_ARG
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        cfg.fixed_k, cfg.wavenumber = 1, bad
        assert L.smcrt_scene_set_phasor(None, C.byref(cfg)) == abi.ERR_INVALID_ARG
        assert b"wavenumber" in L.smcrt_last_error(), bad
    cfg.fixed_k, cfg.wavenumber = 0, float("nan")  # (ignored without fixed_k: only the scene is wrong)
    assert L.smcrt_scene_set_phasor(None, C.byref(cfg)) == abi.ERR_INVALID_ARG
    assert b"wavenumber" not in L.smcrt_last_error()
    cfg.fixed_k, cfg.wavenumber = 1, 0.0  # (zero is allowed)
    assert L.smcrt_scene_set_phasor(None, C.byref(cfg)) == abi.ERR_INVALID_ARG
    assert b"wavenumber" not in L.smcrt_last_error()


def test_write_phasor(lib_path, tmp_path):
    """abs(phasor)**2 as fp32 through the NRRD writer, under phasor/<outfile>."""
    from rsmcrt_amd import output
    rng = np.random.default_rng(11)
    p = rng.normal(size=(3, 4, 5)) + 1j * rng.normal(size=(3, 4, 5))
    name = output.write_phasor(tmp_path, "fringes.nrrd", p)
    assert os.path.samefile(name, tmp_path / "phasor" / "fringes.nrrd")
    want = output.write_data(tmp_path / "want.nrrd", (np.abs(p) ** 2).astype(np.float32))
    assert open(name, "rb").read() == open(want, "rb").read()
    raw = open(name, "rb").read()
    data = np.frombuffer(raw[-3 * 4 * 5 * 4:], dtype="<f4").reshape(3, 4, 5)
    assert np.array_equal(data, (np.abs(p) ** 2).astype(np.float32))  # (raw, little-endian, x fastest)
    with pytest.raises(ValueError):
        output.write_phasor(tmp_path, "x.nrrd", np.zeros((3, 4, 5)))
