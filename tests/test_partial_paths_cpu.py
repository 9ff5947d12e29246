"""Partial path lengths (include/smcrt.h "partial path lengths") without a GPU: the struct layouts and
the flag against abi.py, the new entry points, what they decide without a device, and the numpy
helpers of rsmcrt_amd/partialpaths.py on hand-made arrays with exact expected values."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from rsmcrt_amd import abi
from rsmcrt_amd import partialpaths as PP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smcrt.h")
NEW_FUNCTIONS = ["smcrt_scene_set_partial_paths", "smcrt_scene_partial_path_counts", "smcrt_scene_read_partial_paths"]
STRUCTS = {
    "smcrt_ppath_config": (abi.PPathConfig, ["range_first", "range_count", "max_records", "reserved"]),
    "smcrt_ppath": (abi.PPath, ["photon", "detector", "hit", "status", "layer", "nscatt", "reserved", "start", "dir",
                                "point_sep", "weight"]),
}


def test_struct_layout_and_flag(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("flag %u\\n", (unsigned)SMCRT_FLAG_PARTIAL_PATHS);',
             'printf("cap %d\\n", (int)SMCRT_PPATH_MAX_MEDIA);',
             'printf("version %d\\n", (int)SMCRT_ABI_VERSION);']
    for s, (_, fields) in STRUCTS.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for f in fields:
            lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["flag"]) == abi.FLAG_PARTIAL_PATHS
    assert int(got["cap"]) == abi.PPATH_MAX_MEDIA
    assert int(got["version"]) == abi.SMCRT_ABI_VERSION == 5  # new functions, one flag and new structs only
    for s, (cls, fields) in STRUCTS.items():
        assert int(got[s]) == C.sizeof(cls), s
        for f in fields:
            assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, (s, f)
    dt = abi.ppath_dtype()
    assert dt.itemsize == C.sizeof(abi.PPath)
    for f in STRUCTS["smcrt_ppath"][1]:
        assert dt.fields[f][1] == getattr(abi.PPath, f).offset, f


def test_flag_value():
    assert abi.FLAG_PARTIAL_PATHS == 1 << 10
    others = [abi.FLAG_PATHLENGTH, abi.FLAG_SURVIVAL_BIAS, abi.FLAG_RENDER_SOURCE, abi.FLAG_TEST_KERNEL,
              abi.FLAG_END_EARLY, abi.FLAG_RECORD_PHOTONS, abi.FLAG_ASYNC_FOLD, abi.FLAG_OVERLAP, abi.FLAG_TRACK_PATHS,
              abi.FLAG_PHASOR]
    assert all(abi.FLAG_PARTIAL_PATHS & f == 0 for f in others)
    txt = open(HEADER).read()
    assert re.search(r"SMCRT_FLAG_PARTIAL_PATHS = 1u << 10\b", txt)


def test_exports(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for fn in NEW_FUNCTIONS:
        assert fn in exported, fn
        assert fn in abi.EXPORTED_SYMBOLS, fn


def test_errors_before_the_device(lib_path):
    """NULL scenes are INVALID_ARG with a message, decided without a device."""
    from rsmcrt_amd import engine
    L = engine.load_library(lib_path)
    cfg = abi.PPathConfig()
    cfg.max_records = 1
    assert L.smcrt_scene_set_partial_paths(None, C.byref(cfg)) == abi.ERR_INVALID_ARG and L.smcrt_last_error()
    n = C.c_int64()
    assert L.smcrt_scene_partial_path_counts(None, C.byref(n), None) == abi.ERR_INVALID_ARG
    assert L.smcrt_scene_read_partial_paths(None, None, None) == abi.ERR_INVALID_ARG


def test_launch_choice_keeps_its_eight_arguments():
    """launch_choice takes the lengths' LDS through a defaulted trailing parameter, so the probe of
    tests/sceneplan_probe.cpp, which passes eight, compiles unchanged."""
    txt = open(os.path.join(ROOT, "rsmcrt_amd", "csrc", "sceneplan.h")).read()
    sig = re.search(r"inline LaunchChoice launch_choice\(([^)]*)\)", txt).group(1)
    params = [p.strip() for p in sig.replace("\n", " ").split(",")]
    assert len(params) == 9 and params[8].replace(" ", "") == "size_tppl_lds=0", params
    assert all("=" not in p for p in params[:8])


# ---- the helpers -------------------------------------------------------------------------------
def headers(detector, weight):
    h = np.zeros(len(detector), dtype=abi.ppath_dtype())
    h["detector"] = detector
    h["weight"] = weight
    return h


def test_time_of_flight():
    lengths = np.array([[1.0, 2.0, 0.0], [0.5, 0.0, 4.0], [0.0, 0.0, 0.0]])
    n = [1.0, 1.5, 2.0]
    t = PP.time_of_flight(lengths, n, 2.0)
    assert t.tolist() == [(1.0 + 3.0) / 2.0, (0.5 + 8.0) / 2.0, 0.0]
    assert PP.time_of_flight(np.zeros((0, 3)), n, 2.0).shape == (0,)
    with pytest.raises(ValueError):
        PP.time_of_flight(lengths, [1.0, 1.5], 2.0)


def test_reweight():
    rng = np.random.default_rng(5)
    w = rng.uniform(0.1, 1.0, 40)
    lengths = rng.uniform(0.0, 30.0, (40, 3))
    mua = np.array([0.3, 0.0, 2.5])
    assert np.array_equal(PP.reweight(w, lengths, mua, mua), w)  # a zero change: the weights bit for bit
    assert np.array_equal(PP.reweight(w, lengths, mua, mua.copy()), w)
    # exact values: exp of 0, and of sums that are exactly representable
    got = PP.reweight([1.0, 0.5, 2.0], [[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]], [0.0, 0.0], [0.0, 0.5])
    assert got.tolist() == [1.0, 0.5 * np.exp(-1.0), 2.0 * np.exp(-0.5)]
    # towards less absorption the weight grows
    assert PP.reweight([1.0], [[2.0, 0.0]], [1.0, 0.0], [0.0, 0.0])[0] == np.exp(2.0)
    with pytest.raises(ValueError):
        PP.reweight([1.0], [[1.0, 0.0]], [0.0], [0.0, 0.0])


def test_tof_histogram():
    # times (n = 1, c = 1: the length itself); 0.0 is the first edge, 1.0 an inner edge, 2.0 the right end
    lengths = np.array([[0.0], [1.0], [2.0], [0.5], [1.5], [0.25], [5.0]])
    det = [0, 0, 0, 0, 1, -1, 0]
    w = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0]
    edges = [0.0, 1.0, 2.0]
    h0 = PP.tof_histogram(headers(det, w), lengths, [1.0], 1.0, edges, 0)
    # 0.0 is in bin 0 (the left edge is inclusive), 1.0 in bin 1, 2.0 and 5.0 are out of range
    assert h0.tolist() == [1.0 + 8.0, 2.0]
    assert PP.tof_histogram(headers(det, w), lengths, [1.0], 1.0, edges, 1).tolist() == [0.0, 16.0]
    assert PP.tof_histogram(headers(det, w), lengths, [1.0], 1.0, edges, -1).tolist() == [32.0, 0.0]
    assert PP.tof_histogram(headers(det, w), lengths, [1.0], 1.0, edges, 7).tolist() == [0.0, 0.0]
    # n and c scale the time (t = len / 2 here): below the first edge is dropped too, 0.5 is the right end
    assert PP.tof_histogram(headers(det, w), lengths, [2.0], 4.0, [0.25, 0.5], 0).tolist() == [8.0]
    with pytest.raises(ValueError):
        PP.tof_histogram(headers(det, w), lengths, [1.0], 1.0, [1.0, 1.0], 0)
