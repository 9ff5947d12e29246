"""Test infrastructure only: ctypes front end of tests/voxel_ref.c, the serial restatement of the
voxel-media semantics. Compiled on first use with the oracle Makefile's
floating-point flags and linked against oracle/liboracle.so; `run` has oracle.pyoracle.run's
shape, with a rsmcrt_amd.scene.VoxelScene in place of the SDF scene."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile
import threading

from oracle import pyoracle
from rsmcrt_amd import abi
from rsmcrt_amd.scene import detector_array
from rsmcrt_amd.tallies import Result

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "voxel_ref.c")
HEADER = os.path.join(os.path.dirname(HERE), "include", "smcrt.h")
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-std=c11"]  # oracle/Makefile
UNSUPPORTED_REEMISSION = -100  # VOXEL_REF_UNSUPPORTED
_lock = threading.Lock()
_lib = None


def _build() -> str:
    oracle_so = pyoracle.build()
    out = os.path.join(HERE, "libvoxel_ref.so")
    newest = max(os.path.getmtime(p) for p in (SRC, HEADER, oracle_so))
    if os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    if not os.access(HERE, os.W_OK):
        out = os.path.join(tempfile.mkdtemp(prefix="voxel_ref_"), "libvoxel_ref.so")
    odir = os.path.dirname(oracle_so)
    tmp = f"{out}.{os.getpid()}.tmp"
    subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", tmp, SRC, oracle_so,
                    f"-Wl,-rpath,{odir}", "-lm"], check=True)
    os.replace(tmp, out)
    return out


def lib():
    global _lib
    with _lock:
        if _lib is None:
            pyoracle.lib()  # (liboracle.so is loaded first, whatever the rpath says)
            L = C.CDLL(_build())
            L.voxel_ref_run.argtypes = [C.POINTER(C.c_uint8), C.POINTER(abi.Medium), C.c_int32, C.POINTER(abi.Grid),
                                        C.POINTER(abi.Detector), C.c_int32, C.POINTER(abi.Source),
                                        C.POINTER(abi.RunConfig), C.POINTER(abi.Tallies)]
            _lib = L
    return _lib


def run(vscene, grid, source, n_photons, seed=123456789, flags=abi.FLAG_PATHLENGTH, dets=(), first_photon=0,
        records=False, result=None) -> Result:
    dets = list(dets)
    vscene.check_grid(grid)
    res = result if result is not None else Result(grid, dets, n_photons, records)
    res.n_photons += n_photons
    cfg = abi.RunConfig()
    cfg.n_photons, cfg.first_photon, cfg.seed = n_photons, first_photon, seed
    cfg.flags = flags | (abi.FLAG_RECORD_PHOTONS if records else 0)
    media = vscene.media_array()
    darr = detector_array(dets)
    t = res.tallies()
    st = lib().voxel_ref_run(vscene.labels.ctypes.data_as(C.POINTER(C.c_uint8)), media, vscene.n_media, C.byref(grid),
                             darr, len(dets), C.byref(source), C.byref(cfg), C.byref(t))
    if st != 0:
        raise RuntimeError(f"voxel_ref_run failed: {abi.STATUS_NAMES.get(st, st)}")
    return res
