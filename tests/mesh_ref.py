"""Test infrastructure only: ctypes front end of tests/mesh_ref.c, the serial restatement of the
mesh-media semantics with its brute-force cast. Compiled on first use with the
oracle Makefile's floating-point flags and linked against oracle/liboracle.so, as tests/voxel_ref.py
does; `run` has oracle.pyoracle.run's shape, with a rsmcrt_amd.scene.MeshScene in place of the SDF
scene."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile
import threading

import numpy as np

from oracle import pyoracle
from rsmcrt_amd import abi
from rsmcrt_amd.scene import detector_array
from rsmcrt_amd.tallies import Result

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "mesh_ref.c")
HEADER = os.path.join(os.path.dirname(HERE), "include", "smcrt.h")
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-Wall", "-Wextra", "-std=c11"]  # oracle/Makefile
_lock = threading.Lock()
_lib = None
_DP, _IP, _BP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _build() -> str:
    oracle_so = pyoracle.build()
    out = os.path.join(HERE, "libmesh_ref.so")
    newest = max(os.path.getmtime(p) for p in (SRC, HEADER, oracle_so))
    if os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    if not os.access(HERE, os.W_OK):
        out = os.path.join(tempfile.mkdtemp(prefix="mesh_ref_"), "libmesh_ref.so")
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
            L.mesh_ref_run.argtypes = [_DP, C.c_int32, _IP, _BP, C.c_int32, C.POINTER(abi.Medium), C.c_int32, C.c_int32,
                                       C.POINTER(abi.Grid), C.POINTER(abi.Detector), C.c_int32, C.POINTER(abi.Source),
                                       C.POINTER(abi.RunConfig), C.POINTER(abi.Tallies)]
            L.mesh_ref_cast.argtypes = [_DP, _IP, C.c_int32, C.c_int64, _DP, _DP, _IP, _DP, _IP]
            _lib = L
    return _lib


def cast(verts, tris, origins, dirs, skips):
    """The brute-force cast of every ray: (t, tri), t = inf and tri = -1 where nothing is hit."""
    verts = np.ascontiguousarray(verts, dtype=np.float64)
    tris = np.ascontiguousarray(tris, dtype=np.int32)
    o = np.ascontiguousarray(origins, dtype=np.float64)
    d = np.ascontiguousarray(dirs, dtype=np.float64)
    s = np.ascontiguousarray(skips, dtype=np.int32)
    t, tri = np.empty(len(o)), np.empty(len(o), dtype=np.int32)
    st = lib().mesh_ref_cast(verts.ctypes.data_as(_DP), tris.ctypes.data_as(_IP), len(tris), len(o), o.ctypes.data_as(_DP),
                             d.ctypes.data_as(_DP), s.ctypes.data_as(_IP), t.ctypes.data_as(_DP), tri.ctypes.data_as(_IP))
    assert st == 0
    return t, tri


def run(ms, grid, source, n_photons, seed=123456789, flags=abi.FLAG_PATHLENGTH, dets=(), first_photon=0,
        records=False, result=None) -> Result:
    dets = list(dets)
    ms.check_grid(grid)
    res = result if result is not None else Result(grid, dets, n_photons, records)
    res.n_photons += n_photons
    cfg = abi.RunConfig()
    cfg.n_photons, cfg.first_photon, cfg.seed = n_photons, first_photon, seed
    cfg.flags = flags | (abi.FLAG_RECORD_PHOTONS if records else 0)
    media = ms.media_array()
    darr = detector_array(dets)
    t = res.tallies()
    st = lib().mesh_ref_run(ms.verts.ctypes.data_as(_DP), len(ms.verts), ms.tris.ctypes.data_as(_IP),
                            ms.tri_media.ctypes.data_as(_BP), len(ms.tris), media, ms.n_media, ms.ambient, C.byref(grid),
                            darr, len(dets), C.byref(source), C.byref(cfg), C.byref(t))
    if st != 0:
        raise RuntimeError(f"mesh_ref_run failed: {abi.STATUS_NAMES.get(st, st)}")
    return res
