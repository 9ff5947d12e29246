"""Build and run tests/sceneplan_probe.cpp: the engine's device-free scene plan
(rsmcrt_amd/csrc/sceneplan.h) as a dict, and the plan's culling grid (cull.h) as arrays, on a
machine without a GPU.

The probe is host code only (hipcc in host-only mode over the probe, sceneplan.cpp and
cull.cpp; no kernel object, no libsmcrt.so), cached next to the library and rebuilt
when one of its sources is newer. The SMCRT_* knobs reach it through its environment.
"""
import os
import struct
import subprocess
import tempfile

from rsmcrt_amd import build as B
from rsmcrt_amd import scene as S

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = [os.path.join(HERE, "sceneplan_probe.cpp"), os.path.join(B.PKG, "csrc", "sceneplan.cpp"),
           os.path.join(B.PKG, "csrc", "cull.cpp")]
EXE = os.path.join(B.PKG, "sceneplan_probe")  # (next to libsmcrt.so; git-ignored)


def build() -> str:
    deps = set()
    for src in SOURCES:
        B.includes(src, deps)
    if B._stale(EXE, deps):
        flags = [f for f in B.FLAGS if not f.startswith("--offload-arch")]
        subprocess.run([B.hipcc(), *flags, "-x", "hip", "--offload-host-only", "-o", EXE + ".tmp", *SOURCES, "-lpthread"],
                       check=True)
        os.replace(EXE + ".tmp", EXE)
    return EXE


def _run(args, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("SMCRT_")}
    e.update(env or {})
    out = subprocess.run([build(), *args], env=e, check=True, capture_output=True, text=True).stdout
    return dict(line.split("=", 1) for line in out.splitlines() if "=" in line)


def _value(v):
    if "," in v:
        return [_value(x) for x in v.split(",") if x]
    try:
        return int(v)
    except ValueError:
        return float.fromhex(v)


def _blob(sc, g, dets=(), nodes=None, top=None):
    nodes = sc.node_array() if nodes is None else nodes
    top = list(sc.top) if top is None else list(top)
    return (struct.pack("3i", len(nodes), len(top), len(dets)) + bytes(nodes) + struct.pack(f"{len(top)}i", *top) +
            bytes(g) + (bytes(S.detector_array(dets)) if dets else b""))


def plan(sc, g, dets=(), env=None, nodes=None, top=None):
    """The plan of scene `sc` on grid `g`: ints, floats (exact: the probe prints hex floats) and
    lists of them, plus `status` (abi.OK or an error code) and `error` (its message). `nodes` /
    `top` replace the scene's arrays (invalid scenes)."""
    with tempfile.NamedTemporaryFile(suffix=".scene") as f:
        f.write(_blob(sc, g, dets, nodes, top))
        f.flush()
        raw = _run(["plan", f.name], env)
    out = {"status": int(raw.pop("status")), "error": raw.pop("error")}
    out.update({k: _value(v) for k, v in raw.items()})
    return out


def choices(sc, g, states, dets=(), env=None, kind="sdf"):
    """The launch choices (sceneplan.h launch_choice) of the plan of `sc` on `g`, one dict per run
    state (xsrc, flags, lean_ok, paths_on, phasor_on, n_screens): `family`, the template
    coordinates, `block` ("ws" or "256"), `lds` and `grid_key`. `kind` "voxel" / "mesh" marks the
    plan as such after planning (see the probe's header)."""
    with tempfile.NamedTemporaryFile(suffix=".scene") as f:
        f.write(_blob(sc, g, dets))
        f.flush()
        e = {k: v for k, v in os.environ.items() if not k.startswith("SMCRT_")}
        e.update(env or {})
        args = [str(int(v)) for st in states for v in st]
        lines = subprocess.run([build(), "choice", f.name, kind, *args], env=e, check=True, capture_output=True,
                               text=True).stdout.splitlines()
    assert lines[0] == "status=0", lines[:2]
    out = []
    for line in lines[2:]:
        k, v = line.split("=", 1)
        if k == "family":
            out.append({})
        out[-1][k] = v if k in ("family", "block") else int(v)
    assert len(out) == len(states)
    return out


def cull(sc, g, env=None):
    """The culling grid (cull.h CullHost) of the plan of `sc` on `g`, as the kernels read it: a
    dict with `enabled`, `n` (cells per axis), `lo`, `cell`, `off` (ncells + 1), `list` (entries
    x 2 words: top | flags, node), `elb` (float32 per entry), `lb` (per cell) and `always`."""
    import numpy as np
    with tempfile.NamedTemporaryFile(suffix=".scene") as f, tempfile.NamedTemporaryFile(suffix=".cull") as out:
        f.write(_blob(sc, g))
        f.flush()
        raw = _run(["cull", f.name, out.name], env)
        assert int(raw["status"]) == 0, raw["error"]
        data = out.read()
    enabled, nx, ny, nz, n_always, _ = struct.unpack_from("6i", data, 0)
    geo = struct.unpack_from("4d", data, 24)
    n_off, n_list, n_elb, n_lb = struct.unpack_from("4Q", data, 56)
    pos = 88
    res = {"enabled": bool(enabled), "n": (nx, ny, nz), "lo": geo[:3], "cell": geo[3]}
    for key, dtype, count in (("off", "<u4", n_off), ("list", "<u4", n_list), ("elb", "<f4", n_elb), ("lb", "<f8", n_lb),
                              ("always", "<i4", n_always)):
        res[key] = np.frombuffer(data, dtype=dtype, count=count, offset=pos)
        pos += count * np.dtype(dtype).itemsize
    assert pos == len(data)
    res["list"] = res["list"].reshape(-1, 2)
    return res


def slot_depth(lean_or_far, cap_bytes, total_mem, env=None):
    """sceneplan.h slot_depth with the pool knobs of `env`."""
    return int(_run(["slots", str(int(lean_or_far)), str(int(cap_bytes)), str(int(total_mem))], env)["slots"])
