"""Build and run tests/sceneplan_probe.cpp: the engine's device-free scene plan
(rsmcrt_amd/csrc/sceneplan.h) as a dict, on a machine without a GPU.

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


def plan(sc, g, dets=(), env=None, nodes=None, top=None):
    """The plan of scene `sc` on grid `g`: ints, floats (exact: the probe prints hex floats) and
    lists of them, plus `status` (abi.OK or an error code) and `error` (its message). `nodes` /
    `top` replace the scene's arrays (invalid scenes)."""
    nodes = sc.node_array() if nodes is None else nodes
    top = list(sc.top) if top is None else list(top)
    blob = (struct.pack("3i", len(nodes), len(top), len(dets)) + bytes(nodes) + struct.pack(f"{len(top)}i", *top) +
            bytes(g) + (bytes(S.detector_array(dets)) if dets else b""))
    with tempfile.NamedTemporaryFile(suffix=".scene") as f:
        f.write(blob)
        f.flush()
        raw = _run(["plan", f.name], env)
    out = {"status": int(raw.pop("status")), "error": raw.pop("error")}
    out.update({k: _value(v) for k, v in raw.items()})
    return out


def slot_depth(lean_or_far, cap_bytes, total_mem, env=None):
    """sceneplan.h slot_depth with the pool knobs of `env`."""
    return int(_run(["slots", str(int(lean_or_far)), str(int(cap_bytes)), str(int(total_mem))], env)["slots"])
