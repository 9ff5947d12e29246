"""The volume source (include/smcrt.h "volume source") without a GPU: the exports and the Fortran
text; the refusals made before any device call; smcrt_volume_pick on the edge cases of the table;
smcrt_volume_sample, the text the kernel runs, bit for bit against the rule restated in Python
floats with the oracle's Philox and sincos; the sampler's statistics; and the weight arithmetic
and restore-on-exception of rsmcrt_amd.fluorescence against a stub engine."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from rsmcrt_amd import abi, scene
from rsmcrt_amd import fluorescence as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORTRAN = os.path.join(ROOT, "bindings", "fortran", "smcrt_mod.f90")
FUNCTIONS = ["smcrt_scene_set_volume_source", "smcrt_scene_volume_source_info", "smcrt_volume_sample",
             "smcrt_volume_pick"]
SEED = 123456789
GRID_543 = (5, 4, 3, 1.0, 0.75, 0.4)  # unequal half-extents, no axis a power of two
GRID_888 = (8, 8, 8, 1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def L(lib_path):
    from rsmcrt_amd import engine
    return engine.load_library(lib_path)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def last_error(L):
    return L.smcrt_last_error().decode(errors="replace")


def pick(L, w, u):
    w = np.ascontiguousarray(w, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    out = np.full(len(u), -1, dtype=np.int64)
    st = L.smcrt_volume_pick(_dp(w), len(w), _dp(u), len(u), _ip(out))
    assert st == abi.OK, last_error(L)
    return out


def sample(L, w, g, n, seed=SEED, first=0):
    """(pos (n, 3), dir (n, 3), voxel (n,)) of smcrt_volume_sample."""
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
    pos, d, vox = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, -1, dtype=np.int64)
    st = L.smcrt_volume_sample(_dp(w), C.byref(g), seed, first, n, _dp(pos), _dp(d), _ip(vox))
    assert st == abi.OK, last_error(L)
    return pos, d, vox


def weights_for(dims, seed=7, zero_fraction=0.3):
    """Weights in [0.2, 1) with about `zero_fraction` of the voxels at exactly 0."""
    rng = np.random.default_rng(seed)
    n = dims[0] * dims[1] * dims[2]
    w = rng.uniform(0.2, 1.0, n)
    w[rng.uniform(size=n) < zero_fraction] = 0.0
    return w


# ---- the rule restated (include/smcrt.h): Python floats are IEEE fp64 without fused multiply-add ----
def seq_cdf(w):
    """cdf[i] = cdf[i-1] + w[i], strictly left to right; (cdf, total, last)."""
    cdf, run, last = np.zeros(len(w)), 0.0, -1
    for i, x in enumerate(w):
        nxt = run + float(x)
        if nxt > run:
            last = i
        run = nxt
        cdf[i] = run
    return cdf, run, last


def np_pick(cdf, total, last, u):
    x = np.asarray(u, dtype=np.float64) * total
    i = np.searchsorted(cdf, x, "right")  # the smallest index with cdf[i] > x
    return np.where(i < len(cdf), i, last)


def np_sample(w, dims, n, seed=SEED, first=0):
    nx, ny, nz, xmax, ymax, zmax = dims
    cdf, total, last = seq_cdf(w)
    pos, d, vox = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int64)
    for p in range(n):
        u = [O.uniform(seed, first + p, k) for k in range(6)]
        v = int(np_pick(cdf, total, last, [u[0]])[0])
        cell = (v % nx, (v // nx) % ny, v // (nx * ny))
        for a, (c, m, na) in enumerate(zip(cell, (xmax, ymax, zmax), (nx, ny, nz))):
            f0, f1 = c * 2.0 * m / na, (c + 1) * 2.0 * m / na
            q = f0 + u[1 + a] * (f1 - f0)
            x = q - m
            if x == -m:
                x = x + 7.9e-7
            elif x == m:
                x = x - 7.9e-7
            pos[p, a] = x
        phi = u[4] * 6.283185307179586
        sn, cs = O.sincos(phi)
        cost = 2.0 * u[5] - 1.0
        sint = math.sqrt(1.0 - cost * cost)
        d[p] = (sint * cs, sint * sn, cost)
        vox[p] = v
    return pos, d, vox


# ---- 1. exports, Fortran text ------------------------------------------------------------------------
def test_exports_and_version(lib_path, L):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for fn in FUNCTIONS:
        assert fn in exported, fn
        assert fn in abi.EXPORTED_SYMBOLS, fn
    assert L.smcrt_abi_version() == 5 == abi.SMCRT_ABI_VERSION  # (additive: the version stays)
    assert abi.SRC_VOLUME == 10 and scene.volume_source().kind == 10
    assert abi.SRC_VOLUME not in abi.SOURCE_KINDS.values()  # (no job file names it)


def test_header_value(tmp_path):
    src = tmp_path / "kind.c"
    src.write_text(f'#include <stdio.h>\n#include "{os.path.join(ROOT, "include", "smcrt.h")}"\n'
                   'int main(void){printf("%d %d %zu\\n", (int)SMCRT_SRC_VOLUME, (int)SMCRT_ABI_VERSION, '
                   'sizeof(smcrt_source));return 0;}')
    exe = tmp_path / "kind"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    kind, ver, size = map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert (kind, ver) == (10, 5) and size == C.sizeof(abi.Source)


def test_fortran_module_has_the_interfaces():
    low = re.sub(r"&\s*\n\s*", " ", open(FORTRAN).read().lower())
    assert re.search(r"smcrt_src_volume\s*=\s*10\b", low)
    assert re.search(r"smcrt_mod_abi_version\s*=\s*5\b", low)
    for fn in FUNCTIONS[:2]:
        assert re.search(rf'function {fn}\(.*?\)\s*bind\(c,\s*name="{fn}"\)', low), fn
        assert f"end function {fn}" in low, fn


# ---- 2. refusals before the device ---------------------------------------------------------------
BAD = [("nan", 7, float("nan"), r"voxel 7\b.*not finite"), ("inf", 59, float("inf"), r"voxel 59\b.*not finite"),
       ("-inf", 0, -float("inf"), r"voxel 0\b.*not finite"), ("negative", 3, -1e-300, r"voxel 3\b.*negative")]


@pytest.mark.parametrize("name,index,value,pattern", BAD, ids=[b[0] for b in BAD])
def test_bad_weight_names_the_index(L, name, index, value, pattern):
    w = np.ones(60)
    w[index] = value
    w[min(index + 5, 59)] = value  # (a later offender: the first one is named)
    u, out = np.zeros(1), np.zeros(1, dtype=np.int64)
    assert L.smcrt_volume_pick(_dp(w), 60, _dp(u), 1, _ip(out)) == abi.ERR_INVALID_ARG
    assert re.search(pattern, last_error(L)), last_error(L)
    g = scene.grid(*GRID_543)
    assert L.smcrt_volume_sample(_dp(w), C.byref(g), SEED, 0, 1, None, None, _ip(out)) == abi.ERR_INVALID_ARG
    assert re.search(pattern, last_error(L)), last_error(L)


def test_all_zero_and_overflow(L):
    u, out = np.zeros(1), np.zeros(1, dtype=np.int64)
    w = np.zeros(60)
    assert L.smcrt_volume_pick(_dp(w), 60, _dp(u), 1, _ip(out)) == abi.ERR_INVALID_ARG
    assert re.search(r"every weight is zero.*voxel 0 \.\. 59", last_error(L)), last_error(L)
    w = np.zeros(60)
    w[[4, 9, 11]] = 1.0e308  # finite each; the running sum leaves fp64 at the second
    assert L.smcrt_volume_pick(_dp(w), 60, _dp(u), 1, _ip(out)) == abi.ERR_INVALID_ARG
    assert re.search(r"overflows at voxel 9\b", last_error(L)), last_error(L)
    assert L.smcrt_volume_pick(_dp(np.ones(1)), 0, _dp(u), 1, _ip(out)) == abi.ERR_INVALID_ARG
    bad_u = np.array([0.25, 1.0])
    assert L.smcrt_volume_pick(_dp(np.ones(4)), 4, _dp(bad_u), 2, _ip(np.zeros(2, dtype=np.int64))) == abi.ERR_INVALID_ARG
    assert "uniform 1" in last_error(L)


def test_null_scene_and_null_weights(L):
    w = np.ones(60)
    assert L.smcrt_scene_set_volume_source(None, _dp(w)) == abi.ERR_INVALID_ARG
    assert "scene is NULL" in last_error(L)
    assert L.smcrt_scene_volume_source_info(None, None, None, None) == abi.ERR_INVALID_ARG
    g = scene.grid(*GRID_543)
    assert L.smcrt_volume_sample(None, C.byref(g), SEED, 0, 1, None, None, None) == abi.ERR_INVALID_ARG
    assert L.smcrt_volume_sample(_dp(w), None, SEED, 0, 1, None, None, None) == abi.ERR_INVALID_ARG
    assert L.smcrt_volume_pick(None, 60, None, 0, None) == abi.ERR_INVALID_ARG


def test_job_layer_never_produces_the_kind(lib_path, tmp_path):
    """A kind-10 source through the one scene-free path that makes sources: a job file cannot name it."""
    from rsmcrt_amd import job
    text = open(os.path.join(ROOT, "tests", "golden", "res", "scat_test.toml")).read()
    assert 'name = "point"' in text
    path = tmp_path / "volume.toml"
    path.write_text(text.replace('name = "point"', 'name = "volume"', 1))
    with pytest.raises(Exception, match="INVALID_ARG"):
        job.Job(str(path))
    assert "volume" not in abi.SOURCE_KINDS


# ---- 3. the pick ---------------------------------------------------------------------------------
def check_pick(L, w, u):
    cdf, total, last = seq_cdf(w)
    got = pick(L, w, u)
    want = np_pick(cdf, total, last, u)
    assert np.array_equal(got, want), (got, want)
    assert np.all(np.asarray(w)[got] > 0.0)
    return got


TOP = 1.0 - 2.0 ** -53


def test_pick_edges_on_60_voxels(L):
    w = weights_for((5, 4, 3), seed=11)
    w[[0, 1, 58, 59]] = 0.0  # leading and trailing zeros
    assert np.count_nonzero(w == 0.0) > 8 and np.count_nonzero(w) > 30
    cdf, total, last = seq_cdf(w)
    assert last == np.flatnonzero(w)[-1] < 58
    got = check_pick(L, w, [0.0, TOP])
    assert got[0] == np.flatnonzero(w)[0] == np.flatnonzero(cdf > 0.0)[0]
    assert got[1] == last  # (the clamp goes to `last`, not to nvox - 1)
    # u exactly at every cdf[i] / total, and its neighbours
    edges = cdf / total
    u = np.concatenate([edges, np.nextafter(edges, 0.0), np.nextafter(edges, 2.0)])
    u = u[(u >= 0.0) & (u < 1.0)]
    check_pick(L, w, u)
    check_pick(L, w, np.random.default_rng(5).uniform(size=4000))


def test_pick_at_the_top_of_the_range(L):
    """The largest uniform, 1 - 2^-53, over many totals. Its product with `total` lies at least half
    an ulp below `total` (exactly one ulp below when total is a power of two), so in fp64 it does
    not round up to it and the bisection itself ends on `last`; the clamp to `last` is a guard, and
    with trailing zeros both give `last`, never nvox - 1."""
    rng = np.random.default_rng(3)
    for k in range(200):
        w = np.zeros(60)
        w[rng.integers(5, 50, 6)] = rng.uniform(0.1, 3.0, 6) if k % 4 else 2.0 ** rng.integers(-3, 4, 6)
        cdf, total, last = seq_cdf(w)
        assert TOP * total < total
        assert pick(L, w, [TOP])[0] == last == np.flatnonzero(w)[-1] < 59


@pytest.mark.parametrize("index", [0, 59])
def test_pick_single_positive_voxel(L, index):
    w = np.zeros(60)
    w[index] = 2.5
    got = check_pick(L, w, [0.0, 0.5, TOP])
    assert np.all(got == index)


def test_pick_single_voxel_grid(L):
    assert np.all(check_pick(L, [3.0], [0.0, 0.3, TOP]) == 0)


def test_weight_that_vanishes_against_its_prefix(L):
    w = np.zeros(60)
    w[2], w[3], w[40] = 1e30, 1e-30, 1e-30
    cdf, total, last = seq_cdf(w)
    assert cdf[3] == cdf[2] and last == 2 and total == 1e30
    got = check_pick(L, w, np.concatenate([[0.0, TOP], np.random.default_rng(1).uniform(size=1000)]))
    assert np.all(got == 2)


# ---- 4. the sampler, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("dims", [GRID_543, GRID_888], ids=["5x4x3", "8x8x8"])
def test_sampler_equals_the_restated_rule(L, dims):
    w = weights_for(dims[:3], seed=dims[0])
    n, first = 2000, 3
    pos, d, vox = sample(L, w, scene.grid(*dims), n, first=first)
    rpos, rd, rvox = np_sample(w, dims, n, first=first)
    assert np.array_equal(vox, rvox)
    assert np.array_equal(pos, rpos)  # (== on fp64: bit for bit up to the sign of zero, which cannot occur off the walls)
    assert np.array_equal(d, rd)
    # a shard of the same run is the same photons
    p2, d2, v2 = sample(L, w, scene.grid(*dims), 100, first=first + 500)
    assert np.array_equal(p2, pos[500:600]) and np.array_equal(d2, d[500:600]) and np.array_equal(v2, vox[500:600])
    # and every position lies in its voxel
    nx, ny, nz = dims[:3]
    for a, (na, m) in enumerate(zip((nx, ny, nz), dims[3:])):
        cell = (vox % nx, (vox // nx) % ny, vox // (nx * ny))[a]
        lo, hi = cell * 2.0 * m / na - m, (cell + 1) * 2.0 * m / na - m
        assert np.all(pos[:, a] >= lo - 1e-15) and np.all(pos[:, a] <= hi + 1e-15)


def test_nudge_off_the_outer_walls():
    """u = 0 in the first cell puts q on the grid's wall: the emitters' nudge moves it inside."""
    m, na = 0.75, 4
    f0, f1 = 0 * 2.0 * m / na, 1 * 2.0 * m / na
    x = (f0 + 0.0 * (f1 - f0)) - m
    assert x == -m  # the restatement's branch, which np_sample shares with the library, is reachable


# ---- 5. statistics -------------------------------------------------------------------------------
def test_sampler_statistics(L):
    dims = GRID_543
    w = weights_for(dims[:3], seed=23)
    n = 100_000
    _, d, vox = sample(L, w, scene.grid(*dims), n, seed=987654321)
    counts = np.bincount(vox, minlength=60)
    assert np.all(counts[w == 0.0] == 0)
    pos_w = w > 0.0
    expect = n * w[pos_w] / w.sum()
    assert expect.min() > 100
    chi2 = float(((counts[pos_w] - expect) ** 2 / expect).sum())
    dof = int(pos_w.sum()) - 1
    print(f"chi2 {chi2:.1f}, dof {dof}, bound {dof + 6 * math.sqrt(2 * dof):.1f}")
    assert chi2 <= dof + 6.0 * math.sqrt(2.0 * dof)  # six sigma of a chi-squared variable
    norm = np.sqrt((d * d).sum(axis=1))
    assert np.all(np.abs(norm - 1.0) <= 4 * np.finfo(np.float64).eps), float(np.abs(norm - 1.0).max())
    mean = d.mean(axis=0)
    print("mean direction", mean, "bound", 6.0 / math.sqrt(3 * n))
    assert np.all(np.abs(mean) <= 6.0 / math.sqrt(3 * n))  # var of a component of an isotropic unit vector: 1/3


# ---- 6. fluorescence(): weights and restore, against a stub engine -------------------------------
class StubResult:
    def __init__(self, absorb):
        self.absorb = absorb


class StubEngine:
    """Three layers stacked in z on a 4 x 3 x 6 grid (two voxel planes each), the calls fluorescence() makes."""

    def __init__(self, fail_emission=False):
        self.grid = scene.grid(4, 3, 6, 1.0, 1.0, 1.5)
        self.props = {0: (1, 10.0, 0.5, 0.9, 1.33), 1: (2, 20.0, 1.5, 0.8, 1.4), 2: (3, 5.0, 0.25, 0.0, 1.0)}
        self.absorb = np.random.default_rng(2).uniform(0.0, 3.0, (6, 3, 4))
        self.table, self.log, self.fail_emission = None, [], fail_emission

    def run(self, source, n, seed=0, flags=0):
        self.log.append(("run", source.kind, n, seed, flags, dict(self.props)))
        if source.kind == abi.SRC_VOLUME:
            if self.fail_emission:
                raise RuntimeError("emission run failed")
            return StubResult(np.zeros((6, 3, 4)))
        return StubResult(self.absorb.copy())

    def classify(self, pts):
        z = np.asarray(pts)[:, 2]
        return (np.floor((z + 1.5) / 1.0).astype(np.int32) + 1), np.zeros(len(pts))

    def set_volume_source(self, w):
        self.table = None if w is None else np.array(w, copy=True)

    def get_optprops(self, top):
        return self.props[top]

    def set_optprops(self, top, mus, mua, hgg, n):
        self.props[top] = (self.props[top][0], mus, mua, hgg, n)


def test_fluorescence_weights():
    eng = StubEngine()
    before = dict(eng.props)
    src = scene.pencil_source((0, 0, 1.4), (0, 0, -1))
    out = F.fluorescence(eng, src, 1000, 400, {2: 0.25}, emission_props={1: (7.0, 0.1, 0.5, 1.4)}, seed=42)
    want = np.zeros((6, 3, 4))
    want[2:4] = eng.absorb[2:4] * 0.25  # layer 2 = the middle two planes
    assert np.array_equal(out.weights, want) and np.array_equal(eng.table, want)
    assert out.per_excitation_photon == want.sum() / (1000.0 * 400.0)
    ex, em = eng.log
    assert ex[1:4] == ("run", abi.SRC_PENCIL, 1000, 42)[1:] and em[1:4] == (abi.SRC_VOLUME, 400, 43)
    assert ex[5] == before and em[5][1] == (2, 7.0, 0.1, 0.5, 1.4) and em[5][0] == before[0]
    assert eng.props == before  # put back
    # a sequence is indexed by layer - 1; layers past its end yield nothing
    w2 = F.emission_weights(eng.absorb, eng.classify(F.voxel_centres(eng.grid))[0], [0.0, 0.5])
    assert np.array_equal(w2[2:4], eng.absorb[2:4] * 0.5) and not w2[:2].any() and not w2[4:].any()
    with pytest.raises(ValueError):
        F.emission_weights(eng.absorb, np.ones(72, dtype=np.int32), {1: -1.0})


def test_fluorescence_restores_when_the_emission_run_raises():
    eng = StubEngine(fail_emission=True)
    before = dict(eng.props)
    with pytest.raises(RuntimeError, match="emission run failed"):
        F.fluorescence(eng, scene.point_source(), 10, 10, {2: 1.0}, emission_props={0: (1.0, 2.0, 0.0, 1.0), 2: (3.0, 4.0, 0.1, 1.1)})
    assert eng.log[-1][5][0][1:] == (1.0, 2.0, 0.0, 1.0) and eng.log[-1][5][2][1:] == (3.0, 4.0, 0.1, 1.1)
    assert eng.props == before


def test_voxel_centres_order():
    g = scene.grid(4, 3, 6, 1.0, 1.0, 1.5)
    c = F.voxel_centres(g)
    assert c.shape == (72, 3)
    assert np.allclose(c[0], (-0.75, -1 + 1 / 3, -1.25)) and np.allclose(c[1] - c[0], (0.5, 0, 0))  # x fastest
    assert np.allclose(c[4] - c[0], (0, 2 / 3, 0)) and np.allclose(c[12] - c[0], (0, 0, 0.5))
