"""Test infrastructure only: the scenes of DESIGN.md §3.5 in their three forms (SDF, voxel, mesh),
their closed-form expectations (tests/analytic_ref.py) and the statistics that compare a run with
them. Shared by tests/test_analytic_cpu.py and tests/test_gpu_analytic.py, and for the detector
cases (below the grids') by tests/test_detectors_analytic_cpu.py and
tests/test_gpu_detectors_analytic.py; runs neither the engine nor the restatements, so that what
is compared with what stays in the tests. The scattering-medium cases (S) and the curved-surface
cases (D: a glass sphere on this same grid, in SDF, table and mesh form; no voxel form, a label
volume has no curved surface) follow at the end.

The grid has three different voxel edges (0.25, 0.125, 0.24) and three different counts, so a
swapped axis or stride cannot pass; the slab's planes z = +-0.48 are voxel faces.
"""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy import stats

from rsmcrt_amd import builders, scene
from tests import analytic_ref as AR

NX, NY, NZ = 8, 12, 10
HALF = (1.0, 0.75, 1.2)
EDGES = tuple(2.0 * h / n for h, n in zip(HALF, (NX, NY, NZ)))
DIAG = math.sqrt(sum(e * e for e in EDGES))  # no photon leaves more track than this in one crossing
Z_HALF = 0.48                                # faces 3 and 7 of the 11 z faces
K_SLAB = slice(3, 7)
# A mesh scene takes no step off a surface it has crossed (DESIGN.md §7 "Mesh media"): a leg that
# starts on a surface lying in a voxel wall finds its position and its cell on different sides of
# that wall, which is the reference's error stop (a counted fault), for every photon. The mesh
# form's planes therefore lie 1e-6 inside the walls, and its reference is computed for them. In
# scene C that leaves 1e-6 / 0.24 of the two voxel layers next to a plane in the other medium.
MESH_INSET = 1e-6
N_VOXELS = NX * NY * NZ
SEED = 123456789
BATCHES = 24
ALPHA = 1e-3   # family-wise false-alarm rate of one test, shared equally by its statistics
MIN_EVENTS = 100.0
FORMS = ("sdf", "voxel", "mesh")

# scene A
A_MU = 2.0
A_SRC = (0.09, -0.05, 0.10)
# scene B
B_N_IN, B_MU = 1.5, 2.0
B_ORIGIN = (-0.62, 0.13, 0.93)
B_DIR = (0.5, 0.2, -0.84)
B_POOL_CAP = 1e-3
# The engine moves a photon 1e-8 past every voxel wall and 2e-8 past every surface it crosses
# (update_pos, tauint2), so a track can be short by a few 1e-8 / |direction component| per voxel.
# Where every photon deposits the same chord the batch variance is zero and this is all there is:
# 1e-6 per photon and voxel bounds it (three walls, components above 0.1) and is added to the
# standard error of scene B's tracks. In those voxels it is the whole denominator: an absolute
# tolerance of 1e-6 per photon (1e-5 of the track), not a t test. In the stochastic voxels the
# standard error is about ten times larger at 2e7 photons.
B_TRACK_SLOP = 1e-6
# (Scene D, whose surfaces are curved, derives its slop from the same rule leg by leg: see
# D_EPS_SURFACE and d_slop() in the curved-surface section below.)
# scene C
C_IN = (6.0, 0.8, 0.7, 1.4)    # mus, mua, g, n of the slab
C_OUT = (2.5, 0.4, 0.3, 1.0)
C_SRC = (0.09, -0.05, 0.10)
C_POOL_CAP = 0.05


def grid():
    return scene.grid(NX, NY, NZ, *HALF)


def faces():
    return AR.faces(NX, HALF[0]), AR.faces(NY, HALF[1]), AR.faces(NZ, HALF[2])


def z_half(form):
    return Z_HALF - MESH_INSET if form == "mesh" else Z_HALF


# ------------------------------------------------------------------------------ scenes ----
def _layered(form, inner, outer):
    """A slab |z| < Z_HALF of `inner` in `outer`, both wider than the grid."""
    if form == "sdf":
        return scene.Scene([scene.box((20.0, 20.0, 2.0 * Z_HALF), inner, 1), scene.box((40.0, 40.0, 40.0), outer, 2)])
    if form == "voxel":
        lab = np.zeros((NX, NY, NZ), dtype=np.uint8)
        lab[:, :, K_SLAB] = 1
        return scene.VoxelScene(lab, [outer, inner])
    ms = scene.MeshScene([inner, outer], ambient=1)
    zh = z_half("mesh")
    return ms.add_surface(*builders.box_mesh((-10.0, -10.0, -zh), (10.0, 10.0, zh)), 0, 1)


def scene_a(form):
    """(scene, source): a homogeneous absorber, mus = 0 and mua = A_MU, around a point source."""
    m = scene.mono(0.0, A_MU, 0.0, 1.0)
    src = scene.point_source(A_SRC)
    if form == "sdf":
        return scene.Scene([scene.box((20.0, 20.0, 20.0), m, 1)]), src
    if form == "voxel":
        return scene.VoxelScene(np.zeros((NX, NY, NZ), dtype=np.uint8), [m]), src
    ms = scene.MeshScene([m, m], ambient=1)  # one box far beyond the grid; the same medium around it
    return ms.add_surface(*builders.box_mesh((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0)), 0, 1), src


def scene_b(form):
    """(scene, source): an oblique pencil beam through an absorbing slab of n = 1.5 in vacuum."""
    d = np.array(B_DIR) / math.sqrt(sum(c * c for c in B_DIR))
    return (_layered(form, scene.mono(0.0, B_MU, 0.0, B_N_IN), scene.mono(0.0, 0.0, 0.0, 1.0)),
            scene.pencil_source(B_ORIGIN, tuple(d)))


def scene_c(form):
    """(scene, source): B's layers with scattering in both media, a point source inside the slab."""
    return _layered(form, scene.mono(*C_IN), scene.mono(*C_OUT)), scene.point_source(C_SRC)


def mua_c():
    """mua of every voxel of scene C, (nz, ny, nx)."""
    m = np.full((NZ, NY, NX), C_OUT[1])
    m[K_SLAB] = C_IN[1]
    return m


# -------------------------------------------------------------------------- references ----
def swapped(a, axes):
    """The grid `a` stored with two axes exchanged ("xy", "xz" or "yz") and read as (nz, ny, nx):
    what a swapped stride does. For the negative controls only."""
    order = {"xy": (0, 2, 1), "xz": (2, 1, 0), "yz": (1, 0, 2)}[axes]
    return np.ascontiguousarray(a.transpose(order)).reshape(NZ, NY, NX)


@functools.lru_cache(maxsize=None)
def reference_a(mu=A_MU, src=A_SRC, swap=None):
    """(T, p): expected track and absorption probability per photon and voxel. mu, src and swap
    (two axes exchanged, see `swapped`) are varied only by the negative controls."""
    t = AR.point_source_track(*faces(), src, mu)
    if swap:
        t = swapped(t, swap)
    return t, mu * t


@functools.lru_cache(maxsize=None)
def reference_b(form="sdf", n_in=B_N_IN, polarisation="unpolarised", mu=B_MU, origin=B_ORIGIN, swap=None):
    """(T, p) of scene B in `form`; the other arguments are varied only by the negative controls."""
    t, p = AR.beam_slab(*faces(), origin, B_DIR, z_half(form), n_in, mu, polarisation=polarisation)
    if swap:
        t, p = swapped(t, swap), swapped(p, swap)
    return t, p


# -------------------------------------------------------------------------- statistics ----
def run_batches(run, n_batch, batches=BATCHES):
    """`run(first_photon, n)` -> Result for each of `batches` disjoint photon ranges of one seed:
    (jmean per batch [B, nz, ny, nx], absorb per batch, summed counters as a dict)."""
    jm, ab, ctr = [], [], {}
    for b in range(batches):
        r = run(b * n_batch, n_batch)
        jm.append(r.jmean.copy())
        ab.append(r.absorb.copy())
        for k, v in r.counters_dict().items():
            ctr[k] = ctr.get(k, 0) + v
    return np.array(jm), np.array(ab), ctr


def _bins(expected_events):
    """Every entry with at least MIN_EVENTS expected events is a bin of its own; those with fewer
    (and more than none) are summed into one pooled bin. Returns (index arrays of the bins, the
    pooled index array or None)."""
    e = expected_events.ravel()
    own = np.flatnonzero(e >= MIN_EVENTS)
    pooled = np.flatnonzero((e > 0.0) & (e < MIN_EVENTS))
    return own, (pooled if pooled.size else None)


def count_stats(counts, p, n, alpha):
    """Multinomial counts against probabilities p: each photon falls into at most one voxel, so a
    bin holds Binomial(n, p_v): z_v = (count - n p_v) / sqrt(n p_v (1 - p_v)). Returns a dict with
    max|z|, sum z^2, the number of bins V, the pooled share of the expectation and the bounds:
    `alpha` is shared by two statistics: max|z| over V bins must stay below the two-sided normal
    quantile at alpha / (2 * 2 V) each, and sum z^2 inside the chi^2_V quantiles at alpha / 4 on
    either side (p_v << 1 makes the bins independent to that order)."""
    c, q = np.asarray(counts, dtype=np.float64).ravel(), np.asarray(p, dtype=np.float64).ravel()
    own, pooled = _bins(n * q)
    cc, qq = c[own], q[own]
    if pooled is not None:
        cc, qq = np.append(cc, c[pooled].sum()), np.append(qq, q[pooled].sum())
    z = (cc - n * qq) / np.sqrt(n * qq * (1.0 - qq))
    v = len(z)
    a = alpha / 2.0
    return {"max_z": float(np.abs(z).max()), "chi2": float((z * z).sum()), "bins": v,
            "n_pooled": 0 if pooled is None else int(pooled.size),
            "pooled_share": 0.0 if pooled is None else float(q[pooled].sum() / q.sum()),
            "z_bound": float(stats.norm.isf(a / (2.0 * v))),
            "chi2_lo": float(stats.chi2.ppf(a / 2.0, v)), "chi2_hi": float(stats.chi2.isf(a / 2.0, v))}


def binomial_z(count, p, n):
    """z of a Binomial(n, p) count; |z| is held below binomial_bound(alpha)."""
    return (count - n * p) / math.sqrt(n * p * (1.0 - p))


def binomial_bound(alpha):
    return float(stats.norm.isf(alpha / 2.0))


MEAN_T2_DRAWS = 1_000_000
MEAN_T2_NORMAL_BINS = 200


@functools.lru_cache(maxsize=None)
def mean_t2_bounds(v, nu, a_side):
    """The quantiles at a_side and 1 - a_side of the mean of v independent squares of Student-t
    variables with nu degrees of freedom. From MEAN_T2_NORMAL_BINS bins on: normal, with mean
    nu / (nu - 2) and variance 2 nu^2 (nu - 1) / ((nu - 2)^2 (nu - 4) v), the moments of F(1, nu).
    Below (scene B's few dozen bins, where the heavy tail of t^2 makes a normal quantile far too
    small): the empirical quantiles of MEAN_T2_DRAWS draws from a fixed seed."""
    if v >= MEAN_T2_NORMAL_BINS:
        m = nu / (nu - 2.0)
        sd = math.sqrt(2.0 * nu * nu * (nu - 1.0) / ((nu - 2.0) ** 2 * (nu - 4.0) * v))
        z = float(stats.norm.isf(a_side))
        return m - z * sd, m + z * sd
    rng = np.random.default_rng(1234567)
    chunk = 100_000
    means = np.concatenate([(rng.standard_t(nu, size=(chunk, v)) ** 2).mean(axis=1)
                            for _ in range(MEAN_T2_DRAWS // chunk)])
    return float(np.quantile(means, a_side)), float(np.quantile(means, 1.0 - a_side))


def batch_stats(samples, expected, events, alpha, slop=0.0):
    """Batch means against an expectation: samples [B, ...] per batch, expected [...] per batch,
    events [...] the expected number of contributing photons over all batches (the pooling rule of
    count_stats). t_v = (mean_v - expected_v) / sqrt(s_v^2 / B + slop^2) is Student-t with B - 1
    degrees of freedom when slop = 0 (slop: a bound on a systematic error per bin, which the sum
    takes once per bin). The grid's sum is one more statistic. `alpha` is shared by four
    statistics: max|t| over V bins below the two-sided t quantile at alpha / (4 * 2 V); the mean of
    t_v^2 inside the quantiles, at alpha / 8 on either side, of the mean of V independent squares
    of Student-t variables (mean_t2_bounds: too small a value, an overestimated variance, fails as
    too large a one does; photons shared by the voxels on one ray correlate the bins, which widens
    the true spread, so the bounds err to the strict side); as an extra check each t_v mapped to
    the chi^2_1 value of the same tail probability, q_v = chi2_1.isf(2 t_nu.sf(|t_v|)), whose sum
    is chi^2_V and must stay below its quantile at alpha / 4; and |t| of the sum below the t
    quantile at alpha / (4 * 2). "pooled_share" is the pooled bins' share of the expectation."""
    s = np.asarray(samples, dtype=np.float64).reshape(len(samples), -1)
    e = np.asarray(expected, dtype=np.float64).ravel()
    own, pooled = _bins(np.asarray(events, dtype=np.float64))
    x, m = s[:, own], e[own]
    if pooled is not None:
        x, m = np.hstack([x, s[:, pooled].sum(axis=1, keepdims=True)]), np.append(m, e[pooled].sum())
    b = x.shape[0]
    nu = b - 1

    def tstat(col, want, tol):
        return (col.mean(axis=0) - want) / np.sqrt(col.var(axis=0, ddof=1) / b + tol * tol)

    t = tstat(x, m, slop)
    used = np.concatenate([own, pooled]) if pooled is not None else own
    t_sum = float(tstat(s[:, used].sum(axis=1), e[used].sum(), slop * len(used)))
    v = len(t)
    a = alpha / 4.0
    q = stats.chi2.isf(2.0 * stats.t.sf(np.abs(t), nu), 1)
    lo, hi = mean_t2_bounds(v, nu, a / 2.0)
    total = float(e.sum())
    return {"max_t": float(np.abs(t).max()), "mean_t2": float((t * t).mean()), "score": float(q.sum()),
            "t_sum": t_sum, "bins": v, "n_pooled": 0 if pooled is None else int(pooled.size),
            "pooled_share": float(e[pooled].sum() / total) if pooled is not None and total > 0.0 else 0.0,
            "t_bound": float(stats.t.isf(a / (2.0 * v), nu)), "mean_t2_lo": lo, "mean_t2_hi": hi,
            "score_bound": float(stats.chi2.isf(a, v)), "t_sum_bound": float(stats.t.isf(a / 2.0, nu))}


def check_counts(st):
    assert st["max_z"] <= st["z_bound"], st
    assert st["chi2_lo"] <= st["chi2"] <= st["chi2_hi"], st


def check_batches(st):
    assert st["max_t"] <= st["t_bound"], st
    assert st["mean_t2_lo"] <= st["mean_t2"] <= st["mean_t2_hi"], st
    assert st["score"] <= st["score_bound"], st
    assert abs(st["t_sum"]) <= st["t_sum_bound"], st


# ----------------------------------------------------------------- what a test asserts ----
def evaluate_ab(which, jm, ab, ctr, n_batch, ref, slop=None):
    """Scenes A and B (and D, which names its own `slop` per photon and voxel and is held to B's
    pooling rule): a run in batches (run_batches) against ref = (T, p). ALPHA is shared by three
    groups: the absorb counts (count_stats), the absorbed and escaped counters (one binomial: they
    sum to N) and the tracks (batch_stats). A voxel's track has at least N T_v / DIAG contributing
    photons, none of which leaves more than the voxel's diagonal: that is its event count."""
    t, p = ref
    n = n_batch * len(jm)
    a = ALPHA / 3.0
    if slop is None:
        slop = B_TRACK_SLOP if which == "b" else 0.0
    return {"which": which, "n": n,
            "counts": count_stats(ab.sum(axis=0), p, n, a),
            "z_absorbed": binomial_z(ctr["absorbed"], p.sum(), n),
            "z_escaped": binomial_z(ctr["escaped"], 1.0 - p.sum(), n), "z_bound": binomial_bound(a),
            "tracks": batch_stats(jm, n_batch * t, n * t / DIAG, a, slop=n_batch * slop),
            "absorb_off_support": float(ab.sum(axis=0)[p == 0.0].sum()),
            "jmean_off_support": float(jm.sum(axis=0)[t == 0.0].sum()),
            "faults": ctr.get("faults", 0), "lost": n - ctr["absorbed"] - ctr["escaped"]}


def check_ab(st):
    """The assertions of scenes A and B on evaluate_ab's statistics."""
    assert st["faults"] == 0 and st["lost"] == 0, st
    assert st["absorb_off_support"] == 0.0 and st["jmean_off_support"] == 0.0, st
    for group in ("counts", "tracks"):  # the pooling rule's conditions, on absorptions and on tracks
        if st["which"] == "a":
            assert st[group]["n_pooled"] == 0 and st[group]["bins"] == N_VOXELS, st[group]
        else:
            assert st[group]["pooled_share"] < B_POOL_CAP, st[group]
    check_counts(st["counts"])
    assert abs(st["z_absorbed"]) <= st["z_bound"] and abs(st["z_escaped"]) <= st["z_bound"], st
    check_batches(st["tracks"])


def evaluate_c(jm, ab, ctr, mua=None):
    """Scene C: d = mua(v) jmean[v] - absorb[v] per batch has expectation zero in every voxel (the
    track-length and the collision estimator of absorption). Voxels in which both estimators saw
    fewer than MIN_EVENTS events over all batches (absorptions; tracks, at least jmean / DIAG of
    them) are pooled."""
    mua = mua_c() if mua is None else mua
    d = mua[None] * jm - ab
    events = np.maximum(ab.sum(axis=0), jm.sum(axis=0) / DIAG)
    st = batch_stats(d, np.zeros_like(mua), events, ALPHA)
    st["faults"] = ctr.get("faults", 0)
    st["absorb_sum"], st["track_sum"] = float(ab.sum()), float((mua[None] * jm).sum())
    return st


def check_c(st):
    assert st["faults"] == 0, st
    assert st["n_pooled"] <= C_POOL_CAP * N_VOXELS, st
    check_batches(st)


# ----------------------------------------------------------------------- detector cases ----
# The detector bins of the same scenes against tests/analytic_ref.py. A photon of
# scenes A and B meets one detector at most once, so a detector's bins are multinomial counts and
# its total is binomial.
def _unit(v):
    ln = math.sqrt(sum(c * c for c in v))
    return tuple(c / ln for c in v)


def _inside_grid(points, slack=0.0):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return bool(np.all(np.abs(p) < np.array(HALF) - slack))


def _disc_inside_grid(centre, normal, radius):
    """The disc's extent along axis a is radius * sqrt(1 - n_a^2)."""
    n = np.array(_unit(normal))
    return bool(np.all(np.abs(np.array(centre)) + radius * np.sqrt(1.0 - n * n) < np.array(HALF)))


# D-A: circle, camera, annulus, fibre, the circle again with its normal flipped. The normal has
# three different components, the centres are off the source's foot, the planes lie 0.3 to 0.4
# from A_SRC (exp(-mu s) is about 0.45 there: a missing `t <= pointSep` window doubles the counts).
DA_NORMAL = _unit((0.3, -0.2, 0.93))
DA_CENTRE, DA_RADIUS, DA_NBINS = (0.35, -0.11, 0.38), 0.3, 8
DA_ANN_CENTRE, DA_ANN = (0.15, -0.18, 0.40), (0.1, 0.28, 9)    # r1, r2, nbins
# the camera: a rectangle below the source whose normal e2 x e1 points away from it; five pixels
# a side, so that its 25 bins stand before the annulus', the fibre's and the flipped circle's
DA_CAM_P1, DA_CAM_E1, DA_CAM_E2 = (0.05, -0.15, -0.30), (0.3, -0.025, 0.1), (0.0, 0.4, 0.1)
DA_CAM_NBINS, DA_CAM_MAXVAL = 4, 0.55
# the fibre: its axis passes through A_SRC, the front lens 0.3 away, which is off the focus of the
# front lens (f1 = 0.1): radius-at-the-fibre = a r with a = -0.533, several bins fill and the last
# takes what the clamp sends there. The radius is negative at the pinhole, the back lens and the
# fibre, so those three signed limits never bind; the acceptance angle sets r_max = 0.0402.
DA_FIBRE_AXIS, DA_FIBRE_H, DA_FIBRE_NBINS = _unit((-0.6, 0.5, -0.62)), 0.3, 6
DA_FIBRE = dict(focal1=0.1, focal2=0.1, f1_aperture=0.05, f2_aperture=0.02, front_offset=0.02, back_offset=0.12,
                front_to_pin=0.25, pin_to_back=0.1, pin_aperture=0.01, accept_angle=15.0, core_diameter=0.03)


def _fibre_pos():
    """The fibre's `pos`: the front lens is front_offset further along the axis."""
    return tuple(s + (DA_FIBRE_H - DA_FIBRE["front_offset"]) * a for s, a in zip(A_SRC, DA_FIBRE_AXIS))


def _fibre_front():
    return tuple(s + DA_FIBRE_H * a for s, a in zip(A_SRC, DA_FIBRE_AXIS))


def _fibre_f():
    d = DA_FIBRE
    return [d["focal1"], d["focal2"], d["f1_aperture"], d["f2_aperture"], d["front_offset"], d["back_offset"],
            d["front_to_pin"], d["pin_to_back"], d["pin_aperture"], d["accept_angle"], d["core_diameter"]]


def dets_a():
    r1, r2, nb = DA_ANN
    p1 = np.array(DA_CAM_P1)
    flipped = tuple(-c for c in DA_NORMAL)
    assert _disc_inside_grid(DA_CENTRE, DA_NORMAL, DA_RADIUS) and _disc_inside_grid(DA_ANN_CENTRE, DA_NORMAL, r2)
    assert _disc_inside_grid(_fibre_front(), DA_FIBRE_AXIS, DA_FIBRE["f1_aperture"])
    assert _inside_grid([p1, p1 + DA_CAM_E1, p1 + DA_CAM_E2, p1 + DA_CAM_E1 + DA_CAM_E2])
    for c in (DA_CENTRE, DA_ANN_CENTRE):
        h = sum((a - b) * n for a, b, n in zip(c, A_SRC, DA_NORMAL))
        off = math.sqrt(sum((a - b) ** 2 for a, b in zip(c, A_SRC)) - h * h)
        assert 0.3 < h < 0.4 and off > 0.05, (h, off)
    return [scene.circle_dect(DA_CENTRE, DA_NORMAL, 1, DA_RADIUS, DA_NBINS),
            scene.camera(DA_CAM_P1, tuple(p1 + DA_CAM_E1), tuple(p1 + DA_CAM_E2), 1, DA_CAM_NBINS, DA_CAM_MAXVAL),
            scene.annulus_dect(DA_ANN_CENTRE, DA_NORMAL, 1, r1, r2, nb),
            scene.fibre_dect(_fibre_pos(), DA_FIBRE_AXIS, 1, DA_FIBRE_NBINS, **DA_FIBRE),
            scene.circle_dect(DA_CENTRE, flipped, 1, DA_RADIUS, DA_NBINS)]


@functools.lru_cache(maxsize=None)
def expected_a(control=None):
    """The probability per photon of every bin of dets_a(), one array per detector. `control`
    names a reference that is wrong on purpose (the negative controls only)."""
    mu = 1.01 * A_MU if control == "mu+1%" else A_MU
    normal = DA_NORMAL
    if control == "normal-swapped":
        normal = (DA_NORMAL[1], DA_NORMAL[0], DA_NORMAL[2])
    w = DA_RADIUS / DA_NBINS
    shift = 0.0
    if control == "centre+0.1w":    # along the line from the source's foot to the centre
        rel = np.array(DA_CENTRE) - np.array(A_SRC)
        rel = rel - float(rel @ np.array(DA_NORMAL)) * np.array(DA_NORMAL)
        shift = 0.1 * w * rel / math.sqrt(float(rel @ rel))
    windowed = control != "no-window"
    ce = AR.circle_edges(DA_RADIUS, DA_NBINS)
    r1, r2, nb = DA_ANN
    ae = AR.annulus_edges(r1, r2, nb)
    if control == "floor":          # int(r / w) + 1: every edge half a bin further out
        ce = np.concatenate([[0.0], (np.arange(DA_NBINS) + 1.0) * w])
        ae = r1 + np.concatenate([[0.0], (np.arange(nb) + 1.0) * (r2 - r1) / nb])
    circle = AR.point_source_disc_bins(A_SRC, mu, np.array(DA_CENTRE) + shift, normal, ce, windowed=windowed)
    if control == "floor":
        circle, ann_tail = np.append(circle, 0.0), [0.0]
    else:
        ann_tail = []
    if control == "no-clamp":       # nint(r / w) + 1 beyond the array: the last half bin is lost
        circle = np.append(circle[:-1], 0.0)
    annulus = np.append(AR.point_source_disc_bins(A_SRC, mu, np.array(DA_ANN_CENTRE) + shift, normal, ae, windowed=windowed), ann_tail)
    if control == "annulus-shifted":  # r1 <= r < r2 read as one bin further in
        annulus = np.append(annulus[1:], 0.0)
    # the camera neither looks at the leg's length nor at the side it is met from: mu = 0
    p_cam, xy = AR.point_source_rect(A_SRC, 0.0, DA_CAM_P1, DA_CAM_E1, DA_CAM_E2)
    cam = np.zeros((DA_CAM_NBINS + 1) ** 2)
    cam[AR.camera_pixel(xy, DA_CAM_NBINS, DA_CAM_MAXVAL)] = p_cam
    fibre, r_max, a, _ = AR.fibre_bins(A_SRC, mu, _fibre_front(), DA_FIBRE_AXIS, _fibre_f(), DA_FIBRE_NBINS,
                                       abs_at_pinhole=control == "fibre-abs-pinhole")
    if control is None:
        assert a < -0.1 and np.count_nonzero(fibre) > 2, (a, fibre)
    flipped = circle.copy() if control == "orientation-ignored" else np.zeros_like(circle)
    return [circle, cam, annulus, fibre, flipped]


# D-B: four circles on the beam's planes. +z: the reflected beam and the light leaving the slab
# upwards, 2e-3 above the upper face (the first steps after a crossing) and at z = 1.0; -z: what
# leaves downwards, likewise. The bins are narrower than the distance between successive landings.
DB_GAP = 2e-3
DB_DETS = (  # (centre x, y), height above (+) or below (-) the slab's face or None for |z| = 1, radius, nbins
    ((-0.10, 0.30), +1, DB_GAP, 0.60, 10),
    ((0.20, 0.45), +1, None, 0.56, 7),
    ((0.20, 0.45), -1, DB_GAP, 0.60, 10),
    ((0.25, 0.40), -1, None, 0.50, 10),
)


def _db_geometry(form):
    out = []
    for (x, y), side, gap, radius, nb in DB_DETS:
        z = side * (z_half(form) + gap) if gap is not None else side * 1.0
        assert np.min(np.abs(AR.faces(NZ, HALF[2]) - z)) > 1e-3, "a detector on a voxel face"
        out.append(((x, y, z), (0.0, 0.0, float(side)), radius, nb))
    return out


def dets_b(form):
    return [scene.circle_dect(c, n, 1, radius, nb) for c, n, radius, nb in _db_geometry(form)]


@functools.lru_cache(maxsize=None)
def expected_b(form, control=None):
    """(p per detector, landings per detector) of dets_b(form)."""
    mu = 1.01 * B_MU if control == "mu+1%" else B_MU
    legs = AR.beam_slab_legs(*faces(), B_ORIGIN, B_DIR, z_half(form), B_N_IN, mu_in=mu)
    ps, lands = [], []
    for c, n, radius, nb in _db_geometry(form):
        if control == "orientation-ignored":
            n = tuple(-v for v in n)
        p, landed = AR.legs_on_disc(legs, mu, c, n, AR.circle_edges(radius, nb))
        assert _inside_grid([at for _, _, at, _ in landed], slack=1e-3)
        ps.append(p)
        lands.append(landed)
    return ps, lands


# D-C: no closed form in a scattering scene, but an identity: on one plane inside the slab a
# circle of radius R, one of radius r1 and the annulus r1 < r <= R, each with a single bin.
DC_CENTRE, DC_NORMAL, DC_R1, DC_R = (0.05, 0.0, 0.30), DA_NORMAL, 0.08, 0.15


def dets_c():
    assert abs(DC_CENTRE[2]) + DC_R < Z_HALF - MESH_INSET
    return [scene.circle_dect(DC_CENTRE, DC_NORMAL, 1, DC_R, 0), scene.circle_dect(DC_CENTRE, DC_NORMAL, 1, DC_R1, 0),
            scene.annulus_dect(DC_CENTRE, DC_NORMAL, 1, DC_R1, DC_R, 0)]


def check_identity(det_bins, ctr, weighted):
    """total(circle R) == total(circle r1) + total(annulus): exact integers in an analogue run,
    to rtol 1e-12 where the bins hold fp64 weights added atomically. The detector_hits counter
    counts bin increments."""
    big, small, ann = (float(b) for b in det_bins)
    assert len(det_bins) == 3 and min(big, small, ann) > 0.0, det_bins
    if weighted:
        assert abs(big - (small + ann)) <= 1e-12 * big, det_bins
        assert ctr["detector_hits"] >= big + small + ann
    else:
        assert big == small + ann and all(float(b).is_integer() for b in det_bins), det_bins
        assert ctr["detector_hits"] == big + small + ann, (ctr, det_bins)


# D-O: per-origin totals of batched point sources (SDF form only), D-A's circle, annulus and
# flipped circle. The origins: A_SRC; two more on the near side at other distances; one behind the
# plane (every total exactly 0); one whose foot on the plane is outside the disc.
DO_ORIGINS = (A_SRC, (0.30, -0.22, 0.22), (0.12, 0.05, -0.05), (0.45, -0.25, 0.75), (-0.35, 0.30, 0.15))


def dets_o():
    d = dets_a()
    return [d[0], d[2], d[4]]


@functools.lru_cache(maxsize=None)
def expected_o(origins=DO_ORIGINS):
    """p[k, d]: the probability that a photon from origin k is counted by detector d."""
    r1, r2, _ = DA_ANN
    out = np.zeros((len(origins), 3))
    for k, o in enumerate(origins):
        out[k, 0] = AR.point_source_disc_bins(o, A_MU, DA_CENTRE, DA_NORMAL, [0.0, DA_RADIUS])[0]
        out[k, 1] = AR.point_source_disc_bins(o, A_MU, DA_ANN_CENTRE, DA_NORMAL, [r1, r2])[0]
        out[k, 2] = AR.point_source_disc_bins(o, A_MU, DA_CENTRE, tuple(-c for c in DA_NORMAL), [0.0, DA_RADIUS])[0]
    return out


# ------------------------------------------------------ detector statistics and assertions ----
def evaluate_det(bins, expected, n, hits=None):
    """Detector bins (one array per detector) of n photons against their probabilities. ALPHA is
    shared equally by the statistics of the test: for each detector with a support max |z| and
    sum z^2 of its bins (count_stats, bins below MIN_EVENTS pooled) and the binomial of its total."""
    live = [d for d, p in enumerate(expected) if p.sum() > 0.0]
    a = ALPHA / (3.0 * max(1, len(live)))
    out = {"n": n, "z_bound": binomial_bound(a), "dets": [], "hits": hits,
           "sum_bins": float(sum(np.asarray(b).sum() for b in bins))}
    for d, (b, p) in enumerate(zip(bins, expected)):
        b = np.asarray(b, dtype=np.float64)
        assert b.shape == p.shape, (d, b.shape, p.shape)
        st = {"off_support": float(b[p == 0.0].sum()), "total": float(b.sum()), "p_total": float(p.sum()),
              "integers": bool(np.all(b == np.floor(b)))}
        if d in live:
            st["counts"] = count_stats(b, p, n, 2.0 * a)
            st["z_total"] = binomial_z(b.sum(), p.sum(), n)
        out["dets"].append(st)
    return out


def check_det(st, pool_cap=None):
    for d in st["dets"]:
        assert d["off_support"] == 0.0 and d["integers"], d
        if "counts" in d:
            check_counts(d["counts"])
            assert abs(d["z_total"]) <= st["z_bound"], (d, st["z_bound"])
            if pool_cap is not None:
                assert d["counts"]["pooled_share"] <= pool_cap, d
    if st["hits"] is not None:
        assert st["hits"] == st["sum_bins"], st


def evaluate_origins(totals, expected, n):
    """totals[k, d] of n photons per origin against p[k, d]: one binomial each, ALPHA shared by
    those with p > 0; the others must read exactly zero."""
    t, p = np.asarray(totals, dtype=np.float64), np.asarray(expected)
    assert t.shape == p.shape, (t.shape, p.shape)
    live = p > 0.0
    z = np.zeros_like(p)
    z[live] = (t[live] - n * p[live]) / np.sqrt(n * p[live] * (1.0 - p[live]))
    return {"z": z, "max_z": float(np.abs(z).max()), "z_bound": binomial_bound(ALPHA / max(1, int(live.sum()))),
            "off_support": float(t[~live].sum()), "min_events": float((n * p[live]).min())}


def check_origins(st):
    assert st["off_support"] == 0.0, st
    assert st["min_events"] >= MIN_EVENTS, st
    assert st["max_z"] <= st["z_bound"], st


def digest(bins):
    """An exact fingerprint of integer bins: (sum, sum of (i + 1) * bins[i]) over all detectors'
    bins in order; both are exact in fp64 far beyond the counts used here."""
    b = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in bins])
    return float(b.sum()), float((b * (np.arange(len(b)) + 1.0)).sum())


# The GPU tests' photon counts; the reference's quadrature error is judged at N_GPU.
N_GPU = 20_000_000    # D-A and D-B, per path
N_GPU_C = 2_000_000   # D-C is an identity: no bin needs a count
N_GPU_O = 4_000_000   # per origin, five origins
N_GPU_E = 2_000_000   # per launch cell, eight cells
ESCAPE_GRID = ("none", (2, 2, 2), (0.2, 0.2, 0.8), (0.2, -0.1, 0.1))  # symmetry, cells, half-extents, position


def escape_case():
    """(config, launch-cell indices (k, 3) 0-based, p[k, d]) of the escape check: a 2 x 2 x 2
    symmetry grid without symmetry, its lower four cells before the detectors' planes and its
    upper four behind them."""
    from rsmcrt_amd import escape
    cfg = escape.escape_config(*ESCAPE_GRID[:3], position=ESCAPE_GRID[3])
    idx, pos = escape.cells(cfg)
    assert len(idx) == 8 and _inside_grid(pos)
    return cfg, idx - 1, expected_o(tuple(tuple(float(c) for c in p) for p in pos))


def check_escape(es, n):
    """escape_sym[d, cell] = total / N in fp32 against the binomial of p there."""
    _, idx, p = escape_case()
    tot = np.array([[float(es[d, i, j, k]) * n for d in range(3)] for i, j, k in idx])
    assert np.abs(tot - np.round(tot)).max() < 0.2, tot   # (fp32 of total / N: 6e-8 of the total)
    st = evaluate_origins(np.round(tot), p, n)
    print(st)
    check_origins(st)
    assert np.count_nonzero(p[:, 0]) == 4 and np.count_nonzero(tot[:, 0]) == 4
    return st


def flat_det(st):
    """The figures of evaluate_det that PREDICTED records."""
    out = {"hits": st["hits"]}
    for d, s in enumerate(st["dets"]):
        out[f"total{d}"] = s["total"]
        if "counts" in s:
            out[f"max_z{d}"], out[f"chi2{d}"], out[f"z_total{d}"] = s["counts"]["max_z"], s["counts"]["chi2"], s["z_total"]
    return out


# ------------------------------------------------------------- scattering-medium cases ----
# One homogeneous scattering medium, effectively infinite, against the exact layer expectations
# of tests/analytic_ref.py (scatter_cumulative; DESIGN.md §3.5 "Scattering media"). Shared by
# tests/test_scatter_analytic_cpu.py and tests/test_gpu_scatter_analytic.py.
#
# The grid: 64 x 72 x 52 voxels of 0.2 x 0.175 x 0.24 over half-extents (6.4, 6.3, 6.24), three
# different counts and edges; mut = 10, so the walls are more than 60 mean free paths from every
# source. Figures from the reference alone (test_scatter_analytic_cpu.test_conditions asserts them):
#   expected escapes in 2.016e7 photons, by the bound of escape_bound(): at most 1.8e-4 (iso g = 0.8),
#     1.9e-4 (beam -z, mirror) and 3.2e-4 (beam +z), below 1e-12 for g = 0 and g = -0.5;
#   layers with N p >= 100 along x, y, z: 21, 25, 19 (iso g = 0.8), 15, 16, 12 (g = 0), 13, 15, 11
#     (g = -0.5), 21, 23, 17 and 21, 23, 18 (the beams), 21, 24, 19 (mirror); the layers below hold at
#     most 1.5e-5 of the absorptions;
#   the reference's error, by doubling the k-range, the k-resolution and L: at most 3.6e-3 of a
#     layer's standard error at 2.016e7 photons (the beams; 2.1e-3 for the point sources).
S_NX, S_NY, S_NZ = 64, 72, 52
S_HALF = (6.4, 6.3, 6.24)
S_EDGES = tuple(2.0 * h / n for h, n in zip(S_HALF, (S_NX, S_NY, S_NZ)))
S_MUS, S_MUA = 7.0, 3.0
S_SRC = (0.087, -0.061, 0.07)        # on no face and no voxel centre
S_MIRROR_SRC = (0.1, 0.0, 0.12)      # a voxel centre in x and z, a voxel face in y
S_POOL_CAP = 1e-3
S_ESCAPE_CAP = 1e-3                  # expected escapes over the whole run
S_REF_ERR_CAP = 1e-2                 # the reference's error per layer, in standard errors at N_GPU_S
N_GPU_S = 24 * 840_000
# case -> (source kind, position, direction or None, g)
S_CASES = {
    "iso-g0.8": ("point", S_SRC, None, 0.8),
    "iso-g0": ("point", S_SRC, None, 0.0),
    "iso-g-0.5": ("point", S_SRC, None, -0.5),
    "beam-z-": ("pencil", S_SRC, (0.0, 0.0, -1.0), 0.8),
    "beam-z+": ("pencil", S_SRC, (0.0, 0.0, 1.0), 0.8),
    "mirror": ("point", S_MIRROR_SRC, None, 0.8),
}
S_MIN_LAYERS = {"iso-g0.8": 16, "beam-z-": 16, "beam-z+": 16, "mirror": 16, "iso-g0": 8, "iso-g-0.5": 8}
# the reference's quadrature, doubled (the estimate of its error)
S_DOUBLED = dict(kmax=2.0 * AR.SC_KMAX, panel=0.5 * AR.SC_PANEL, ratio=0.5 * AR.SC_RATIO, l0=2 * AR.SC_L0, lk=2.0 * AR.SC_LK)


def grid_s():
    return scene.grid(S_NX, S_NY, S_NZ, *S_HALF)


def faces_s():
    return AR.faces(S_NX, S_HALF[0]), AR.faces(S_NY, S_HALF[1]), AR.faces(S_NZ, S_HALF[2])


def scene_s(case, form):
    """(scene, source) of a scattering case: the medium fills an SDF box far larger than the grid,
    an all-zero label volume, or both sides of a mesh box far beyond the grid."""
    kind, pos, direction, g = S_CASES[case]
    m = scene.mono(S_MUS, S_MUA, g, 1.0)
    src = scene.point_source(pos) if kind == "point" else scene.pencil_source(pos, direction)
    if form == "sdf":
        return scene.Scene([scene.box((60.0, 60.0, 60.0), m, 1)]), src
    if form == "voxel":
        return scene.VoxelScene(np.zeros((S_NX, S_NY, S_NZ), dtype=np.uint8), [m]), src
    ms = scene.MeshScene([m, m], ambient=1)
    return ms.add_surface(*builders.box_mesh((-30.0, -30.0, -30.0), (30.0, 30.0, 30.0)), 0, 1), src


S_CONTROLS = ("g+1%", "mut+1%", "mua+1%", "mus+1%", "g2=g", "isotropic", "reversed", "x-y-swapped", "x-z-swapped",
              "y-z-swapped", "source+0.1dx", "source+0.1dy", "source+0.1dz")


@functools.lru_cache(maxsize=None)
def reference_s(case, control=None, doubled=False):
    """The absorption probability per photon of every voxel layer along x, y and z: three arrays.
    The expected track per photon is that over S_MUA. `control` names a reference that is wrong
    on purpose (the negative controls only); `doubled` doubles the quadrature's parameters."""
    kind, pos, direction, g = S_CASES[case]
    mus, mua = S_MUS, S_MUA
    pos = list(pos)
    if control == "g+1%":
        g = 1.01 * g
    elif control == "mut+1%":     # the albedo as it is
        mus, mua = 1.01 * mus, 1.01 * mua
    elif control == "mua+1%":
        mua = 1.01 * mua
    elif control == "mus+1%":
        mus = 1.01 * mus
    elif control == "isotropic":
        g = 0.0
    elif control == "reversed" and direction is not None:
        direction = tuple(-c for c in direction)
    elif control is not None and control.startswith("source+0.1d"):
        a = "xyz".index(control[-1])
        pos[a] += 0.1 * S_EDGES[a]
    elif control is not None and control.endswith("-swapped"):   # the scene with two axes exchanged
        i, j = "xyz".index(control[0]), "xyz".index(control[2])
        pos[i], pos[j] = pos[j], pos[i]
        if direction is not None:
            direction = list(direction)
            direction[i], direction[j] = direction[j], direction[i]
    kw = dict(S_DOUBLED) if doubled else {}
    if control == "g2=g":         # the right mean cosine, the wrong shape
        g = (g, g)
    xs = [e - s for e, s in zip(faces_s(), pos)]
    cum = [None, None, None]
    # the axes with the same direction cosine of the source share one k-integral
    for mu0 in ([None] if kind == "point" else sorted({float(c) for c in direction})):
        axes = [a for a in range(3) if kind == "point" or float(direction[a]) == mu0]
        c = AR.scatter_cumulative(np.concatenate([xs[a] for a in axes]), mus, mua, g, mu0, **kw)
        for a, part in zip(axes, np.split(c, np.cumsum([len(xs[a]) for a in axes])[:-1])):
            cum[a] = part
    return [np.maximum(np.diff(c), 0.0) for c in cum]   # (the far layers: 1e-9 of either sign)


def escape_bound(case):
    """A bound on the expected escapes per photon, from the reference alone: a photon that crosses
    a wall outward flies straight to its next collision, which lies beyond the wall, and is
    absorbed there with probability 1 - a; so P(cross) <= P(absorption site beyond the wall) / (1 - a),
    summed over the six walls, each tail by Chernoff's bound on the moment generating function."""
    kind, pos, direction, g = S_CASES[case]
    total = 0.0
    for a in range(3):
        mu0 = None if kind == "point" else float(direction[a])
        for side in (1, -1):
            total += AR.scatter_tail_bound(S_HALF[a] - side * pos[a], S_MUS, S_MUA, g, mu0, side)
    return total / (1.0 - S_MUS / (S_MUS + S_MUA))


def layer_sums(a):
    """The sums of a grid (nz, ny, nx) over the voxel layers along x, y and z."""
    return [a.sum(axis=(0, 1)), a.sum(axis=(0, 2)), a.sum(axis=(1, 2))]


def run_layers(run, n_batch, batches=BATCHES, keep_grid=False):
    """`run(first_photon, n)` -> Result for each of `batches` disjoint photon ranges of one seed,
    reduced at once: {"ab": per axis [B, layers] of absorb, "jm": the same of jmean, "ctr": summed
    counters, "grid": absorb summed over the batches (keep_grid) or None}."""
    ab, jm, ctr, g = [[], [], []], [[], [], []], {}, None
    for b in range(batches):
        r = run(b * n_batch, n_batch)
        for a, (sa, sj) in enumerate(zip(layer_sums(r.absorb.astype(np.float64)), layer_sums(r.jmean.astype(np.float64)))):
            ab[a].append(sa)
            jm[a].append(sj)
        if keep_grid:
            g = r.absorb.astype(np.float64) if g is None else g + r.absorb
        for k, v in r.counters_dict().items():
            ctr[k] = ctr.get(k, 0) + v
    return {"ab": [np.array(x, dtype=np.float64) for x in ab], "jm": [np.array(x, dtype=np.float64) for x in jm],
            "ctr": ctr, "grid": g}


def evaluate_s(run, n_batch, ref, weighted=False):
    """A scattering case's run (run_layers) against ref = the three arrays of layer probabilities.
    ALPHA is shared by seven groups: per axis the absorb layer sums (a multinomial, count_stats;
    with survival bias they hold weights and are batch means like the tracks) and the batch means
    of the jmean layer sums (batch_stats; a layer's events are its expected absorptions, each of
    which left track there), and the `scatters` counter, whose mean per photon is a / (1 - a) and
    variance a / (1 - a)^2 (the collisions before the absorbing one are geometric). With survival
    bias no photon ends at a collision, so the counter has no such law and is not tested."""
    n = n_batch * len(run["ab"][0])
    a = ALPHA / 7.0
    ctr = run["ctr"]
    _, _, s_mean, s_var = AR.scatter_moments(S_MUS, S_MUA, 0.0)
    st = {"n": n, "weighted": weighted, "axes": [], "z_bound": binomial_bound(a),
          "z_scatters": (ctr["scatters"] - n * s_mean) / math.sqrt(n * s_var),
          "absorbed": ctr["absorbed"], "escaped": ctr["escaped"], "faults": ctr.get("faults", 0), "photons": ctr["photons"]}
    for ab, jm, p in zip(run["ab"], run["jm"], ref):
        assert ab.shape[1] == len(p) and jm.shape[1] == len(p)
        counts = batch_stats(ab, n_batch * p, n * p, a) if weighted else count_stats(ab.sum(axis=0), p, n, a)
        st["axes"].append({"counts": counts, "tracks": batch_stats(jm, n_batch * p / S_MUA, n * p, a),
                           "own": int(np.count_nonzero(n * p >= MIN_EVENTS))})
    return st


def check_s(st, min_layers=8, pool_cap=S_POOL_CAP):
    assert st["faults"] == 0 and st["escaped"] == 0 and st["photons"] == st["n"], st
    if not st["weighted"]:
        assert st["absorbed"] == st["n"], st
        assert abs(st["z_scatters"]) <= st["z_bound"], st
    for ax in st["axes"]:
        for group in ("counts", "tracks"):
            assert ax[group]["pooled_share"] <= pool_cap and ax["own"] >= min_layers, ax[group]
        (check_batches if st["weighted"] else check_counts)(ax["counts"])
        check_batches(ax["tracks"])


def flat_s(st):
    """The figures of evaluate_s that PREDICTED records."""
    out = {} if st["weighted"] else {"z_scatters": st["z_scatters"]}
    for name, ax in zip("xyz", st["axes"]):
        c, t = ax["counts"], ax["tracks"]
        if st["weighted"]:
            out[name + "_ab_max_t"], out[name + "_ab_mean_t2"], out[name + "_ab_t_sum"] = c["max_t"], c["mean_t2"], c["t_sum"]
        else:
            out[name + "_max_z"], out[name + "_chi2"] = c["max_z"], c["chi2"]
        out[name + "_max_t"], out[name + "_mean_t2"], out[name + "_score"], out[name + "_t_sum"] = t["max_t"], t["mean_t2"], t["score"], t["t_sum"]
    return out


# S-mirror: the source on a voxel centre in x and z and on a voxel face in y, so that the grid's
# voxels fall into mirror orbits (x -> -x, y -> -y, z -> -z about the source) of 8 voxels of one
# size with equal expectations; 4 or 2 where the orbit lies in the source's x or z layer.
def mirror_window(counts):
    """The absorb grid (nz, ny, nx) cut to the largest window that is symmetric about S_MIRROR_SRC."""
    xe, ye, ze = faces_s()
    i0 = int(np.searchsorted(xe, S_MIRROR_SRC[0])) - 1
    jf = int(np.argmin(np.abs(ye - S_MIRROR_SRC[1])))
    k0 = int(np.searchsorted(ze, S_MIRROR_SRC[2])) - 1
    assert abs(0.5 * (xe[i0] + xe[i0 + 1]) - S_MIRROR_SRC[0]) < 1e-12 and abs(ye[jf] - S_MIRROR_SRC[1]) < 1e-12
    assert abs(0.5 * (ze[k0] + ze[k0 + 1]) - S_MIRROR_SRC[2]) < 1e-12
    for e in (xe, ye, ze):
        assert np.ptp(np.diff(e)) < 1e-12, "an orbit would mix voxels of different size"
    rx, ry, rz = min(i0, S_NX - 1 - i0), min(jf, S_NY - jf), min(k0, S_NZ - 1 - k0)
    return np.asarray(counts, dtype=np.float64)[k0 - rz:k0 + rz + 1, jf - ry:jf + ry, i0 - rx:i0 + rx + 1], (rx, ry, rz)


def mirror_stats(counts, alpha=ALPHA):
    """Homogeneity of every mirror orbit whose members expect at least MIN_EVENTS absorptions
    (the orbit's total over its size: given the total, the members are equiprobable, so that is
    their expectation): z_m = (c_m - e) / sqrt(e (1 - 1/m)) and sum (c_m - e)^2 / e, chi^2 with
    m - 1 degrees of freedom per orbit; and per axis the two halves of the layer sums, pair by pair,
    z = (c+ - c-) / sqrt(c+ + c-). alpha is shared by the four groups, and in each by max |z| and
    the chi^2 range."""
    w, (rx, ry, rz) = mirror_window(counts)
    stack = np.array([w[::sz, ::sy, ::sx] for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)])
    stack = stack[:, rz:, ry:, rx:]                       # one octant: every orbit once
    size = np.full(stack.shape[1:], 8.0)
    size[0, :, :] /= 2.0                                  # the source's z layer mirrors onto itself
    size[:, :, 0] /= 2.0
    e = stack.sum(axis=0) / 8.0                           # (a member that counts twice is there twice)
    use = e >= MIN_EVENTS
    d = (stack - e[None])[:, use]
    chi = float(((d * d / e[use][None]).sum(axis=0) * size[use] / 8.0).sum())
    dof = int((size[use] - 1.0).sum())
    z = d / np.sqrt(e[use] * (1.0 - 1.0 / size[use]))[None]
    a = alpha / 4.0
    members = int(size[use].sum())
    out = {"orbits": int(use.sum()), "orbits_of_8": int(np.count_nonzero(size[use] == 8.0)), "members": members,
           "max_z": float(np.abs(z).max()), "chi2": chi, "dof": dof,
           "z_bound": float(stats.norm.isf(a / (4.0 * members))),
           "chi2_lo": float(stats.chi2.ppf(a / 4.0, dof)), "chi2_hi": float(stats.chi2.isf(a / 4.0, dof)), "halves": []}
    for axis, r, even in ((2, rx, False), (1, ry, True), (0, rz, False)):
        s = w.sum(axis=tuple(i for i in range(3) if i != axis))
        lo, hi = (s[:r][::-1], s[r:]) if even else (s[:r][::-1], s[r + 1:])
        keep = 0.5 * (lo + hi) >= MIN_EVENTS
        zz = (hi[keep] - lo[keep]) / np.sqrt(hi[keep] + lo[keep])
        v = len(zz)
        out["halves"].append({"pairs": v, "max_z": float(np.abs(zz).max()), "chi2": float((zz * zz).sum()),
                              "z_bound": float(stats.norm.isf(a / (4.0 * v))),
                              "chi2_lo": float(stats.chi2.ppf(a / 4.0, v)), "chi2_hi": float(stats.chi2.isf(a / 4.0, v))})
    return out


def check_mirror(st, min_orbits=50):
    assert st["orbits_of_8"] >= min_orbits, st
    for s in [st] + st["halves"]:
        assert s["max_z"] <= s["z_bound"], s
        assert s["chi2_lo"] <= s["chi2"] <= s["chi2_hi"], s


def flat_mirror(st):
    out = {"orbits": st["orbits"], "m_max_z": st["max_z"], "m_chi2": st["chi2"]}
    for name, h in zip("xyz", st["halves"]):
        out[name + "_half_chi2"] = h["chi2"]
    return out


# ------------------------------------------------------------------- curved surfaces (D) ----
# A sphere of glass in vacuum against tests/analytic_ref.py (beam_legs, cast_sphere,
# cast_triangles, centre_source_sphere; DESIGN.md §3.5 "Curved surfaces"). Shared by
# tests/test_curved_analytic_cpu.py and tests/test_gpu_curved_analytic.py.
#
# The grid is grid() above, 8 x 12 x 10: the conditions below hold on it (34 voxels wholly inside
# the sphere, 779 wholly outside, 147 cut). The sphere: centre D_CENTRE, off every voxel wall and
# off the grid's centre, R = 0.55, n = 1.5, mus = 0, mua = D_MU (D_TIR_MU in D-tir), in vacuum
# wider than the grid. Nothing scatters: every path is a tree of straight legs.
#   D-centre  a point source at the sphere's centre (SDF forms): normal incidence everywhere
#   D-beam    a pencil from outside, impact parameter 0.6 R, in no coordinate plane (SDF, mesh):
#             15 legs with q >= 1e-14, 7 of them inside (rho a = 0.006 per bounce; mesh 17 and 8)
#   D-tir     a pencil from inside at sin(incidence) = 0.8 > 1 / n (SDF, mesh): a star polygon of
#             66 legs (mu chord = 0.495), none of which leaves the sphere; in the mesh form the
#             facets' normals differ from the radial one and some hits transmit
# Forms: "sdf" (sphere and vacuum box: ws_kernel, or transport_kernel with SMCRT_LEAN=0), "table"
# (the same with nine index-matched vacuum spheres outside the grid, ten tops and more: the
# cooperative EVAL with its table) and "mesh" (builders.icosphere(2, R, centre), a polyhedron
# whose reference is cast_triangles on the same vertices and triangles). There is no voxel form:
# a label volume has no curved surface.
D_CENTRE = A_SRC
D_R, D_N, D_MU, D_TIR_MU = 0.55, 1.5, 2.0, 0.75
D_Q_MIN = 1e-14
D_FORMS = ("sdf", "table", "mesh")
D_MESH_LEVEL = 2
D_BEAM_DIR = _unit((0.45, -0.3, -0.84))
D_BEAM_B, D_BEAM_BACK = 0.33, 0.85      # the impact parameter (0.6 R) and the run back from the foot
D_TIR_DIR = _unit((0.3, 0.7, -0.5))
D_TIR_SIN, D_TIR_ALONG = 0.8, 0.1
D_EXTRA_Y, D_EXTRA_Z, D_EXTRA_R = 0.95, -1.45, 0.04   # the table form's spheres: outside the grid
D_CLEAR = 0.05
# The track slop, derived from the engine's rule (tauint2) and not fitted: a photon stops within
# 1e-8 of a surface, turns there, steps 2e-8 (+ 1e-8 per glancing round) past it along its ray, and
# steps 1e-8 past every voxel wall. So a crossing is made at most D_EPS_SURFACE = 3e-8 off the
# surface, which along a ray of cosine c to the normal is 3e-8 / c: the leg that arrives and the
# leg that leaves are each off by that much in length where they end and start.
# What a crossing made at radius R - e instead of R does to the later legs: reflection and
# refraction about a radial normal keep Bouguer's invariant n |r x d| wherever on the ray they
# happen, so no later impact parameter and no later angle of incidence changes. What changes is
# the angle the path has turned through about the centre: a ray of impact parameter b spans
# acos(b / r) from its closest approach to radius r, whose derivative by r is tan(theta) / r, so
# the crossing turns every later leg about the centre by at most e (tan(theta_1) + tan(theta')) / R,
# theta' the angle it leaves with (theta_1 reflected, theta_2 refracted). The turns add up along a
# path, they do not compound. A leg after the crossings 1 .. m is therefore displaced by at most
#   Delta = far * sum_j 3e-8 (tan(theta_1j) + tan(theta'_j)) / R,
# far its largest distance from the centre. In a voxel a displacement Delta moves the leg's entry
# through a wall normal to axis a by Delta / |d_a| along the ray and the wall's own step adds
# 1e-8 / |d_a|, likewise for the exit through a wall normal to axis b; an end that lies on the
# surface inside the voxel adds its 3e-8 / c instead; and a leg's track in a voxel is never off by
# more than it is long there. Summed with the legs' q that is d_slop(), per photon and voxel; its
# largest value over the voxels is the `slop` that batch_stats adds to the standard error of every
# voxel of that case (d_track_slop). calcNormal's error on a sphere (h^2 / R^2 truncation, 1e-16 / h
# cancellation: 1e-10 rad) is a thousandth of one crossing's turn and is covered by the margin
# between 1e-8 + 2e-8 c and 3e-8. A mesh scene makes its crossing on the facet itself, without stop
# or step, and a flat facet turns nothing: only the walls' 1e-8 remain. The sphere's
# bound is applied to it unchanged, which is more than it needs.
# Figures (d_conditions()): D-beam 3.8e-7 (SDF) and 1.1e-6 (mesh), D-tir 5.9e-7 and 9.4e-7 per
# photon and voxel, beside B_TRACK_SLOP = 1e-6; in every voxel that holds at least
# D_SLOP_MIN_TRACK of expected track per photon that is at most 4.9e-5 of the track, and the plain
# sum of q x (3e-8 / c over the crossings before the leg) at most 6e-6 of it, which is held below
# D_SLOP_SHARE (a less grazing beam otherwise). Below D_SLOP_MIN_TRACK a voxel holds a sliver of a
# leg next to one of its edges, whose length any displacement changes by a large share of itself
# whatever the beam's incidence; there the absolute bound is what is tested.
D_EPS_SURFACE, D_EPS_WALL = 3e-8, 1e-8
D_SLOP_SHARE = 1e-5   # of a voxel's expected track: the cap on q x (3e-8 / c) summed per voxel
D_SLOP_MIN_TRACK = 1e-2


def d_origin(case):
    """The pencil's origin: off the centre by the impact parameter, across the beam."""
    c = np.array(D_CENTRE)
    if case == "beam":
        d = np.array(D_BEAM_DIR)
        u = np.cross(d, (0.3, 0.9, 0.2))
        return tuple(c + D_BEAM_B * u / math.sqrt(float(u @ u)) - D_BEAM_BACK * d)
    d = np.array(D_TIR_DIR)
    u = np.cross(d, (0.8, -0.1, 0.6))
    return tuple(c + D_TIR_SIN * D_R * u / math.sqrt(float(u @ u)) + D_TIR_ALONG * d)


def d_mu(case):
    return D_TIR_MU if case == "tir" else D_MU


def d_extras():
    """Centres of the table form's nine small spheres, all outside the grid."""
    return [(-0.8 + 0.2 * i, D_EXTRA_Y, D_EXTRA_Z) for i in range(9)]


def scene_d(case, form):
    """(scene, source) of case "centre", "beam" or "tir" in `form`."""
    glass, vac = scene.mono(0.0, d_mu(case), 0.0, D_N), scene.mono(0.0, 0.0, 0.0, 1.0)
    if case == "centre":
        assert form != "mesh", "D-centre has no mesh form: the polyhedron is not met at normal incidence"
        src = scene.point_source(D_CENTRE)
    else:
        src = scene.pencil_source(d_origin(case), D_BEAM_DIR if case == "beam" else D_TIR_DIR)
    if form == "mesh":
        ms = scene.MeshScene([glass, vac], ambient=1)
        return ms.add_surface(*builders.icosphere(D_MESH_LEVEL, D_R, D_CENTRE), 0, 1), src
    tops = [scene.sphere(D_R, glass, 1, transform=scene.invert(scene.translate(D_CENTRE)))]
    if form == "table":
        tops += [scene.sphere(D_EXTRA_R, vac, i + 2, transform=scene.invert(scene.translate(p)))
                 for i, p in enumerate(d_extras())]
    return scene.Scene(tops + [scene.box((40.0, 40.0, 40.0), vac, len(tops) + 1)]), src


D_CONTROLS = ("n+1%", "R+1%", "mu+1%", "s-polarised", "normal-tilted", "exit-normal-unturned",
              "x-y-swapped", "x-z-swapped", "y-z-swapped")
D_TILT, D_TILT_AXIS = 5e-3, (0.5, -0.6, 0.62)


def _d_cast(form, radius=D_R):
    if form == "mesh":
        v, t = builders.icosphere(D_MESH_LEVEL, radius, D_CENTRE)
        n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
        assert np.all((n * (v[t[:, 0]] - np.array(D_CENTRE))).sum(axis=1) > 0.0), "a facet wound inwards"
        return AR.cast_triangles(v, t)
    return AR.cast_sphere(D_CENTRE, radius)


@functools.lru_cache(maxsize=None)
def trace_d(case, form="sdf", control=None):
    """beam_legs of D-beam or D-tir: (track, p_abs, legs, hits, paths). `control` names a reference
    that is wrong on purpose (the negative controls only). The table form is the SDF form."""
    form = "mesh" if form == "mesh" else "sdf"
    n = 1.01 * D_N if control == "n+1%" else D_N
    mu = (1.01 if control == "mu+1%" else 1.0) * d_mu(case)
    cast = _d_cast(form, 1.01 * D_R if control == "R+1%" else D_R)
    if control == "normal-tilted":
        cast = AR.tilted(cast, D_TILT_AXIS, D_TILT)
    out = AR.beam_legs(*faces(), d_origin(case), D_BEAM_DIR if case == "beam" else D_TIR_DIR, cast, n, 1.0, mu,
                       D_Q_MIN, polarisation="s" if control == "s-polarised" else "unpolarised",
                       exit_normal_unturned=control == "exit-normal-unturned")
    if control is not None and control.endswith("-swapped"):
        ax = control[0] + control[2]
        out = (swapped(out[0], ax), swapped(out[1], ax)) + out[2:]
    return out


def reference_d(case, form="sdf", control=None):
    """(T, p) of D-beam and D-tir: expected track and absorption probability per photon and voxel."""
    return trace_d(case, form, control)[:2]


def centre_d(control=None):
    """centre_source_sphere of D-centre."""
    return _centre_d(control)


@functools.lru_cache(maxsize=None)
def _centre_d(control):
    return AR.centre_source_sphere(*faces(), D_CENTRE, 1.01 * D_R if control == "R+1%" else D_R,
                                   1.01 * D_N if control == "n+1%" else D_N, (1.01 if control == "mu+1%" else 1.0) * D_MU)


def reduce_centre(a, control=None):
    """A grid [..., nz, ny, nx] of D-centre as [..., M + 1]: the voxels the surface does not cut,
    then the sum of the cut ones. The -swapped controls exchange two axes of the data first."""
    a = np.asarray(a, dtype=np.float64)
    if control is not None and control.endswith("-swapped"):
        flat = a.reshape(-1, NZ, NY, NX)
        a = np.array([swapped(g, control[0] + control[2]) for g in flat]).reshape(a.shape)
    cut = centre_d()["cut"]
    return np.concatenate([a[..., ~cut], a[..., cut].sum(axis=-1, keepdims=True)], axis=-1)


def reference_centre(control=None):
    """(T, p) of D-centre in reduce_centre's layout. The cut mask is the right sphere's also under
    a control, so that data and reference are pooled alike."""
    control = None if control is None or control.endswith("-swapped") else control
    ref = centre_d(control)
    cut = centre_d()["cut"]
    if control is None:
        t = np.append(ref["track"][~cut], ref["cut_track"])
        p = np.append(ref["p_abs"][~cut], ref["cut_p_abs"])
    else:   # a wrong sphere cuts other voxels: what it leaves undetermined goes to the pooled bin by conservation
        known = ~cut & ~ref["cut"]
        t_all = ref["cut_track"] + float(ref["track"][~ref["cut"]].sum())
        p_all = ref["cut_p_abs"] + float(ref["p_abs"][~ref["cut"]].sum())
        t = np.append(np.where(known, ref["track"], 0.0)[~cut], 0.0)
        p = np.append(np.where(known, ref["p_abs"], 0.0)[~cut], 0.0)
        # the voxels the wrong sphere cuts but the right one does not: their share is unknown, and a
        # control may not claim more than it knows, so they are given the right reference's values
        gap = ~cut & ref["cut"]
        good = centre_d()
        t[:-1] += np.where(gap, good["track"], 0.0)[~cut]
        p[:-1] += np.where(gap, good["p_abs"], 0.0)[~cut]
        t[-1], p[-1] = t_all - t[:-1].sum(), p_all - p[:-1].sum()
    return t, p


def d_slop(case, form="sdf"):
    """The bound on the systematic track error per photon of every voxel, (nz, ny, nx): see above."""
    _, _, legs, _, paths = trace_d(case, form)
    xe, ye, ze = faces()
    zz, yy, xx = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    lo = np.stack([xe[xx], ye[yy], ze[zz]], axis=-1)
    hi = np.stack([xe[xx + 1], ye[yy + 1], ze[zz + 1]], axis=-1)
    c = np.array(D_CENTRE)
    out = np.zeros((NZ, NY, NX))

    def tan(cosine):
        return math.sqrt(max(0.0, 1.0 - cosine * cosine)) / cosine

    for (o, d, q, length, _), path in zip(legs, paths):
        end = o + length * d
        far = max(math.sqrt(float((o - c) @ (o - c))), math.sqrt(float((end - c) @ (end - c))))
        delta = far * sum(D_EPS_SURFACE * (tan(c1) + tan(c_out)) / D_R for c1, c_out in path)
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (lo - o) / d, (hi - o) / d
        t_in, t_out = np.minimum(ta, tb), np.maximum(ta, tb)
        s0, s1 = t_in.max(axis=-1), t_out.min(axis=-1)
        per_wall = (delta + D_EPS_WALL) / np.abs(d)
        off_in = np.where(s0 > 0.0, per_wall[t_in.argmax(axis=-1)], D_EPS_SURFACE / path[-1][1] if path else 0.0)
        on_surface = bool(np.all(np.abs(end) < np.array(HALF) - 1e-9))     # (the leg ends inside the grid)
        c_end = abs(float(d @ (end - c))) / math.sqrt(float((end - c) @ (end - c)))
        off_out = np.where(s1 < length, per_wall[t_out.argmin(axis=-1)], D_EPS_SURFACE / c_end if on_surface else 0.0)
        run = np.minimum(s1, length) - np.maximum(s0, 0.0)
        out += q * np.where(run > 1e-12, np.minimum(run, off_in + off_out), 0.0)
    return out


@functools.lru_cache(maxsize=None)
def d_track_slop(case, form="sdf"):
    """The `slop` of evaluate_ab for a case: the largest d_slop() of a voxel."""
    return float(d_slop(case, form).max())


@functools.lru_cache(maxsize=None)
def d_conditions(n=24 * 840_000):
    """The conditions on scene D's inputs at n photons, asserted from the references alone; returns
    the figures (tests/test_curved_analytic_cpu.py prints them): D-centre's voxel counts and fewest
    events; per beam case and form the legs, hits, smallest incidence cosine, pooled shares, slop
    and its shares of a voxel's track."""
    xe, ye, ze = faces()
    out = {}
    assert np.all(np.abs(np.array(D_CENTRE)) + D_R < np.array(HALF)), "the sphere leaves the grid"
    for a, e in enumerate((xe, ye, ze)):
        assert np.min(np.abs(e - D_CENTRE[a])) > 1e-3 and abs(D_CENTRE[a]) > 1e-3
    for p in d_extras():
        assert any(abs(p[a]) - D_EXTRA_R > HALF[a] + D_CLEAR for a in range(3)), "an extra sphere near the grid"
    c = centre_d()
    t, p = reference_centre()
    assert int(c["inside"].sum()) >= 30 and int(c["outside"].sum()) >= 300, (c["inside"].sum(), c["outside"].sum())
    own_t, pool_t = _bins(n * t / DIAG)
    own_p, pool_p = _bins(n * p)
    assert pool_t is None and pool_p is None, "a D-centre voxel below MIN_EVENTS"
    out["centre"] = {"inside": int(c["inside"].sum()), "outside": int(c["outside"].sum()), "cut": int(c["cut"].sum()),
                     "min_track_events": float((n * t / DIAG).min()), "min_absorb_events": float((n * p[p > 0.0]).min())}
    for case in ("beam", "tir"):
        for form in ("sdf", "mesh"):
            tr, pa, legs, hits, paths = trace_d(case, form)
            for point, c1, q, inside, bary in hits:
                for a, e in enumerate((xe, ye, ze)):
                    assert np.min(np.abs(e - point[a])) > 1e-6, "a surface hit on a voxel wall"
                if form == "mesh" and q >= 1e-9:
                    assert bary > 1e-6, "a leg meets the edge of a facet"
            for pooled, ref in ((_bins(n * pa)[1], pa), (_bins(n * tr / DIAG)[1], tr)):
                share = 0.0 if pooled is None else float(ref.ravel()[pooled].sum() / ref.sum())
                assert share <= B_POOL_CAP, (case, form, share)
            slop = d_slop(case, form)
            own = tr >= D_SLOP_MIN_TRACK
            share = float((slop[own] / tr[own]).max())
            shift = np.zeros_like(tr)   # sum of q x (3e-8 / c over the crossings before the leg), per voxel
            for leg, path in zip(legs, paths):
                shift += leg[2] * sum(D_EPS_SURFACE / min(pair) for pair in path) * (AR.leg_voxels(xe, ye, ze, leg) > 0.0)
            shift_share = float((shift[own] / tr[own]).max())
            assert shift_share <= D_SLOP_SHARE, (case, form, shift_share)
            out[case, form] = {"legs": len(legs), "inside_legs": sum(1 for leg in legs if leg[4]), "hits": len(hits),
                               "min_cos": min(h[1] for h in hits), "own_share_voxels": int(own.sum()), "slop": d_track_slop(case, form), "slop_share": share, "shift_share": shift_share,
                               "p_abs": float(pa.sum()), "voxels": int(np.count_nonzero(tr))}
    return out


def evaluate_weighted(jm, ab, ctr, n_batch, ref, slop):
    """A run of D-tir with FLAG_SURVIVAL_BIAS against ref = (T, p), by batch means as scene C's.
    The sphere's albedo is 0, so a photon leaves its whole weight at its first interaction (absorb
    holds fp64 weights that happen to be ones) and goes on with weight 0 if the roulette spares it:
    what it then deposits is 0.0, wherever it goes, and how it ends (`absorbed`, `escaped`) follows
    no law of the scene, so the counters are not tested. ALPHA is shared by the absorb grid and
    the tracks, both batch_stats."""
    t, p = ref
    n = n_batch * len(jm)
    a = ALPHA / 2.0
    # (the reference follows no leg below D_Q_MIN: it misses at most D_Q_MIN / (1 - exp(-mu chord)) < 10 D_Q_MIN
    # per photon, which is all that separates it from a batch whose every photon was absorbed)
    return {"n": n, "counts": batch_stats(ab, n_batch * p, n * p, a, slop=n_batch * 10.0 * D_Q_MIN),
            "tracks": batch_stats(jm, n_batch * t, n * t / DIAG, a, slop=n_batch * slop),
            "absorb_off_support": float(ab.sum(axis=0)[p == 0.0].sum()), "absorb_sum": float(ab.sum()),
            "jmean_off_support": float(jm.sum(axis=0)[t == 0.0].sum()), "faults": ctr.get("faults", 0)}


def check_weighted(st):
    assert st["faults"] == 0, st
    assert st["absorb_off_support"] == 0.0 and st["jmean_off_support"] == 0.0, st
    for group in ("counts", "tracks"):
        assert st[group]["pooled_share"] < B_POOL_CAP, st[group]
        check_batches(st[group])


# D-beam's detectors, both forms: one circle across the first doubly refracted leg (outside, after
# two crossings) and one across the first externally reflected leg (outside, after one), each
# D_DET_RUN along the leg from the sphere, which is 0.3 or more from its surface. The bins are
# rings D_DET_W wide; the disc is tilted against the leg and placed so that the leg lands in the
# middle of ring D_DET_BIN = 1, at radius w. A ring sees only the radius, and a landing moved by
# delta in the worst direction (through the disc's centre) leaves ring 1 once delta > 2.5 w: a
# direction error of 1e-3 rad moves it by 4.2e-4 = 2.8 w, so it changes the bin whichever way it
# points. (A landing far out in a wide disc would not notice an error along its ring.)
D_DET_RUN, D_DET_W, D_DET_NBINS, D_DET_BIN = 0.42, 1.5e-4, 20, 1
D_DET_TILT = (0.25, 0.1, -0.2)


def _d_det_geometry(form):
    _, _, legs, _, paths = trace_d("beam", form)
    out = []
    for crossings in (2, 1):
        leg = next(lg for lg, path in zip(legs, paths) if len(path) == crossings and not lg[4]
                   and (crossings == 1 or lg[2] > 0.1))
        o, d = leg[0], leg[1]
        at = o + D_DET_RUN * d
        assert math.sqrt(float((at - np.array(D_CENTRE)) @ (at - np.array(D_CENTRE)))) - D_R >= 0.3 and leg[3] > D_DET_RUN + 0.01
        n = d + np.array(D_DET_TILT)
        n = n / math.sqrt(float(n @ n))
        u = np.cross(n, d)
        centre = at + D_DET_BIN * D_DET_W * u / math.sqrt(float(u @ u))
        assert _disc_inside_grid(centre, n, D_DET_W * D_DET_NBINS)
        out.append((tuple(centre), tuple(n), D_DET_W * D_DET_NBINS, D_DET_NBINS))
    return out


def dets_d(form):
    return [scene.circle_dect(c, n, 1, radius, nb) for c, n, radius, nb in _d_det_geometry(form)]


@functools.lru_cache(maxsize=None)
def expected_d(form, control=None):
    """(p per detector, landings per detector) of dets_d(form); the discs stay where the right
    reference puts them under a control."""
    legs = trace_d("beam", form, control)[2]
    mu = (1.01 if control == "mu+1%" else 1.0) * D_MU
    ps, lands = [], []
    for c, n, radius, nb in _d_det_geometry(form):
        p, landed = AR.legs_on_disc(legs, mu, c, n, AR.circle_edges(radius, nb))
        ps.append(p)
        lands.append(landed)
    if control is None:
        assert [[b for b, _, _, _ in ld] for ld in lands] == [[D_DET_BIN], [D_DET_BIN]], lands
    return ps, lands
