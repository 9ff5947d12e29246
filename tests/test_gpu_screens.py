"""Field screens and the optical-path option on the GPU (include/smcrt.h "field screens").

A screen adds weight * exp(i k phi) to the pixel a photon crosses, phi being the photon's phase at
the start of the leg plus n_leg * t along it. Straight pencils are checked against the hit rule
restated in numpy (tests/test_screens_cpu.py np_rule) on every PHAS instantiation of
transport_kernel, the phase carried over leg ends with index-matched surfaces on the way, the
optical path with a slab of n = 1.5, a scattering scene against the polylines of its own recorded
paths, the emitter's phase with the double-slit source; and a run with screens against the same
run without them."""
import ctypes as C
import math

import numpy as np
import pytest

from rsmcrt_amd import abi, scene
from rsmcrt_amd.engine import Engine, SmcrtError, _check, load_library
from tests import plan_cases, planprobe
from tests.test_gpu_parity import SEED, compare
from tests.test_gpu_phasor import (FLAG_CASES, PENCIL_DIR, PENCIL_K, PENCIL_START, PH, PL, RTOL, SMALL_GRIDS, SNAP,
                                   assert_close, near_vacuum, walk)
from tests.test_screens_cpu import np_rule

pytestmark = pytest.mark.gpu

VAC = scene.mono(1e-9, 0.0, 0.0, 1.0)


def grid8():
    return scene.grid(8, 8, 8, 1, 1, 1)


# ---- screens and expectations for one straight line -------------------------------------------
def tilted_screen(centre, nu=4, nv=3, lu=0.5, lv=0.4, at=(0.37, 0.58)):
    """A rectangle whose edges lie along no axis, with `centre` at (u, v) = `at`: away from every
    pixel edge of the 4 x 3 pixels (u * 4 = 1.48, v * 3 = 1.74)."""
    e1 = np.array([0.6, 0.3, -0.2])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(np.array([0.1, -0.5, 0.7]), e1)
    e2 -= e1 * (e2 @ e1)
    e2 /= np.linalg.norm(e2)
    eu, ev = lu * e1, lv * e2
    return scene.screen(np.asarray(centre) - at[0] * eu - at[1] * ev, eu, ev, nu, nv)


def pencil_screens(s=1.0):
    """Test 1's screens, lengths scaled by `s`: a 1 x 1 across the beam, a tilted 4 x 3 around the
    beam's point at path length 1.2, a 2 x 2 behind the source, and a 3 x 5 that takes only photons
    going up (the beam goes down). Four sizes, so a wrong offset shows."""
    centre = s * (np.array(PENCIL_START) + 1.2 * PENCIL_DIR)
    return [scene.screen((-s, -s, 0.3 * s), (2 * s, 0, 0), (0, 2 * s, 0), 1, 1),
            tilted_screen(centre, lu=0.5 * s, lv=0.4 * s),
            scene.screen((-s, -s, 0.95 * s), (2 * s, 0, 0), (0, 2 * s, 0), 2, 2),
            scene.screen((-s, -s, 0.0), (2 * s, 0, 0), (0, 2 * s, 0), 3, 5, sides=+1)]


def line_fields(screens, start, d, k, n, phase0=0.0):
    """What n unit-weight photons flying along one line leave in each screen: (fields, hits)."""
    out, hits = [], []
    for s in screens:
        hit, t, un, vn = np_rule(s, np.array([start], dtype=float), np.array([d], dtype=float), np.array([1e3]))
        f = np.zeros((s.nv, s.nu), dtype=np.complex128)
        if hit[0]:
            for x in (un[0], vn[0]):
                assert abs(x - round(x)) > 1e-3, "the line passes a pixel edge too closely"
            f[min(int(vn[0]), s.nv - 1), min(int(un[0]), s.nu - 1)] = n * np.exp(1j * k * (phase0 + t[0]))
        out.append(f)
        hits.append(bool(hit[0]))
    return out, hits


def check_pencil(got, screens, start, d, k, n, what):
    """Test 1's statement: the one pixel numpy names holds n * exp(i k t) within n * k * 1e-12, every
    other pixel and the screens the beam must not score in are exactly 0."""
    want, hits = line_fields(screens, start, d, k, n)
    assert hits == [True, True, False, False] and len(got) == len(screens)
    for i, (gf, wf) in enumerate(zip(got, want)):
        assert gf.shape == wf.shape and gf.dtype == np.complex128
        err = np.maximum(np.abs(gf.real - wf.real), np.abs(gf.imag - wf.imag))
        print(f"{what}, screen {i}: max |error| {err.max():.3e} (bound {n * k * 1e-12:.3e})")
        assert np.all(gf[wf == 0.0] == 0.0), (what, i)
        assert np.all(err <= n * k * 1e-12), (what, i, float(err.max()))
    assert abs(got[0][0, 0]) > 0.99 * n and np.count_nonzero(got[1]) == 1


# ---- 1. straight pencil ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 3000])
def test_straight_pencil(n):
    """One leg from the source to the medium's wall: one wave, then several blocks."""
    sc, g, src = near_vacuum(2.0), grid8(), scene.pencil_source(PENCIL_START, PENCIL_DIR)
    scr = pencil_screens()
    with Engine(sc, g) as eng:
        eng.set_screens(scr)  # (before the phasor configuration: either order works)
        eng.set_phasor(PENCIL_K)
        res = eng.run(src, n, seed=SEED, flags=PH, records=True)
        got = eng.screens()
    assert res.counter("photons") == n and res.counter("faults") == 0 and res.counter("scatters") == 0
    assert np.all(res.records["dir"] == PENCIL_DIR)
    check_pencil(got, scr, PENCIL_START, PENCIL_DIR, PENCIL_K, n, f"pencil, N = {n}")


# ---- 2. the phase at a leg's start ---------------------------------------------------------------
def sphere_crossings(start, d, r):
    """Path lengths at which the line meets the sphere of radius r about the origin."""
    start = np.asarray(start)
    b, c = start @ d, start @ start - r * r
    return -b - math.sqrt(b * b - c), -b + math.sqrt(b * b - c)


def test_phase_at_leg_start():
    """Two nested index-matched spheres end a leg at every surface; the screen behind the second
    crossing must see the whole path, not the length of its own leg."""
    n = 500
    sc = scene.Scene([scene.sphere(0.35, VAC, 1), scene.sphere(0.6, VAC, 2), scene.box((4.0,) * 3, VAC, 3)])
    g, src = grid8(), scene.pencil_source(PENCIL_START, PENCIL_DIR)
    scr = [scene.screen((-1, -1, -0.05), (2, 0, 0), (0, 2, 0), 1, 1)]
    (want,), hits = line_fields(scr, PENCIL_START, PENCIL_DIR, PENCIL_K, n)
    t_hit = (PENCIL_START[2] + 0.05) / -PENCIL_DIR[2]
    t1, t4 = sphere_crossings(PENCIL_START, PENCIL_DIR, 0.6)
    t2, t3 = sphere_crossings(PENCIL_START, PENCIL_DIR, 0.35)
    assert hits == [True] and 0.0 < t1 < t2 < t_hit < t3 < t4
    with Engine(sc, g) as eng:
        eng.set_phasor(PENCIL_K)
        eng.set_screens(scr)
        res = eng.run(src, n, seed=SEED, flags=PH)
        (got,) = eng.screens()
    assert res.counter("photons") == n and res.counter("faults") == 0 and res.counter("scatters") == 0
    cells, ts, per_axis = walk(PENCIL_START, PENCIL_DIR, g)
    walls = int(np.count_nonzero(ts < t_hit))
    assert walls >= 3
    atol = 2.0 * n * PENCIL_K * walls * SNAP / np.abs(PENCIL_DIR).min()
    assert_close(got, want, atol, "phase at a leg's start")
    # teeth: the leg's own length alone misses by far more
    own = n * np.exp(1j * PENCIL_K * (t_hit - t2))
    assert max(abs((own - want[0, 0]).real), abs((own - want[0, 0]).imag)) > 10.0 * atol


# ---- 3. optical path ------------------------------------------------------------------------------
def test_optical_path():
    """Normal incidence through a slab of n = 1.5: k = 2 pi j / L2 with odd j puts the photons that
    bounced inside the slab in phase with the direct ones in both modes, and the modes pi apart."""
    n, L1, L2, L3, j = 2000, 0.55, 0.3, 0.45, 3
    k = 2.0 * math.pi * j / L2
    x, y, z0 = 0.03, 0.05, 0.9
    slab = scene.box((3.0, 3.0, L2), scene.mono(1e-9, 0.0, 0.0, 1.5), 1,
                     transform=scene.invert(scene.translate((0.0, 0.0, z0 - L1 - 0.5 * L2))))
    sc = scene.Scene([slab, scene.box((4.0,) * 3, VAC, 2)])
    g, src = grid8(), scene.pencil_source((x, y, z0), (0.0, 0.0, -1.0))
    scr = [scene.screen((-1, -1, z0 - L1 - L2 - L3), (2, 0, 0), (0, 2, 0), 1, 1, sides=-1)]  # N = +z, the beam goes down
    fields, grids = {}, {}
    with Engine(sc, g) as eng:
        eng.set_screens(scr)
        for mode, kk, opt in (("count", 0.0, False), ("geometric", k, False), ("optical", k, True)):
            eng.set_phasor(kk, optical_path=opt)  # (a new configuration starts from a zero grid)
            eng.reset_screens()
            res = eng.run(src, n, seed=SEED, flags=PH)
            assert res.counter("photons") == n and res.counter("faults") == 0 and res.counter("scatters") == 0
            assert res.counter("fresnel") >= 2 * 0.85 * n
            fields[mode], grids[mode] = eng.screens()[0][0, 0], eng.phasor()
    M = fields["count"].real
    assert fields["count"].imag == 0.0 and M == round(M) and 0.85 * n < M <= n
    walls = 5  # z = 0.75, 0.5, 0.25, 0, -0.25 between the source and the screen
    atol = 2.0 * M * k * walls * SNAP / 1.0 + M * k * 0.5 * 6e-8
    for mode, path in (("geometric", L1 + L2 + L3), ("optical", L1 + 1.5 * L2 + L3)):
        want = M * np.exp(1j * k * path)
        err = max(abs((fields[mode] - want).real), abs((fields[mode] - want).imag))
        print(f"optical path, {mode}: M = {M:.0f}, |error| {err:.3e}, tolerance {atol:.3e}")
        assert err <= atol, (mode, fields[mode], want)
    # the modes are pi apart, far more than the tolerance
    assert abs(fields["geometric"] + fields["optical"]) <= 2.0 * math.sqrt(2.0) * atol < 1e-3 * M
    # the voxel phasor: the same above the slab, pi apart in the beam's voxels behind it
    pg, po = grids["geometric"], grids["optical"]
    top_of_slab = 5  # the slab's upper face, z = 0.35, lies in voxel layer 5 (z in 0.25 .. 0.5)
    d = np.abs(pg - po)
    assert np.all(d[top_of_slab + 1:] <= atol), float(d[top_of_slab + 1:].max())
    ix, iy = int((x + 1.0) / 0.25), int((y + 1.0) / 0.25)
    below = pg[:4, iy, ix]  # voxel layers wholly behind the slab (its lower face, z = 0.05, is in layer 4)
    assert np.all(np.abs(below) > 0.85 * n) and np.all(np.abs(below + po[:4, iy, ix]) <= 4.0 * atol)
    assert d[top_of_slab, iy, ix] > 0.5 * n  # (the wall z = 0.25 is inside the slab)


# ---- 4. a scattering scene against its own recorded paths ---------------------------------------
def snap_bound(a, b, g):
    """The snap rule of test_straight_track for straight stretches a -> b (arrays of points): 2 *
    SNAP * (voxel walls crossed inside the grid) / min |dir| over the axes crossed."""
    half = np.array([g.xmax, g.ymax, g.zmax])
    h = 2.0 * half / np.array([g.nx, g.ny, g.nz])
    d = b - a
    ln = np.linalg.norm(d, axis=1)
    ia = np.floor((np.clip(a, -half, half) + half) / h)
    ib = np.floor((np.clip(b, -half, half) + half) / h)
    cnt = np.abs(ib - ia)
    with np.errstate(divide="ignore", invalid="ignore"):
        comp = np.where(cnt > 0, np.abs(d) / ln[:, None], np.inf)
    mind = comp.min(axis=1)
    return np.where(cnt.sum(axis=1) > 0, 2.0 * SNAP * cnt.sum(axis=1) / mind, 0.0)


def polyline_hits(scr, A, B, len0, tol0, g):
    """Every crossing of the stretches A -> B with screen `scr` by the rule: (stretch index, pixel,
    t, path length before the stretch, snap bound up to the crossing), after asserting that no
    crossing lies within 1e-6 of a pixel edge, a screen edge or its stretch's end."""
    d = B - A
    sep = np.linalg.norm(d, axis=1)
    d = d / sep[:, None]
    hit, t, un, vn = np_rule(scr, A, d, sep)
    eu, ev = np.array(list(scr.eu)), np.array(list(scr.ev))
    pu, pv = np.linalg.norm(eu) / scr.nu, np.linalg.norm(ev) / scr.nv  # pixel sizes
    m = 1e-6
    with np.errstate(invalid="ignore"):
        near_plane = np.isfinite(t) & (t > -m) & (t < sep + m)
        near_rect = near_plane & (un * pu > -m) & (un * pu < scr.nu * pu + m) & (vn * pv > -m) & (vn * pv < scr.nv * pv + m)
    idx = np.nonzero(near_rect)[0]
    assert np.all(np.abs(un[idx] - np.rint(un[idx])) * pu > m) and np.all(np.abs(vn[idx] - np.rint(vn[idx])) * pv > m)
    assert np.all(np.abs(t[idx] - sep[idx]) > m) and np.all(np.abs(t[idx]) > m)
    idx = np.nonzero(hit)[0]
    px = np.minimum(un[idx].astype(int), scr.nu - 1) + scr.nu * np.minimum(vn[idx].astype(int), scr.nv - 1)
    partial = snap_bound(A[idx], A[idx] + t[idx, None] * d[idx], g)
    return idx, px, t[idx], len0[idx], tol0[idx] + partial


def test_scattering_scene_against_recorded_paths():
    """Run A records every photon's path; run B, the same photons, tallies two screens inside the
    sphere. numpy intersects A's polylines with the screens: with k = 0 the fields are the integer
    hit counts, with k = PENCIL_K the sum of exp(i k (length so far + t))."""
    n, k = 2000, PENCIL_K
    sc = scene.Scene([scene.sphere(0.8, scene.mono(5.0, 1.0, 0.5, 1.0), 1), scene.box((4.0,) * 3, VAC, 2)])
    g, src = grid8(), scene.point_source((0.03, 0.05, -0.02))  # (off the voxel walls that meet at the origin)
    scr = [scene.screen((-0.4, -0.3, 0.2), (0.8, 0, 0), (0, 0.6, 0), 4, 3),
           tilted_screen((-0.05, 0.1, -0.25), nu=5, nv=7, lu=0.6, lv=0.5, at=(0.5, 0.5))]
    for s in scr:
        o, eu, ev = (np.array(list(v)) for v in (s.origin, s.eu, s.ev))
        assert all(np.linalg.norm(o + a * eu + b * ev) < 0.75 for a in (0, 1) for b in (0, 1))  # inside the sphere
    with Engine(sc, g) as eng:
        eng.set_path_tracking(range_count=n, max_vertices=64)
        a = eng.run(src, n, seed=SEED, flags=PL | abi.FLAG_TRACK_PATHS, records=True)
        hdr, vtx, counts = eng.paths()
        eng.set_path_tracking(None)
        eng.set_screens(scr)
        eng.set_phasor(0.0)
        b0 = eng.run(src, n, seed=SEED, flags=PH, records=True)
        f0 = eng.screens()
        eng.set_phasor(k)
        eng.reset_screens()
        eng.run(src, n, seed=SEED, flags=PH)
        fk = eng.screens()
    assert counts["n_dropped"] == 0 and counts["n_truncated"] == 0 and len(hdr) == n
    assert np.array_equal(hdr["photon"], np.arange(n, dtype=np.uint64))
    compare(b0, a)
    assert a.counter("scatters") > n and a.counter("faults") == 0
    # the stretches of every polyline: its vertices, then the record's final position
    A, B, len0, tol0 = [], [], [], []
    for i in range(n):
        o = int(hdr["offset"][i])
        pts = np.vstack([vtx[o:o + int(hdr["n_stored"][i]), :3], a.records["pos"][i][None, :]])
        ln = np.linalg.norm(pts[1:] - pts[:-1], axis=1)
        keep = ln > 0.0  # (an absorbed photon's last vertex is its final position)
        sb = snap_bound(pts[:-1], pts[1:], g)
        A.append(pts[:-1][keep]); B.append(pts[1:][keep])
        len0.append((np.cumsum(ln) - ln)[keep]); tol0.append((np.cumsum(sb) - sb)[keep])
    A, B, len0, tol0 = np.vstack(A), np.vstack(B), np.concatenate(len0), np.concatenate(tol0)
    for si, s in enumerate(scr):
        idx, px, t, l0, tol = polyline_hits(s, A, B, len0, tol0, g)
        npx = s.nu * s.nv
        count = np.bincount(px, minlength=npx).astype(np.float64)
        assert len(idx) > 20 * npx // 4
        assert np.array_equal(f0[si].ravel(), count.astype(np.complex128)), si  # k = 0: exact, imaginary part 0
        want, own, atol = np.zeros(npx, dtype=np.complex128), np.zeros(npx, dtype=np.complex128), np.zeros(npx)
        np.add.at(want, px, np.exp(1j * k * (l0 + t)))
        np.add.at(own, px, np.exp(1j * k * t))
        np.add.at(atol, px, k * tol)
        print(f"screen {si}: {len(idx)} hits, per-pixel tolerance median {np.median(atol):.3e}, max {atol.max():.3e}")
        assert_close(fk[si].ravel(), want, atol, f"scattering scene, screen {si}")
        miss = np.maximum(np.abs((own - want).real), np.abs((own - want).imag))
        assert np.count_nonzero(miss > 10.0 * atol) > npx // 2  # teeth
        hitpx = count > 0
        assert np.count_nonzero(atol[hitpx] < 0.05 * np.abs(want[hitpx])) >= 0.9 * np.count_nonzero(hitpx)


# ---- 5. emitter phase and sampled wavelength --------------------------------------------------------
def test_dslit_emitter_phase_on_a_screen():
    """The dslit run of test_dslit_emitter_phase with a screen across the grid: each photon's start
    phase and its own k = 2 pi / lambda, rebuilt from its record as that test does."""
    lam, n = 0.01, 256
    g = scene.grid(16, 16, 16, 5, 5, 5)
    src = scene.attach_spectrum(scene.dslit_source(), scene.spectrum_constant(lam))
    scr = [scene.screen((-5, -5, 0.3), (10, 0, 0), (0, 10, 0), 8, 6)]
    with Engine(near_vacuum(6.0), g) as eng:
        eng.set_phasor()
        eng.set_screens(scr)
        res = eng.run(src, n, seed=SEED, flags=PH, records=True)
        (got,) = eng.screens()
    assert res.counter("photons") == n and res.counter("faults") == 0 and res.counter("scatters") == 0
    assert res.counter("emit_retries") == 0
    k = 2.0 * math.pi / lam
    z2 = 5.0 - (1.e-5 * (2.0 * (5.0 / 400.0)))
    z1 = (10000.0 * lam) - 5.0
    want, bare, atol = (np.zeros((6, 8), dtype=np.complex128), np.zeros((6, 8), dtype=np.complex128), np.zeros((6, 8)))
    for r in res.records:
        pos, d = np.array(r["pos"]), np.array(r["dir"])
        emit = pos + d * ((z2 - pos[2]) / d[2])
        slit = pos + d * ((z1 - pos[2]) / d[2])
        phase0 = float(np.linalg.norm(emit - slit))
        hit, t, un, vn = np_rule(scr[0], emit[None, :], d[None, :], np.array([100.0]))
        assert abs(un[0] - round(un[0])) > 1e-6 and abs(vn[0] - round(vn[0])) > 1e-6
        if not hit[0]:  # (a line that leaves the grid sideways above the screen meets its plane beside it)
            continue
        iu, iv = int(un[0]), int(vn[0])
        want[iv, iu] += np.exp(1j * k * (phase0 + t[0]))
        bare[iv, iu] += np.exp(1j * k * t[0])
        atol[iv, iu] += k * 1e-9
    assert_close(got, want, atol, "dslit on a screen")
    assert np.all(got[atol == 0.0] == 0.0) and np.sum(atol) > 0.85 * n * k * 1e-9  # (most photons score)
    miss = np.maximum(np.abs((bare - want).real), np.abs((bare - want).imag))
    assert np.count_nonzero(miss > 10.0 * atol) > np.count_nonzero(atol) // 2  # teeth: the start phase matters


# ---- 6. every PHAS instantiation -----------------------------------------------------------------
def coop_vacuum(ext):
    """Ten tops (the cooperative EVAL) that no photon interacts in: nine small index-matched
    spheres away from the pencil, in the near-vacuum box."""
    tops = [scene.sphere(0.05 * ext, VAC, i + 1,
                         transform=scene.invert(scene.translate(((-0.8 + 0.2 * i) * ext, 0.8 * ext, -0.8 * ext))))
            for i in range(9)]
    return scene.Scene(tops + [scene.box((4.0 * ext,) * 3, VAC, 10)])


KERNELS = [(gm, xsrc, coop) for gm in (2, 1, 0) for xsrc in (0, 1) for coop in (0, 1)]


@pytest.mark.parametrize("gm,xsrc,coop", KERNELS, ids=[f"G{a}-x{b}-c{c}" for a, b, c in KERNELS])
def test_pencil_on_every_instantiation(gm, xsrc, coop, monkeypatch):
    """Test 1 on transport_kernel<false, GM, XSRC, COOP, false, true>: the grid picks GM, ten tops
    COOP, and a disc source of radius 0 (the general emitter's pencil) XSRC. Lengths scale with the
    grid's half-extent and k with its inverse."""
    monkeypatch.setenv("SMCRT_LEAN", "0")
    nx, ny, nz, ext = SMALL_GRIDS[gm]
    n, k = 200, PENCIL_K / ext
    start = tuple(ext * v for v in PENCIL_START)
    sc = coop_vacuum(ext) if coop else near_vacuum(2.0 * ext)
    g = scene.grid(nx, ny, nz, ext, ext, ext)
    src = scene.circular_source(start, PENCIL_DIR, 0.0) if xsrc else scene.pencil_source(start, PENCIL_DIR)
    plan = planprobe.plan(sc, g, env={"SMCRT_LEAN": "0"})
    assert plan["status"] == abi.OK, plan["error"]
    assert plan["grid_mode"] == gm and (plan["coop_lanes"] > 0) == bool(coop)
    assert plan_cases.kernel_of(plan, xsrc)[0] == "transport_kernel"
    assert (src.kind not in (abi.SRC_POINT, abi.SRC_PENCIL, abi.SRC_UNIFORM)) == bool(xsrc)
    scr = pencil_screens(ext)
    with Engine(sc, g) as eng:
        eng.set_phasor(k)
        eng.set_screens(scr)
        res = eng.run(src, n, seed=SEED, flags=PH, records=True)
        got = eng.screens()
        kt = eng.kernel_times()
    assert kt["lean_launches"] == 0
    assert res.counter("photons") == n and res.counter("faults") == 0 and res.counter("scatters") == 0
    d = res.records["dir"][0]
    assert np.all(res.records["dir"] == d) and np.allclose(d, PENCIL_DIR, rtol=0.0, atol=1e-15)
    # (the disc source builds its position through a transform: the line is the record's, backed up)
    p = res.records["pos"][0]
    start_np = np.array(start) if not xsrc else p + d * ((start[2] - p[2]) / d[2])
    assert np.allclose(start_np, start, rtol=0.0, atol=1e-14 * ext)
    check_pencil(got, scr, start_np, d, k, n, f"G{gm}-x{xsrc}-c{coop}")


TWELVE = [c for c in FLAG_CASES if not c[-1]]  # (without the far-field extra: one case per kernel)


@pytest.mark.parametrize("case", TWELVE, ids=[c[0] for c in TWELVE])
def test_screens_change_nothing_else(case, monkeypatch):
    """The scattering scenes of test_flag_changes_nothing_else, one per PHAS instantiation: a phasor
    run with screens against the same run without them. Counters, records, absorb, emission and
    detector bins equal, jmean and the phasor grid at 1e-12. The screens themselves: one rectangle
    taken from both sides is the sum of the two one-sided ones, and a screen outside the medium,
    placed between them in the list, stays exactly 0."""
    name, make_scene, (nx, ny, nz, ext), make_src, n, gm, xsrc, coop, far = case
    monkeypatch.setenv("SMCRT_LEAN", "0")
    sc, g, src = make_scene(), scene.grid(nx, ny, nz, ext, ext, ext), make_src()
    rect = ((-0.7 * ext, -0.6 * ext, 0.13 * ext), (1.4 * ext, 0, 0), (0, 1.2 * ext, 0), 3, 4)
    # (every scene here ends at a bounding box of half-width 1. The rule takes `dir` for a unit
    # vector, as the detectors do; the disc source keeps its direction (1, 2, 2) as given, as the
    # reference does, so until such a photon scatters its legs count three times their length.
    # No leg reaches 20.)
    scr = [scene.screen(*rect, sides=0), scene.screen((-1.0, -1.0, -20.0), (2.0, 0, 0), (0, 2.0, 0), 2, 5),
           scene.screen(*rect, sides=+1), scene.screen(*rect, sides=-1)]
    with Engine(sc, g) as eng:
        eng.set_phasor(3.0 / ext)
        bare = eng.run(src, n, seed=SEED, flags=PH, records=True)
        ph_bare = eng.phasor()
        eng.reset_phasor()
        eng.set_screens(scr)
        with_scr = eng.run(src, n, seed=SEED, flags=PH, records=True)
        ph_scr = eng.phasor()
        both, outside, up, down = eng.screens()
    compare(with_scr, bare)
    np.testing.assert_allclose(ph_scr, ph_bare, rtol=RTOL, atol=1e-300)
    assert np.all(outside == 0.0)
    hits = np.abs(up).sum() + np.abs(down).sum()
    if not coop:  # (the scattering sphere: photons cross the rectangle both ways)
        assert np.count_nonzero(both) > 0 and hits > 20.0
    np.testing.assert_allclose(both, up + down, rtol=0.0, atol=1e-12 * max(hits, 1.0))


# ---- 7. accumulate, reset, off; refusals ------------------------------------------------------------
def test_accumulate_reset_and_off():
    sc, g, src = near_vacuum(2.0), grid8(), scene.pencil_source(PENCIL_START, PENCIL_DIR)
    scr = pencil_screens()
    L = load_library()
    with Engine(sc, g) as eng:
        eng.set_screens(scr)
        n_, nd = C.c_int32(), C.c_int64()
        _check(L.smcrt_scene_screen_info(eng._h, C.byref(n_), C.byref(nd)))
        assert (n_.value, nd.value) == (4, 2 * (1 + 12 + 4 + 15))
        # screens without a phasor configuration: a plain run works and tallies nothing
        eng.run(src, 50, seed=SEED, flags=PL)
        assert all(np.all(f == 0.0) for f in eng.screens())
        with pytest.raises(SmcrtError, match="INVALID_ARG"):  # the flag still needs smcrt_scene_set_phasor
            eng.run(src, 50, seed=SEED, flags=PH)
        eng.set_phasor(PENCIL_K)
        eng.run(src, 100, seed=SEED, flags=PH)
        a = eng.screens()
        eng.reset_screens()
        assert all(np.all(f == 0.0) for f in eng.screens())
        eng.run(src, 50, seed=SEED, flags=PH, first_photon=100)
        b = eng.screens()
        eng.reset_screens()
        eng.run(src, 100, seed=SEED, flags=PH)
        eng.run(src, 50, seed=SEED, flags=PH, first_photon=100)
        both = eng.screens()
        for fa, fb, fab in zip(a, b, both):
            np.testing.assert_allclose(fab, fa + fb, rtol=RTOL, atol=1e-300)
        assert abs(both[0][0, 0]) > 149.0
        eng.run(src, 50, seed=SEED, flags=PL)  # a run without the flag leaves the fields alone
        assert all(np.array_equal(x, y) for x, y in zip(eng.screens(), both))
        eng.set_phasor(PENCIL_K)  # (a new phasor configuration does not touch the screens)
        assert all(np.array_equal(x, y) for x, y in zip(eng.screens(), both))
        out = np.ones(nd.value)  # the reader adds into its output
        _check(L.smcrt_scene_read_screens(eng._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        flat = np.concatenate([f.ravel().view(np.float64) for f in both])
        assert np.array_equal(out, 1.0 + flat)
        eng.set_screens(scr[:2])  # a new list starts from zero
        assert [f.shape for f in eng.screens()] == [(1, 1), (3, 4)] and all(np.all(f == 0.0) for f in eng.screens())
        eng.set_screens(None)
        _check(L.smcrt_scene_screen_info(eng._h, C.byref(n_), C.byref(nd)))
        assert (n_.value, nd.value) == (0, 0)
        with pytest.raises(SmcrtError, match="INVALID_ARG"):
            eng.screens()
        with pytest.raises(SmcrtError, match="INVALID_ARG"):
            eng.reset_screens()
        eng.run(src, 50, seed=SEED, flags=PH)  # a phasor run without screens is what it was
        assert np.count_nonzero(eng.phasor()) > 10
        bad = pencil_screens()
        bad[2].nu = 0
        with pytest.raises(SmcrtError, match="INVALID_ARG.*screen 2"):
            eng.set_screens(bad)
        cfg = abi.PhasorConfig()
        cfg.reserved = 2  # (bit 0 is the only option)
        assert L.smcrt_scene_set_phasor(eng._h, C.byref(cfg)) == abi.ERR_INVALID_ARG
        assert b"reserved" in L.smcrt_last_error()
        assert np.count_nonzero(eng.phasor()) > 10  # (a refused configuration changes nothing)


def test_refused_on_voxel_and_mesh_scenes():
    from tests import mesh_cases as M
    from tests.test_gpu_voxel import pattern_case
    vs, vg, _ = pattern_case(2)
    for sc, g, kind in ((vs, vg, "voxel"), (M.nested_scene(), M.grid16(), "mesh")):
        with Engine(sc, g) as eng:
            with pytest.raises(SmcrtError, match=f"UNSUPPORTED.*{kind}"):
                eng.set_screens(pencil_screens())
            with pytest.raises(SmcrtError, match=f"UNSUPPORTED.*{kind}"):
                eng.screens()
            with pytest.raises(SmcrtError, match=f"UNSUPPORTED.*{kind}"):
                eng.reset_screens()
            with pytest.raises(SmcrtError, match=f"UNSUPPORTED.*{kind}"):
                eng.set_phasor(1.0, optical_path=True)
            with pytest.raises(SmcrtError, match="INVALID_ARG.*screen 0"):  # (validation comes first)
                bad = pencil_screens()
                bad[0].sides = 3
                eng.set_screens(bad)
