"""Test infrastructure only: closed-form per-voxel expectations that need neither the engine nor
its CPU restatement. Plain numpy in float64; everything is passed in as numbers.

Grids are given by their three arrays of voxel faces (`faces(n, half)`), results have the shape
(nz, ny, nx) of rsmcrt_amd.tallies.Result.

  point_source_track   scene A: an isotropic point source in a homogeneous absorber
  point_source_escape  scene A: the probability of leaving the grid unabsorbed
  beam_slab            scene B: a pencil beam through an index-mismatched absorbing slab
  beam_legs            scene D: the same beam against any surface given as a ray cast
  cast_sphere, cast_triangles   scene D: the casts of a sphere and of a closed triangle surface
  sphere_beam_series   scene D: the geometric series of a beam's legs inside a sphere
  centre_source_sphere scene D: a point source at the centre of an absorbing glass sphere

and per-bin expectations of the detectors (their hit rules are stated above circle_edges):

  point_source_disc_bins  scene A: the rings of a circle or annulus detector anywhere in space
  point_source_rect       scene A: a camera's rectangle, and the one pixel its hits go to
  fibre_bins              scene A: a fibre detector whose axis passes through the source
  beam_slab_legs, legs_on_disc  scene B: where each leg of the beam lands on a disc

and the exact voxel-layer expectations of a homogeneous scattering medium without walls:

  scatter_cumulative, scatter_layers_point, scatter_layers_beam  absorptions per layer along an axis
  scatter_mgf, scatter_tail_bound   the moment generating function of the absorption site, and
                                    Chernoff's bound on its tails (for the expected escapes)
  scatter_moments                   exact second and first moments, scatterings per photon
"""
from __future__ import annotations

import math

import numpy as np

GL_ORDER = 32


def faces(n: int, half: float) -> np.ndarray:
    """The n + 1 faces of n equal voxels over [-half, half]."""
    return -float(half) + (2.0 * float(half) / int(n)) * np.arange(int(n) + 1)


def _gl(order=GL_ORDER):
    x, w = np.polynomial.legendre.leggauss(order)
    return 0.5 * (x + 1.0), 0.5 * w  # on [0, 1]


# ---------------------------------------------------------------------------- scene A ----
# Per photon the expected track length in a region V is T(V) = int_V exp(-mu r) / (4 pi r^2) dV
# and the probability of being absorbed there mu T(V). In spherical coordinates about the source
# the radial integral is closed: with Phi(rho) = (1 - exp(-mu rho)) / (4 pi mu), Phi(0) = 0,
#   T(V) = int dOmega [Phi(rho_out) - Phi(rho_in)].
# For a box every rho_in/out lies on a face, and on the face in the plane at signed height h from
# the source dOmega = |h| / rho^3 dA, so
#   T(box) = sum over its six faces of  sign * int int h Phi(rho) / rho^3 dA,   rho^2 = u^2 + v^2 + h^2,
# with h measured along the outward normal. Each term is the pyramid from the source to that face:
# this is the inclusion-exclusion of corner boxes, summed face by face, so that no term needs the
# singular point. The integrand is smooth on a face; a voxel face is one Gauss-Legendre panel.

def _phi(rho, mu):
    if mu == 0.0:
        return rho / (4.0 * math.pi)
    return -np.expm1(-mu * rho) / (4.0 * math.pi * mu)


def _panel_integrals(h, ue, ve, f, order):
    """int int over every panel [ue[a], ue[a+1]] x [ve[b], ve[b+1]] of h f(rho) / rho^3 for each
    height h[c]: array [c, b, a]. Coordinates are relative to the source."""
    x, w = _gl(order)
    u = ue[:-1, None] + np.diff(ue)[:, None] * x[None, :]           # [a, i]
    wu = np.diff(ue)[:, None] * w[None, :]
    v = ve[:-1, None] + np.diff(ve)[:, None] * x[None, :]           # [b, j]
    wv = np.diff(ve)[:, None] * w[None, :]
    out = np.empty((len(h), len(ve) - 1, len(ue) - 1))
    for c, hc in enumerate(h):
        rho = np.sqrt(u[None, :, None, :] ** 2 + v[:, None, :, None] ** 2 + hc * hc)  # [b, a, j, i]
        g = hc * f(rho) / rho ** 3
        out[c] = np.einsum("baji,bj,ai->ba", g, wv, wu)
    return out


def _face_terms(xe, ye, ze, src, f, order):
    """The pyramid integral of every voxel face: (Jx[k, j, i'], Jy[k, j', i], Jz[k', j, i]) for the
    faces normal to x, y and z (primes: face indices, one more than voxels)."""
    x, y, z = (np.asarray(e, dtype=np.float64) - s for e, s in zip((xe, ye, ze), src))
    jx = _panel_integrals(x, y, z, f, order)   # [i', k, j]  (u = y, v = z)
    jy = _panel_integrals(y, x, z, f, order)   # [j', k, i]
    jz = _panel_integrals(z, x, y, f, order)   # [k', j, i]
    return jx.transpose(1, 2, 0), jy.transpose(1, 0, 2), jz


def point_source_track(xe, ye, ze, src, mu, order=GL_ORDER) -> np.ndarray:
    """T(V) of every voxel of the grid with faces xe, ye, ze: the expected track length per photon
    of an isotropic point source at `src` (on no face) in a homogeneous medium with mus = 0 and
    mua = mu. The probability of absorption in V is mu * T(V). mu = 0 gives the integral of
    1 / (4 pi r^2) and mu < 0 that of exp(|mu| r) / (4 pi r^2) (a stream that runs towards the
    source, scene D): Phi is the same radial integral for either sign."""
    mu = float(mu)
    for e, s in zip((xe, ye, ze), src):
        assert np.min(np.abs(np.asarray(e) - s)) > 0.0, "the source lies on a voxel face"
    jx, jy, jz = _face_terms(xe, ye, ze, src, lambda r: _phi(r, mu), order)
    return (jx[:, :, 1:] - jx[:, :, :-1]) + (jy[:, 1:, :] - jy[:, :-1, :]) + (jz[1:] - jz[:-1])


def point_source_escape(xe, ye, ze, src, mu, order=GL_ORDER) -> float:
    """P(the photon leaves the grid): int int h exp(-mu rho) / (4 pi rho^3) over the six outer
    faces, in the same panels. Not derived from point_source_track: their sum closing to 1 is a check."""
    mu = float(mu)
    jx, jy, jz = _face_terms(xe, ye, ze, src, lambda r: np.exp(-mu * r) / (4.0 * math.pi), order)
    return float((jx[:, :, -1] - jx[:, :, 0]).sum() + (jy[:, -1, :] - jy[:, 0, :]).sum() + (jz[-1] - jz[0]).sum())


def point_source_track_direct(xe, ye, ze, src, mu, order=GL_ORDER) -> np.ndarray:
    """The same T(V) as a tensor Gauss-Legendre integral of exp(-mu r) / (4 pi r^2) over each voxel:
    valid where the voxel does not hold the source (there it is NaN). A self-check only."""
    x, w = _gl(order)

    def nodes(e, s):
        e = np.asarray(e, dtype=np.float64) - s
        return e[:-1, None] + np.diff(e)[:, None] * x[None, :], np.diff(e)[:, None] * w[None, :]

    (px, wx), (py, wy), (pz, wz) = nodes(xe, src[0]), nodes(ye, src[1]), nodes(ze, src[2])
    out = np.empty((len(ze) - 1, len(ye) - 1, len(xe) - 1))
    for k in range(out.shape[0]):
        r2 = (pz[k][:, None, None, None, None] ** 2 + py[None, :, None, :, None] ** 2
              + px[None, None, :, None, :] ** 2)                    # [c, j, i, b, a]
        g = np.exp(-mu * np.sqrt(r2)) / (4.0 * math.pi * r2)
        out[k] = np.einsum("cjiba,c,jb,ia->ji", g, wz[k], wy, wx)
    i, j, k = (int(np.searchsorted(e, s)) - 1 for e, s in zip((xe, ye, ze), src))
    out[k, j, i] = np.nan
    return out


# ---------------------------------------------------------------------------- scene B ----
def fresnel_unpolarised(cos1, n1, n2, polarisation="unpolarised"):
    """(R, cos2): the reflectance of a plane interface from n1 into n2 at incidence cosine cos1
    and the cosine of the refracted ray; R = 1 and cos2 = None under total internal reflection.
    polarisation "s" or "p" gives that component alone (used only by a negative control)."""
    sin2 = (n1 / n2) ** 2 * (1.0 - cos1 * cos1)
    if sin2 >= 1.0:
        return 1.0, None
    cos2 = math.sqrt(1.0 - sin2)
    rs = ((n1 * cos1 - n2 * cos2) / (n1 * cos1 + n2 * cos2)) ** 2
    rp = ((n1 * cos2 - n2 * cos1) / (n1 * cos2 + n2 * cos1)) ** 2
    return {"unpolarised": 0.5 * (rs + rp), "s": rs, "p": rp}[polarisation], cos2


def _clip(lo, hi, o, d, s_max):
    """Slab method on all voxels at once: the parameter interval [s0, s1] of the ray o + s d,
    0 <= s <= s_max, inside each box [lo, hi] (arrays [..., 3]); s1 < s0 where it misses."""
    s0 = np.zeros(lo.shape[:-1])
    s1 = np.full(lo.shape[:-1], float(s_max))
    for a in range(3):
        if d[a] == 0.0:
            miss = (o[a] < lo[..., a]) | (o[a] > hi[..., a])
            s1 = np.where(miss, -1.0, s1)
            continue
        ta, tb = (lo[..., a] - o[a]) / d[a], (hi[..., a] - o[a]) / d[a]
        s0 = np.maximum(s0, np.minimum(ta, tb))
        s1 = np.minimum(s1, np.maximum(ta, tb))
    return s0, s1


def beam_slab(xe, ye, ze, origin, direction, z_half, n_in, mu_in, n_out=1.0, q_min=1e-14,
              polarisation="unpolarised"):
    """A pencil beam from `origin` along `direction` through the slab |z| < z_half (index n_in,
    mua = mu_in, mus = 0) in a medium of index n_out without absorption or scattering, both wider
    than the grid, which ends the world. Returns (track, p_abs): per photon and voxel the expected
    track length and the probability of absorption. Every leg that carries more than q_min is
    followed through reflection and refraction at the two planes."""
    xe, ye, ze = (np.asarray(e, dtype=np.float64) for e in (xe, ye, ze))
    zz, yy, xx = np.meshgrid(np.arange(len(ze) - 1), np.arange(len(ye) - 1), np.arange(len(xe) - 1), indexing="ij")
    lo = np.stack([xe[xx], ye[yy], ze[zz]], axis=-1)
    hi = np.stack([xe[xx + 1], ye[yy + 1], ze[zz + 1]], axis=-1)
    glo = np.array([xe[0], ye[0], ze[0]])
    ghi = np.array([xe[-1], ye[-1], ze[-1]])
    track = np.zeros(lo.shape[:-1])
    p_abs = np.zeros(lo.shape[:-1])
    d0 = np.asarray(direction, dtype=np.float64)
    d0 = d0 / math.sqrt(float(d0 @ d0))
    o0 = np.asarray(origin, dtype=np.float64)
    assert abs(o0[2]) != z_half and np.all(o0 > glo) and np.all(o0 < ghi)
    legs = [(o0, d0, 1.0, abs(o0[2]) < z_half)]
    while legs:
        o, d, q, inside = legs.pop()
        mu = mu_in if inside else 0.0
        # the grid's exit and the next plane
        _, s_exit = _clip(glo, ghi, o, d, math.inf)
        s_exit = float(s_exit)
        s_plane, z_plane = math.inf, 0.0
        if d[2] != 0.0:
            for zp in (-z_half, z_half):
                s = (zp - o[2]) / d[2]
                if s > 1e-12 and s < s_plane:  # (the leg starts on one of the planes, or between them)
                    s_plane, z_plane = s, zp
        s_end = min(s_exit, s_plane)
        s0, s1 = _clip(lo, hi, o, d, s_end)
        hit = s1 - s0 > 1e-12  # (a plane in a voxel face: no sliver of rounding error in the voxel beyond)
        if mu > 0.0:
            w = np.where(hit, np.exp(-mu * np.where(hit, s0, 0.0)) - np.exp(-mu * np.where(hit, s1, 0.0)), 0.0)
            track += q * w / mu
            p_abs += q * w
        else:
            track += q * np.where(hit, s1 - s0, 0.0)
        if s_plane >= s_exit:
            continue
        q = q * math.exp(-mu * s_plane)
        if q < q_min:
            continue
        p = o + s_plane * d
        p[2] = z_plane
        n1, n2 = (n_in, n_out) if inside else (n_out, n_in)
        cos1 = abs(d[2])
        r, cos2 = fresnel_unpolarised(cos1, n1, n2, polarisation)
        if q * r >= q_min:
            legs.append((p, np.array([d[0], d[1], -d[2]]), q * r, inside))
        if cos2 is not None and q * (1.0 - r) >= q_min:
            eta = n1 / n2
            t = np.array([eta * d[0], eta * d[1], math.copysign(cos2, d[2])])  # Snell: the tangential part scales
            legs.append((p, t, q * (1.0 - r), not inside))
    return track, p_abs


def beam_slab_legs(xe, ye, ze, origin, direction, z_half, n_in, n_out=1.0, mu_in=0.0, q_min=1e-14,
                   polarisation="unpolarised"):
    """The legs beam_slab follows, as a list of (origin, direction, q, length, inside): q is the
    probability that a photon walks this leg at all (the Fresnel choices and the absorption on the
    legs before it), length its run to the next plane or to the grid's wall, inside whether it lies
    in the slab (where a photon survives a run s with probability exp(-mu_in s))."""
    xe, ye, ze = (np.asarray(e, dtype=np.float64) for e in (xe, ye, ze))
    glo = np.array([xe[0], ye[0], ze[0]])
    ghi = np.array([xe[-1], ye[-1], ze[-1]])
    d0 = np.asarray(direction, dtype=np.float64)
    d0 = d0 / math.sqrt(float(d0 @ d0))
    o0 = np.asarray(origin, dtype=np.float64)
    assert abs(o0[2]) != z_half and np.all(o0 > glo) and np.all(o0 < ghi)
    todo = [(o0, d0, 1.0, abs(o0[2]) < z_half)]
    out = []
    while todo:
        o, d, q, inside = todo.pop()
        mu = mu_in if inside else 0.0
        _, s_exit = _clip(glo, ghi, o, d, math.inf)
        s_exit = float(s_exit)
        s_plane, z_plane = math.inf, 0.0
        if d[2] != 0.0:
            for zp in (-z_half, z_half):
                s = (zp - o[2]) / d[2]
                if s > 1e-12 and s < s_plane:
                    s_plane, z_plane = s, zp
        out.append((o, d, q, min(s_exit, s_plane), inside))
        if s_plane >= s_exit:
            continue
        q = q * math.exp(-mu * s_plane)
        if q < q_min:
            continue
        p = o + s_plane * d
        p[2] = z_plane
        n1, n2 = (n_in, n_out) if inside else (n_out, n_in)
        r, cos2 = fresnel_unpolarised(abs(d[2]), n1, n2, polarisation)
        if q * r >= q_min:
            todo.append((p, np.array([d[0], d[1], -d[2]]), q * r, inside))
        if cos2 is not None and q * (1.0 - r) >= q_min:
            eta = n1 / n2
            todo.append((p, np.array([eta * d[0], eta * d[1], math.copysign(cos2, d[2])]), q * (1.0 - r), not inside))
    return out


# ---------------------------------------------------------------------------- scene D ----
# Curved surfaces. Nothing scatters, so a photon's path is a tree of straight legs with Fresnel
# probabilities at the nodes; the surface enters only as a ray cast, `cast(o, d)` -> None or
# (s, N[, b]): the distance s > 0 to the next surface point along the unit vector d, the unit
# normal N there pointing out of the body, and for a triangle surface the smallest barycentric
# coordinate b of the hit in its facet.
CAST_EPS = 1e-9   # a leg that starts on the surface does not meet it again at its own origin


def cast_sphere(centre, radius):
    """The cast of the sphere |x - centre| = radius: the roots of s^2 + 2 (oc . d) s + |oc|^2 - R^2
    and the radial normal."""
    c, r = np.asarray(centre, dtype=np.float64), float(radius)

    def cast(o, d):
        oc = o - c
        b = float(oc @ d)
        disc = b * b - (float(oc @ oc) - r * r)
        if disc <= 0.0:
            return None
        root = math.sqrt(disc)
        for s in (-b - root, -b + root):
            if s > CAST_EPS:
                p = oc + s * d
                return s, p / math.sqrt(float(p @ p))
        return None
    return cast


def cast_triangles(verts, tris):
    """The cast of a closed surface of triangles wound anticlockwise seen from outside: every
    triangle is tried (Moeller-Trumbore: the ray's point o + s d written as v0 + u e1 + v e2 by
    Cramer's rule), the nearest hit wins, the normal is e1 x e2 of that facet."""
    verts = np.asarray(verts, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    v0 = verts[tris[:, 0]]
    e1, e2 = verts[tris[:, 1]] - v0, verts[tris[:, 2]] - v0
    nrm = np.cross(e1, e2)
    nrm = nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]

    def cast(o, d):
        pv = np.cross(d[None, :], e2)
        det = (e1 * pv).sum(axis=1)
        ok = det != 0.0
        inv = 1.0 / np.where(ok, det, 1.0)
        tv = o[None, :] - v0
        u = (tv * pv).sum(axis=1) * inv
        qv = np.cross(tv, e1)
        v = (qv * d[None, :]).sum(axis=1) * inv
        s = (e2 * qv).sum(axis=1) * inv
        bary = np.minimum(np.minimum(u, v), 1.0 - u - v)
        hit = ok & (bary >= 0.0) & (s > CAST_EPS)
        if not hit.any():
            return None
        i = int(np.argmin(np.where(hit, s, np.inf)))
        return float(s[i]), nrm[i], float(bary[i])
    return cast


def tilted(cast, axis, angle):
    """`cast` with every normal turned by `angle` about `axis` (Rodrigues). A negative control."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / math.sqrt(float(k @ k))

    def wrapped(o, d):
        hit = cast(o, d)
        if hit is None:
            return None
        n = hit[1]
        n = n * math.cos(angle) + np.cross(k, n) * math.sin(angle) + k * float(k @ n) * (1.0 - math.cos(angle))
        return (hit[0], n) + tuple(hit[2:])
    return wrapped


def beam_legs(xe, ye, ze, origin, direction, cast, n_in, n_out, mu_in, q_min, polarisation="unpolarised",
              exit_normal_unturned=False):
    """beam_slab for any body: a pencil beam from `origin` (inside the grid, which ends the world)
    along `direction` against the body whose surface is `cast` (index n_in, mua = mu_in, mus = 0;
    around it index n_out, no absorption). At a hit with outward normal N and incidence cosine
    c1 = |d . N| the reflected leg is d - 2 (d . N) N and the refracted one
    eta d + (eta c1 - c2) m, eta = n1 / n2, m the normal turned against the ray. Every leg that
    carries q >= q_min is followed. Returns (track, p_abs, legs, hits, paths): the grids of
    beam_slab, the legs in the format of beam_slab_legs, per followed surface hit
    (point, c1, q on arrival, from inside?, barycentric minimum or None), and per leg the tuple of
    the crossings before it, in order, each as (c1, the cosine the path left the surface with:
    c1 reflected, c2 refracted).
    exit_normal_unturned (a negative control) refracts an outgoing ray about N as it stands."""
    xe, ye, ze = (np.asarray(e, dtype=np.float64) for e in (xe, ye, ze))
    zz, yy, xx = np.meshgrid(np.arange(len(ze) - 1), np.arange(len(ye) - 1), np.arange(len(xe) - 1), indexing="ij")
    lo = np.stack([xe[xx], ye[yy], ze[zz]], axis=-1)
    hi = np.stack([xe[xx + 1], ye[yy + 1], ze[zz + 1]], axis=-1)
    glo = np.array([xe[0], ye[0], ze[0]])
    ghi = np.array([xe[-1], ye[-1], ze[-1]])
    track = np.zeros(lo.shape[:-1])
    p_abs = np.zeros(lo.shape[:-1])
    d0 = np.asarray(direction, dtype=np.float64)
    d0 = d0 / math.sqrt(float(d0 @ d0))
    o0 = np.asarray(origin, dtype=np.float64)
    assert np.all(o0 > glo) and np.all(o0 < ghi)
    first = cast(o0, d0)
    todo = [(o0, d0, 1.0, first is not None and float(first[1] @ d0) > 0.0, ())]  # leaving first: it starts inside
    legs, hits, paths = [], [], []
    while todo:
        o, d, q, inside, path = todo.pop()
        mu = mu_in if inside else 0.0
        _, s_exit = _clip(glo, ghi, o, d, math.inf)
        s_exit = float(s_exit)
        hit = cast(o, d)
        s_hit = math.inf if hit is None else hit[0]
        s_end = min(s_exit, s_hit)
        legs.append((o, d, q, s_end, inside))
        paths.append(path)
        s0, s1 = _clip(lo, hi, o, d, s_end)
        on = s1 - s0 > 1e-12
        if mu > 0.0:
            w = np.where(on, np.exp(-mu * np.where(on, s0, 0.0)) - np.exp(-mu * np.where(on, s1, 0.0)), 0.0)
            track += q * w / mu
            p_abs += q * w
        else:
            track += q * np.where(on, s1 - s0, 0.0)
        if s_hit >= s_exit:
            continue
        q = q * math.exp(-mu * s_hit)
        if q < q_min:
            continue
        p = o + s_hit * d
        nrm = hit[1]
        dn = float(d @ nrm)
        assert (dn > 0.0) == inside, "the surface is met from the wrong side"
        n1, n2 = (n_in, n_out) if inside else (n_out, n_in)
        c1 = abs(dn)
        r, c2 = fresnel_unpolarised(c1, n1, n2, polarisation)
        hits.append((p, c1, q, inside, hit[2] if len(hit) > 2 else None))
        if q * r >= q_min:
            todo.append((p, d - 2.0 * dn * nrm, q * r, inside, path + ((c1, c1),)))
        if c2 is not None and q * (1.0 - r) >= q_min:
            eta = n1 / n2
            m = nrm if (dn < 0.0 or exit_normal_unturned) else -nrm
            t = eta * d + (eta * c1 - c2) * m
            todo.append((p, t / math.sqrt(float(t @ t)), q * (1.0 - r), not inside, path + ((c1, c2),)))
    return track, p_abs, legs, hits, paths


def leg_voxels(xe, ye, ze, leg):
    """The length of one leg (o, d, q, length, inside) in every voxel, (nz, ny, nx)."""
    xe, ye, ze = (np.asarray(e, dtype=np.float64) for e in (xe, ye, ze))
    zz, yy, xx = np.meshgrid(np.arange(len(ze) - 1), np.arange(len(ye) - 1), np.arange(len(xe) - 1), indexing="ij")
    lo = np.stack([xe[xx], ye[yy], ze[zz]], axis=-1)
    hi = np.stack([xe[xx + 1], ye[yy + 1], ze[zz + 1]], axis=-1)
    s0, s1 = _clip(lo, hi, leg[0], leg[1], leg[3])
    return np.where(s1 - s0 > 1e-12, s1 - s0, 0.0)


def ball_voxels(xe, ye, ze, centre, radius):
    """(inside, outside): the voxels wholly inside and wholly outside the ball, (nz, ny, nx), by
    the farthest and the nearest point of each voxel from the centre."""
    near2, far2 = 0.0, 0.0
    for e, s, shape in ((xe, centre[0], (1, 1, -1)), (ye, centre[1], (1, -1, 1)), (ze, centre[2], (-1, 1, 1))):
        e = np.asarray(e, dtype=np.float64)
        a, b = e[:-1] - s, e[1:] - s
        near = np.where((a < 0.0) & (b > 0.0), 0.0, np.minimum(np.abs(a), np.abs(b)))
        near2 = near2 + (near ** 2).reshape(shape)
        far2 = far2 + (np.maximum(np.abs(a), np.abs(b)) ** 2).reshape(shape)
    return far2 < radius * radius, near2 > radius * radius


def sphere_beam_series(sin_i, radius, n, mu, from_inside=False, first_run=0.0):
    """The legs of a beam in a sphere of index n and mua = mu in vacuum, in closed form. A ray that
    meets a sphere at the incidence angle i keeps it at every later hit, so every interior chord is
    c = 2 R cos t (t the angle inside) and every hit has one reflectance rho.
    From outside (sin_i = impact parameter / R): interior leg k starts with q_k = (1 - rho) (rho a)^k,
    a = exp(-mu c). From inside (sin_i the sine inside, first_run the run to the first hit):
    q_0 = 1 and q_k = exp(-mu first_run) rho^k a^(k-1).
    Returns a dict: rho, chord, absorbed, escaped, reflected (the share that never enters) and
    q(k)."""
    if from_inside:
        cos_t = math.sqrt(1.0 - sin_i * sin_i)
        rho, _ = fresnel_unpolarised(cos_t, n, 1.0)
        chord = 2.0 * radius * cos_t
        a, a0 = math.exp(-mu * chord), math.exp(-mu * first_run)
        escaped = a0 * (1.0 - rho) / (1.0 - rho * a) if rho * a < 1.0 else 0.0
        return {"rho": rho, "chord": chord, "escaped": escaped, "absorbed": 1.0 - escaped, "reflected": 0.0,
                "q": lambda k: 1.0 if k == 0 else a0 * rho ** k * a ** (k - 1)}
    rho, cos_t = fresnel_unpolarised(math.sqrt(1.0 - sin_i * sin_i), 1.0, n)
    back, _ = fresnel_unpolarised(cos_t, n, 1.0)
    assert abs(back - rho) < 1e-14   # (Stokes: the same reflectance from either side)
    chord = 2.0 * radius * cos_t
    a = math.exp(-mu * chord)
    absorbed = (1.0 - rho) * (1.0 - a) / (1.0 - rho * a)
    return {"rho": rho, "chord": chord, "absorbed": absorbed, "escaped": rho + (1.0 - rho) ** 2 * a / (1.0 - rho * a),
            "reflected": rho, "q": lambda k: (1.0 - rho) * (rho * a) ** k}


def centre_source_sphere(xe, ye, ze, centre, radius, n, mu, order=GL_ORDER):
    """An isotropic point source at the centre of a sphere (index n, mua = mu > 0, mus = 0) in
    vacuum: every ray meets the surface at normal incidence, reflects with r0 = ((n - 1) / (n + 1))^2
    and runs back along its diameter, through the centre and on to the opposite side. With
    D = 1 - r0 exp(-2 mu R) the expected track density per photon is g(r) / (4 pi r^2),
      inside   g = [exp(-mu r) + r0 exp(-mu (2 R - r))] / D   (the streams away from and towards the centre),
      outside  g = (1 - r0) exp(-mu R) / D = P(escape the sphere),
    so a voxel wholly inside holds [T(mu) + r0 exp(-2 mu R) T(-mu)] / D and one wholly outside
    g T(0), T = point_source_track. The voxels the surface cuts are given as one pooled sum, exact
    by conservation: the interior track is P(absorbed) / mu in all, the exterior track inside the
    grid g (sum of T(0) over the grid - R), R being the integral of 1 / (4 pi r^2) over the ball.
    Returns a dict: track, p_abs (the cut voxels hold NaN), inside, outside, cut (masks),
    cut_track, cut_p_abs, p_escape (from the sphere; no photon is absorbed outside)."""
    xe, ye, ze = (np.asarray(e, dtype=np.float64) for e in (xe, ye, ze))
    c, r, mu = np.asarray(centre, dtype=np.float64), float(radius), float(mu)
    assert mu > 0.0
    r0 = ((n - 1.0) / (n + 1.0)) ** 2
    dd = 1.0 - r0 * math.exp(-2.0 * mu * r)
    g_out = (1.0 - r0) * math.exp(-mu * r) / dd
    inside, outside = ball_voxels(xe, ye, ze, c, r)
    cut = ~(inside | outside)
    t_out = point_source_track(xe, ye, ze, c, mu, order)
    t_in = point_source_track(xe, ye, ze, c, -mu, order)
    t_0 = point_source_track(xe, ye, ze, c, 0.0, order)
    track = np.where(inside, (t_out + r0 * math.exp(-2.0 * mu * r) * t_in) / dd, g_out * t_0)
    p_abs = np.where(inside, mu * track, 0.0)
    p_absorbed = 1.0 - g_out
    cut_track = p_absorbed / mu + g_out * (float(t_0.sum()) - r) - float(track[~cut].sum())
    cut_p_abs = p_absorbed - float(p_abs[inside].sum())
    track[cut], p_abs[cut] = np.nan, np.nan
    return {"track": track, "p_abs": p_abs, "inside": inside, "outside": outside, "cut": cut,
            "cut_track": cut_track, "cut_p_abs": cut_p_abs, "p_escape": g_out, "r0": r0}


# --------------------------------------------------------------------------- detectors ----
# The hit rules, read from the reference's text (geometryMod.f90:217-270, detector_base.f90:137-235,
# detectors.f90:147-469). A flight leg from l0 along the unit vector l of length L meets the plane
# through `centre` with unit normal n at t = dot(centre - l0, n) / dot(n, l).
#   circle   hit when dot(n, l) > 1e-6 (oriented: only photons going along n), 0 < t <= L and the
#            landing radius r <= R. Bin nint(r / w) + 1, at most nbins + 1, w = R / nbins: the
#            nbins + 1 bins have the edges 0, w/2, 3w/2, ..., (nbins - 1/2) w, R, the first and the
#            last half as wide as the others. nbins = 0: one bin (w = 1 and the clamp).
#   annulus  "not inside r1, inside r2" with the same plane rule: r1 < r <= r2, binned by r - r1
#            with w = (r2 - r1) / nbins.
#   fibre    a circle of the front aperture on the front lens, then a thin-lens chain in (radius,
#            gradient) with signed comparisons (fibre_bins).
#   camera   NOT oriented and NOT windowed: t = dot(p1 - l0, n) / dot(l, n) >= 0 and the landing
#            point strictly inside the rectangle is all check_hit_camera asks (detectors.f90:460-468),
#            so every leg whose forward ray meets the rectangle counts, whether or not the photon
#            gets there. record_hit_2D then files the hit, with weight 1, into the pixel of the
#            leg's START (hit%pos), x = start.z + p1.x, y = start.y + p1.y, int() and not nint(),
#            out of nbins + 1 pixels per side. That is the reference's behaviour and is kept.
# The detectors' `layer` field is read by none of these rules.

def _plane_frame(normal):
    n = np.asarray(normal, dtype=np.float64)
    n = n / math.sqrt(float(n @ n))
    a = np.zeros(3)
    a[int(np.argmin(np.abs(n)))] = 1.0
    u = np.cross(n, a)
    u = u / math.sqrt(float(u @ u))
    return n, u, np.cross(n, u)


def circle_edges(radius, nbins):
    """The edges of a circle detector's nbins + 1 bins (one bin for nbins = 0)."""
    if nbins == 0:
        return np.array([0.0, float(radius)])
    w = float(radius) / nbins
    return np.concatenate([[0.0], (np.arange(nbins) + 0.5) * w, [float(radius)]])


def annulus_edges(r1, r2, nbins):
    """The edges in r of an annulus detector's nbins + 1 bins: r1 < r <= r2."""
    return float(r1) + circle_edges(float(r2) - float(r1), nbins)


def point_source_disc_bins(src, mu, centre, normal, edges, order=GL_ORDER, panels=16, windowed=True):
    """Per photon of an isotropic point source at `src` in a homogeneous absorber (mus = 0, mua =
    mu, wider than the detector's plane is far): the probability of crossing the plane through
    `centre` along `normal`, before being absorbed, at radius edges[i] < r <= edges[i + 1] from
    `centre`. With h the height of the plane above the source along the normal and s the distance
    from the source, that is the integral of h exp(-mu s) / (4 pi s^3) over the ring, here by a
    tensor Gauss-Legendre rule in polar coordinates about `centre` (`order` points per ring in r,
    `panels` panels of `order` points in the angle): the centre need not be the source's foot.
    A plane behind the source (h <= 0) is never crossed along its normal: all zeros.
    windowed=False drops exp(-mu s) (a negative control: no `t <= pointSep` window)."""
    edges = np.asarray(edges, dtype=np.float64)
    n, u, v = _plane_frame(normal)
    rel = np.asarray(centre, dtype=np.float64) - np.asarray(src, dtype=np.float64)
    h = float(rel @ n)
    out = np.zeros(len(edges) - 1)
    if h <= 0.0:
        return out
    cu, cv = float(rel @ u), float(rel @ v)   # the centre, in the plane, from the source's foot
    x, w = _gl(order)
    pe = 2.0 * math.pi * np.arange(panels + 1) / panels
    phi = (pe[:-1, None] + np.diff(pe)[:, None] * x[None, :]).ravel()
    wphi = (np.diff(pe)[:, None] * w[None, :]).ravel()
    for i in range(len(out)):
        r = edges[i] + (edges[i + 1] - edges[i]) * x
        wr = (edges[i + 1] - edges[i]) * w
        a = cu + r[:, None] * np.cos(phi)[None, :]
        b = cv + r[:, None] * np.sin(phi)[None, :]
        s = np.sqrt(a * a + b * b + h * h)
        g = h / (4.0 * math.pi * s ** 3)
        if windowed:
            g = g * np.exp(-mu * s)
        out[i] = float(np.einsum("rp,r,p->", g * r[:, None], wr, wphi))
    return out


def point_source_rect(src, mu, p1, e1, e2, order=GL_ORDER):
    """The integral of |h| exp(-mu s) / (4 pi s^3) over the rectangle p1 + a e1 + b e2, 0 < a, b < 1
    (e1 and e2 orthogonal), for a point source at `src`: with mu = 0 the share of the source's
    directions whose ray meets the rectangle (which is what the reference's camera counts, see
    above), with mu > 0 the probability of getting there unabsorbed. Returns (p, (x, y)): the
    coordinates record_hit_2D bins a direct hit by, x = src.z + p1.x and y = src.y + p1.y: the
    pixel comes from the position of the source (the start of the leg), not from where the
    rectangle is met, so every direct hit lands in one pixel (camera_pixel)."""
    p1, e1, e2, src = (np.asarray(a, dtype=np.float64) for a in (p1, e1, e2, src))
    assert abs(float(e1 @ e2)) <= 1e-12 * math.sqrt(float(e1 @ e1) * float(e2 @ e2)), "not a rectangle"
    nrm = np.cross(e2, e1)
    area = math.sqrt(float(nrm @ nrm))
    h = abs(float((p1 - src) @ nrm)) / area
    x, w = _gl(order)
    pts = p1[None, None, :] + x[:, None, None] * e1[None, None, :] + x[None, :, None] * e2[None, None, :] - src
    s = np.sqrt((pts * pts).sum(axis=-1))
    g = h * np.exp(-mu * s) / (4.0 * math.pi * s ** 3)
    return float(np.einsum("ab,a,b->", g, w, w)) * area, (float(src[2] + p1[0]), float(src[1] + p1[1]))


def camera_pixel(xy, nbins, maxval):
    """The index in a camera's (nbins + 1)^2 block of the pixel record_hit_2D picks for the
    coordinates xy: int(x / w) + 1 with w = maxval / (nbins + 1), at most nbins + 1, and a value
    below 1 also goes to nbins + 1; x runs fastest."""
    nb = int(nbins) + 1
    w = 1.0 if nbins == 0 else float(maxval) / nb
    idx = []
    for c in xy:
        i = min(int(c / w) + 1, nb)   # int() truncates towards zero, as Fortran's does
        idx.append(nb if i < 1 else i)
    return (idx[0] - 1) + nb * (idx[1] - 1)


def fibre_chain(r, h, f, abs_at_pinhole=False):
    """check_hit_fibre's thin-lens chain for a ray that meets the front lens at radius r with the
    gradient r / h (a source on the axis, h in front of the lens). f: focalLength1, focalLength2,
    f1Aperture, f2Aperture, frontOffset, backOffset, frontToPinSep, pinToBackSep, pinAperture,
    acceptAngle (degrees), coreDiameter. Returns (accepted, |radius at the fibre|). The comparisons
    are signed as in the reference: a ray that has crossed the axis (negative radius) passes every
    aperture. abs_at_pinhole is a negative control."""
    f1, f2, ap1, ap2, _, back, to_pin, to_back, pin, accept, core = (float(v) for v in f)
    if r > ap1:
        return False, 0.0
    grad = r / h
    grad = -r / f1 + grad
    rad = r + grad * to_pin
    if (abs(rad) if abs_at_pinhole else rad) > pin:
        return False, 0.0
    rad = rad + grad * to_back
    if rad > ap2:
        return False, 0.0
    grad = -rad / f2 + grad
    rad = rad + grad * back
    if abs(math.atan(grad)) * 360.0 / (2.0 * math.pi) > accept or rad > core / 2.0:
        return False, abs(rad)
    return True, abs(rad)


def fibre_bins(src, mu, front, axis, f, nbins, abs_at_pinhole=False, order=GL_ORDER):
    """A fibre detector whose axis passes through the point source: `front` the centre of the front
    lens (pos + dir * frontOffset), `axis` its direction, pointing away from the source. Every
    step of the chain is linear in r, so radius-at-the-fibre = a r and each of the five limits
    (front aperture, pinhole, back aperture, acceptance angle, core radius) is c_k r <= l_k: with
    signed comparisons a negative c_k never binds, and the accepted set is 0 <= r <= r_max. The
    bin is nint(|a| r / w) + 1 with w = core / 2 / nbins, at most nbins + 1. Returns (probability
    per bin [nbins + 1], r_max, a, the edges in r)."""
    f = [float(v) for v in f]
    n, _, _ = _plane_frame(axis)
    rel = np.asarray(front, dtype=np.float64) - np.asarray(src, dtype=np.float64)
    h = float(rel @ n)
    assert h > 0.0 and math.sqrt(float(rel @ rel) - h * h if float(rel @ rel) > h * h else 0.0) < 1e-9, "source off the axis"
    f1, f2, ap1, ap2, _, back, to_pin, to_back, pin, accept, core = f
    g1 = 1.0 / h - 1.0 / f1                 # gradient after the front lens, per r
    c_pin = 1.0 + g1 * to_pin               # radius at the pinhole
    c_back = c_pin + g1 * to_back           # radius at the back lens
    g2 = g1 - c_back / f2                   # gradient after the back lens
    a = c_back + g2 * back                  # radius at the fibre
    limits = [ap1]
    for c, lim in ((abs(c_pin) if abs_at_pinhole else c_pin, pin), (c_back, ap2), (a, core / 2.0)):
        if c > 0.0:
            limits.append(lim / c)
    if g2 != 0.0:
        limits.append(math.tan(accept * 2.0 * math.pi / 360.0) / abs(g2))
    r_max = min(limits)
    nb = int(nbins) + 1
    w = 1.0 if nbins == 0 else core / 2.0 / nbins
    assert a != 0.0
    inner = np.concatenate([[0.0], (np.arange(nb - 1) + 0.5) * w / abs(a), [math.inf]]) if nb > 1 else np.array([0.0, math.inf])
    edges = np.minimum(inner, r_max)
    p = np.zeros(nb)
    live = np.flatnonzero(np.diff(edges) > 0.0)
    p[live] = point_source_disc_bins(src, mu, front, n, edges, order=order)[live]
    return p, r_max, a, edges


def legs_on_disc(legs, mu, centre, normal, edges, margin=1e-6):
    """A pencil beam's legs (beam_slab_legs) against one circle or annulus with bin edges `edges`:
    a leg that crosses the plane along the normal within its length lands at one radius. Returns
    (p per bin, landings): the bin of that radius gets q exp(-mu s) (mu inside the slab, 0
    outside), every other bin exactly 0; landings lists (bin, probability, landing point, radius).
    No landing radius may lie within `margin` of a bin edge, where rounding would pick the bin."""
    edges = np.asarray(edges, dtype=np.float64)
    n, _, _ = _plane_frame(normal)
    c = np.asarray(centre, dtype=np.float64)
    p = np.zeros(len(edges) - 1)
    landings = []
    for o, d, q, length, inside in legs:
        den = float(n @ d)
        if not den > 1e-6:
            continue
        t = float((c - o) @ n) / den
        assert abs(t) > margin and abs(t - length) > margin, "a leg ends within the margin of the plane"
        if not 0.0 < t <= length:
            continue
        at = o + t * d
        r = math.sqrt(float((at - c) @ (at - c)))
        assert np.min(np.abs(edges - r)) > margin, (r, edges)
        if not edges[0] < r <= edges[-1]:
            continue
        b = int(np.searchsorted(edges, r, side="left")) - 1
        pr = q * math.exp(-(mu if inside else 0.0) * t)
        p[b] += pr
        landings.append((b, pr, at, r))
    return p, landings


# ------------------------------------------------------------- scattering medium, layers ----
# A homogeneous medium (mus, mua, g; Henyey-Greenstein) that is effectively infinite. Project the
# absorption sites onto a fixed axis n: their density is mua times the scalar flux phi_0(x) of a
# 1-D plane-geometry transport problem. With mu the direction cosine to n, k the Fourier variable
# of x (phi(k) = int phi(x) exp(-i k x) dx) and phi_l the Legendre moments of the angular flux,
#   i k [(l + 1) phi_{l+1} + l phi_{l-1}] / (2 l + 1) + sigma_l phi_l = q_l(k),   l = 0 ... L,
#   sigma_l = mut - mus g^l   (sigma_0 = mua),
# a tridiagonal system whose elimination from l = L downwards is
#   D_L = sigma_L, D_{l-1} = sigma_{l-1} + k^2 c_l / D_l, c_l = l^2 / ((2 l - 1)(2 l + 1)),
#   u_L = q_L,     u_{l-1} = q_{l-1} - i k l / (2 l - 1) u_l / D_l,        phi_0 = u_0 / D_0:
# for q_l = delta_l0 the continued fraction 1 / (sigma_0 + k^2 c_1 / (sigma_1 + k^2 c_2 / ...)).
# 1 / (mut + i k mu) has Legendre moments up to l of a few k / mut, which sets the truncation L.
# The layer [x1, x2] (coordinates from the source) holds per photon
#   mua / pi Re int_0^inf phi_0(k) (exp(i k x2) - exp(i k x1)) / (i k) dk
# absorptions and 1 / mua times that as track length. The uncollided flux decays slowly in k and
# has a closed form in x: it is taken out of phi_0 and added back per layer. What is left decays
# as 1 / k or faster but matters up to k of 1e3 to 1e4 next to the source, so the k-integral is
# Gauss-Legendre panels up to SC_K1 mut and beyond that a Filon rule on geometrically spaced
# nodes: phi_c(k) / (i k) piecewise linear, integrated against exp(i k x) exactly.
SC_K1 = 6.0          # in units of mut: the end of the Gauss-Legendre panels
SC_KMAX = 5.0e2      # in units of mut: the end of the k-integral
SC_PANEL = 0.1       # in units of mut: one 16-point panel (x up to 100 / mut: 10 radians per panel)
SC_RATIO = 0.004     # the geometric nodes' spacing, relative to k
SC_L0, SC_LK = 64, 5.0   # L = SC_L0 + SC_LK k / mut


def exp_integral_2(x):
    """E2(x) = int_1^inf exp(-x t) / t^2 dt for x >= 0: exp(-x) - x E1(x), E1 by its power series
    up to x = 1 and by the continued fraction (modified Lentz) beyond."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    assert np.all(x >= 0.0)
    e1 = np.zeros_like(x)
    small = (x > 0.0) & (x <= 1.0)
    if small.any():
        xs = x[small]
        s, term = np.zeros_like(xs), np.ones_like(xs)
        for n in range(1, 40):
            term = term * (-xs) / n
            s -= term / n
        e1[small] = -0.5772156649015329 - np.log(xs) + s
    big = x > 1.0
    if big.any():
        xb = x[big]
        b = xb + 1.0
        c = np.full_like(xb, 1e300)
        d = 1.0 / b
        h = d.copy()
        for n in range(1, 200):
            an = -float(n * n)
            b = b + 2.0
            d = 1.0 / (an * d + b)
            c = b + an / c
            h = h * (c * d)
        e1[big] = h * np.exp(-xb)
    return np.exp(-x) - x * e1


def _moments(g, lmax):
    """The Legendre moments g_0 ... g_lmax of the scattering kernel: g^l for Henyey-Greenstein. A
    tuple (g, g_2) replaces the second moment (a negative control: the right mean cosine, the
    wrong shape)."""
    if isinstance(g, tuple):
        m = float(g[0]) ** np.arange(lmax + 1)
        m[2] = float(g[1])
        return m
    return float(g) ** np.arange(lmax + 1)


def _sigma(mus, mua, g, lmax):
    return (mus + mua) - mus * _moments(g, lmax)


def _legendre_at(mu0, lmax):
    p = np.empty(lmax + 1)
    p[0] = 1.0
    if lmax >= 1:
        p[1] = mu0
    for l in range(1, lmax):
        p[l + 1] = ((2 * l + 1) * mu0 * p[l] - l * p[l - 1]) / (l + 1)
    return p


def phi0_point(k, mus, mua, g, lmax):
    """phi_0(k) of the isotropic point source, q_l = delta_l0, as the continued fraction; k may be
    imaginary (k = i lam gives the moment generating function E[exp(lam x)] / mua). Returns
    (phi_0, the smallest denominator met: positive while lam lies below the first pole)."""
    k2 = np.asarray(k) ** 2
    sig = _sigma(mus, mua, g, lmax)
    d = np.full(k2.shape, sig[lmax], dtype=k2.dtype)
    dmin = np.full(k2.shape, np.inf)
    for l in range(lmax, 0, -1):
        d = sig[l - 1] + k2 * (l * l / ((2.0 * l - 1.0) * (2.0 * l + 1.0))) / d
        dmin = np.minimum(dmin, d.real)
    return 1.0 / d, dmin


def phi0_solve(ik, mus, mua, g, q, lmax):
    """phi_0 of the tridiagonal system above for the sources q[l] (an array [lmax + 1, len(ik)] or
    [lmax + 1, 1]); `ik` is i k, or a real -lam for the moment generating function. Returns
    (phi_0, the smallest real part of a denominator)."""
    ik = np.asarray(ik)
    sig = _sigma(mus, mua, g, lmax)
    k2 = -(ik * ik)
    d = np.full(ik.shape, sig[lmax], dtype=ik.dtype)
    u = np.broadcast_to(q[lmax], ik.shape).astype(ik.dtype)
    dmin = np.full(ik.shape, np.inf)
    for l in range(lmax, 0, -1):
        u = q[l - 1] - ik * (l / (2.0 * l - 1.0)) * u / d
        d = sig[l - 1] + k2 * (l * l / ((2.0 * l - 1.0) * (2.0 * l + 1.0))) / d
        dmin = np.minimum(dmin, d.real)
    return u / d, dmin


def _beam_q(ik, mus, mua, g, mu0, lmax):
    """The first-collision source of a pencil beam with direction cosine mu0 to the axis: collisions
    at x = mu0 s with density mus exp(-mut s), re-emitted with the Henyey-Greenstein kernel about
    the beam, whose azimuthal average about the axis is sum (2l+1)/(4 pi) g^l P_l(mu) P_l(mu0)."""
    gl = _moments(g, lmax) * _legendre_at(mu0, lmax)
    return mus * gl[:, None] / ((mus + mua) + np.asarray(ik)[None, :] * mu0)


def _collided(k, mus, mua, g, mu0, l0, lk):
    """phi_0 minus the uncollided flux at the real k (ascending), L chosen per octave of k."""
    mut = mus + mua
    out = np.empty(len(k), dtype=np.complex128)
    start = 0
    top = max(2.0 * mut, float(k[0]))
    while start < len(k):
        stop = int(np.searchsorted(k, top, side="right"))
        if stop > start:
            kk = k[start:stop]
            lmax = int(l0 + lk * kk[-1] / mut)
            if mu0 is None:
                out[start:stop] = phi0_point(kk, mus, mua, g, lmax)[0] - np.arctan(kk / mut) / kk
            else:
                ik = 1j * kk
                out[start:stop] = phi0_solve(ik, mus, mua, g, _beam_q(ik, mus, mua, g, mu0, lmax), lmax)[0]
        start, top = stop, 2.0 * top
    return out


def _collided_cumulative(x, mus, mua, g, mu0, kmax, panel, ratio, l0, lk):
    """C(x) = mua / pi Re int_0^K phi_c(k) (exp(i k x) - 1) / (i k) dk for every x: the collided
    absorptions per photon between the source's plane and x (signed)."""
    mut = mus + mua
    x = np.asarray(x, dtype=np.float64)
    # Gauss-Legendre panels: the integrand is smooth, (exp(i k x) - 1) / (i k) -> x at k = 0
    k1 = SC_K1 * mut
    pe = np.linspace(0.0, k1, int(round(SC_K1 / panel)) + 1)
    gx, gw = _gl(16)
    k = (pe[:-1, None] + np.diff(pe)[:, None] * gx[None, :]).ravel()
    w = (np.diff(pe)[:, None] * gw[None, :]).ravel()
    f = _collided(k, mus, mua, g, mu0, l0, lk)
    low = ((f * w / (1j * k))[None, :] * np.expm1(1j * k[None, :] * x[:, None])).sum(axis=1)
    # Filon: F = phi_c / (i k) linear between the nodes, against exp(i k x) and against 1
    kn = k1 * (1.0 + ratio) ** np.arange(int(math.ceil(math.log(kmax / SC_K1) / math.log1p(ratio))) + 1)
    fn = _collided(kn, mus, mua, g, mu0, l0, lk) / (1j * kn)
    h = np.diff(kn)
    theta = x[:, None] * h[None, :]
    ok = np.abs(theta) > 1e-2
    th = np.where(ok, theta, 1.0)
    e = np.exp(1j * th)
    a_big = (e - 1.0) / (1j * th)
    b_big = e / (1j * th) + (e - 1.0) / (th * th)
    ts = np.where(ok, 0.0, theta)
    a_small = 1.0 + 0.5j * ts - ts ** 2 / 6.0 - 1j * ts ** 3 / 24.0 + ts ** 4 / 120.0
    b_small = 0.5 + 1j * ts / 3.0 - ts ** 2 / 8.0 - 1j * ts ** 3 / 30.0 + ts ** 4 / 144.0
    a, b = np.where(ok, a_big, a_small), np.where(ok, b_big, b_small)
    seg = np.exp(1j * x[:, None] * kn[None, :-1]) * h[None, :] * (fn[None, :-1] * a + np.diff(fn)[None, :] * b)
    high = seg.sum(axis=1) - (h * 0.5 * (fn[:-1] + fn[1:])).sum()
    return mua / math.pi * (low + high).real


def _uncollided_point(x, mus, mua):
    """The uncollided absorptions of the point source between the source's plane and x: the
    marginal of mua exp(-mut r) / (4 pi r^2) integrated, mua (1 - E2(mut |x|)) / (2 mut), odd."""
    mut = mus + mua
    x = np.asarray(x, dtype=np.float64)
    return np.sign(x) * mua * (1.0 - exp_integral_2(mut * np.abs(x))) / (2.0 * mut)


def _uncollided_beam(x, mus, mua, mu0):
    """The same for the beam: absorptions with density mua exp(-mut s) at x = mu0 s."""
    mut = mus + mua
    x = np.asarray(x, dtype=np.float64)
    if mu0 == 0.0:
        return np.where(x > 0.0, 0.5, np.where(x < 0.0, -0.5, 0.0)) * mua / mut   # all in the source's plane
    s = np.maximum(x / mu0, 0.0)
    return math.copysign(1.0, mu0) * mua / mut * -np.expm1(-mut * s)


def scatter_cumulative(x, mus, mua, g, mu0=None, kmax=SC_KMAX, panel=SC_PANEL, ratio=SC_RATIO, l0=SC_L0, lk=SC_LK):
    """Absorptions per photon between the source's plane and the plane at x (signed, any array of
    coordinates along the axis measured from the source) in a homogeneous infinite medium, for an
    isotropic point source (mu0 None) or a pencil beam with direction cosine mu0 to the axis. For
    mu0 = 0 the uncollided absorptions all lie in the source's plane: no x may be 0 then."""
    mus, mua = float(mus), float(mua)
    assert mua > 0.0 and mus >= 0.0 and abs(g[0] if isinstance(g, tuple) else g) < 1.0
    x = np.asarray(x, dtype=np.float64)
    if mu0 is None:
        unc = _uncollided_point(x, mus, mua)
    else:
        assert mu0 != 0.0 or np.min(np.abs(x)) > 0.0, "the beam lies in a layer's face"
        unc = _uncollided_beam(x, mus, mua, float(mu0))
    if mus == 0.0:
        return unc
    return unc + _collided_cumulative(x, mus, mua, g, mu0, kmax * (mus + mua), panel, ratio, l0, lk)


def scatter_layers(edges, source, mus, mua, g, mu0=None, **kw):
    """Absorptions per photon in every layer between successive `edges` (ascending, absolute
    coordinates along the axis) for a source at the coordinate `source` (scatter_cumulative). The
    expected track length per photon in a layer is this over mua."""
    return np.diff(scatter_cumulative(np.asarray(edges, dtype=np.float64) - float(source), mus, mua, g, mu0, **kw))


def scatter_layers_point(edges, source, mus, mua, g, **kw):
    return scatter_layers(edges, source, mus, mua, g, None, **kw)


def scatter_layers_beam(edges, source, mus, mua, g, mu0, **kw):
    return scatter_layers(edges, source, mus, mua, g, float(mu0), **kw)


def scatter_mgf(lam, mus, mua, g, mu0=None, lmax=200):
    """E[exp(lam x)] of the absorption site's coordinate x along the axis (from the source), for
    real lam below the first pole: mua phi_0(k = i lam), the uncollided part included. Returns
    (value, valid): valid is False where a denominator of the elimination is not positive."""
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    mut = mus + mua
    if mu0 is None:
        v, dmin = phi0_point(1j * lam, mus, mua, g, lmax)
        v = v.real
    else:
        ok = mut - lam * mu0 > 0.0
        ik = np.where(ok, -lam, 0.0)
        v, dmin = phi0_solve(ik, mus, mua, g, _beam_q(ik, mus, mua, g, mu0, lmax), lmax)
        v = v + 1.0 / (mut + ik * mu0)
        dmin = np.where(ok, dmin, -1.0)
    return mua * v, dmin > 0.0


def scatter_tail_bound(w, mus, mua, g, mu0=None, side=1):
    """A rigorous bound on P(absorption site beyond x = side * w), w > 0 from the source:
    Chernoff's min over lam of E[exp(side lam x)] exp(-lam w), on a grid of lam below the pole."""
    lam = np.linspace(0.0, mus + mua, 4001)[1:]
    m, valid = scatter_mgf(side * lam, mus, mua, g, mu0)
    valid = np.cumprod(valid).astype(bool) & (m > 0.0)
    assert valid.any()
    return float(np.min(m[valid] * np.exp(-lam[valid] * w)))


def scatter_moments(mus, mua, g):
    """(<x^2> of the point source's absorption sites along any axis, <z> of a beam's along itself,
    mean and variance of the scatterings per photon)."""
    mut = mus + mua
    a = mus / mut
    return (2.0 / (3.0 * mut * mut * (1.0 - a) * (1.0 - a * g)), 1.0 / (mut * (1.0 - a * g)),
            a / (1.0 - a), a / (1.0 - a) ** 2)
