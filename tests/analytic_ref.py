"""Test infrastructure only: closed-form per-voxel expectations that need neither the engine nor
its CPU restatement. Plain numpy in float64; everything is passed in as numbers.

Grids are given by their three arrays of voxel faces (`faces(n, half)`), results have the shape
(nz, ny, nx) of rsmcrt_amd.tallies.Result.

  point_source_track   scene A: an isotropic point source in a homogeneous absorber
  point_source_escape  scene A: the probability of leaving the grid unabsorbed
  beam_slab            scene B: a pencil beam through an index-mismatched absorbing slab
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
    mua = mu > 0. The probability of absorption in V is mu * T(V)."""
    mu = float(mu)
    assert mu > 0.0
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
