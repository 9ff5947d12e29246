// invoxel.h — does a deposit segment (update_grids, inttau2.f90:401-441) end inside the voxel it
// starts in? Plain C++: compiled for the device (ws.h) and by a host compiler alone
// (tests/invoxel_probe.cpp).
//
// What the reference does with such a segment. wall_dist (:467-521) forms, for the start cell's
// face f_a towards which each axis moves,
//     d_a = RN(RN(f_a - old_a) / dir_a)   (dir_a != 0),     d_a = 100000   (dir_a == 0),
// (-999 for a NaN component) and dcell = min(d_x, d_y, d_z). With the running length d = 0 of
// a fresh segment, update_grids (:421-429) tests d + dcell > len: if so this crossing is the
// last, it deposits real(len - 0, sp) * weight into the start voxel, moves by len without
// snapping to a face and leaves the packet's cells alone. If moreover dcell >= 0 there is no
// error stop (:510-516), and the iteration guard counts one iteration. transport.h's
// dda_step_r computes the same dcell bit for bit.
//
// The test. With n_a = RN(f_a - old_a) (the reference's own numerator, the same subtraction),
// s_a = sign(dir_a) and m = 1 + 2^-41, invoxel_segment returns true only if
//     (G)  2^-400 <= len < 100000                      (false for NaN, infinities and len = 0),
// and for every axis either dir_a == 0 (+0 or -0), or
//     (A1) |dir_a| >= 2^-500                            (false for NaN),
//     (A2) s_a n_a > RN(RN(len |dir_a|) m).
// s_a n_a is exact (a sign flip). By (G) and (A1) p = RN(len |dir_a|) >= 2^-900 is a normal
// number (or +inf, for which (A2) is false), so p >= len |dir_a| (1 - 2^-53) and
// RN(p m) >= p m (1 - 2^-53). (A2) then gives, in real numbers,
//     n_a / dir_a = s_a n_a / |dir_a| > len m (1 - 2^-53)^2 > len (1 + 2^-42).
// len is normal, so its successor is at most len (1 + 2^-52) < len (1 + 2^-42); the real
// quotient exceeds 2^-400, so it rounds as a normal number (or to +inf), and rounding is
// monotone: d_a = RN(n_a / dir_a) >= succ(len) > len. An axis with dir_a == 0 has
// d_a = 100000 > len by (G). Hence the reference's three facts:
//     dcell = min d_a > len >= 0, so  dcell >= 0  (no error stop; no d_a is -999 either, a NaN
//     component fails (A1));  0 + dcell = dcell > len  (the first crossing is the last);  the
//     guard sees iteration 1.
// What comes out false: a NaN anywhere ((G), (A1), or the comparison (A2) itself), an infinite
// len, 0 < |dir_a| < 2^-500 (denormals included), and a numerator whose sign is against the
// direction (a start within an ulp outside its own cell, the error stop the walker must see):
// then s_a n_a <= 0 <= the right-hand side. False is always safe: the segment is walked as
// before.
//
// The margin. far.h's loop tests RN(n_a r_a) > RN(len (1 + 2^-40)) with r_a the refined
// reciprocal of dir_a (relative error below 2^-51), which needs n_a / dir_a >
// len (1 + 2^-40) (1 - 2^-50). (A2) accepts from len (1 + 2^-41) (1 + 2^-51) on, which is
// smaller: every segment far.h's form accepts (with len >= 2^-400) this form accepts too, and
// it costs no reciprocal.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMCRT_INVOXEL_HD __host__ __device__ inline
#else
#define SMCRT_INVOXEL_HD inline
#endif

namespace smcrt {

// One axis: start coordinate `o` (corner coordinates), direction component `dir`, the face `f`
// wall_dist measures to (the start cell's upper face for dir > 0, its lower face otherwise).
SMCRT_INVOXEL_HD bool invoxel_axis(double f, double o, double dir, double len) {
  if (dir == 0.0) return true;
  const double ad = dir < 0.0 ? -dir : dir;
  const double n = f - o;
  const double sn = dir < 0.0 ? -n : n;
  const double rhs = (len * ad) * (1.0 + 0x1.0p-41);
  return ad >= 0x1.0p-500 && sn > rhs;
}

// true: the segment from (ox, oy, oz) along (dx, dy, dz) over `len` provably makes exactly one
// deposit, real(len, sp) * weight into its start voxel, and changes neither cells nor flags.
SMCRT_INVOXEL_HD bool invoxel_segment(double ox, double oy, double oz, double dx, double dy, double dz, double len,
                                      double fx, double fy, double fz) {
  if (!(len >= 0x1.0p-400 && len < 100000.0)) return false;
  return invoxel_axis(fx, ox, dx, len) && invoxel_axis(fy, oy, dy, len) && invoxel_axis(fz, oz, dz, len);
}

}  // namespace smcrt
