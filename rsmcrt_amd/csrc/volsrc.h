// volsrc.h — the rule of the volume source (include/smcrt.h "volume source"),
// written once for host and device, as screen.h and meshcast.h are.
//
// emit_ext (transport.h, case SMCRT_SRC_VOLUME) and smcrt_volume_sample / smcrt_volume_pick
// (smcrt.hip, host) compile this very text with -ffp-contract=off. The functions take the
// uniforms as arguments: the kernel draws them from the photon's Philox stream, the host export
// from the same stream restated on the host, so the same photon index gives the same voxel,
// position and direction everywhere.
//
// The table (volsrc_table, host): cdf[i] = cdf[i-1] + w[i], summed strictly left to right in fp64;
// total = cdf[nvox-1]; last = the largest i with cdf[i] > cdf[i-1] (cdf[-1] = 0).
//
// A voxel with cdf[i] == cdf[i-1] is never picked: the pick returns the smallest i with
// cdf[i] > x, and x >= 0 together with cdf[i] == cdf[i-1] makes i-1 (or an earlier index) satisfy
// the condition whenever i does. That covers a zero weight, and a weight that vanishes against
// its prefix in fp64 (1e-30 after 1e30).
#pragma once
#include <stdint.h>

#include "detmath.h"
#include "geometry.h"

namespace smcrt {

// Pick: x = u0 * total; the smallest i with cdf[i] > x by plain bisection; none: `last`. (A guard:
// for u0 <= 1 - 2^-53, the largest draw, the product lies at least half an ulp below total and
// does not round up to it.) Grids hold fewer than 2^32 voxels and lo <= hi <= nvox throughout, so
// lo + (hi - lo) / 2 in 32 bits is (lo + hi) / 2 without its overflow.
__host__ __device__ inline uint32_t volsrc_pick(const double* __restrict__ cdf, uint32_t nvox, uint32_t last, double total,
                                                double u0) {
  const double x = u0 * total;
  uint32_t lo = 0, hi = nvox;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cdf[mid] > x) hi = mid;
    else lo = mid + 1;
  }
  return lo < nvox ? lo : last;
}

// Place, one axis: q = face[c] + u * (face[c+1] - face[c]) in un-centred coordinates (c 0-based),
// pos = q - max, then the emitters' nudge off the grid's outer walls (nudge_faces, transport.h).
__host__ __device__ inline double volsrc_place(double f0, double f1, double u, double max) {
  const double q = f0 + u * (f1 - f0);
  double p = q - max;
  if (p == -max) p = p + 7.9e-7;
  else if (p == max) p = p - 7.9e-7;
  return p;
}

// Direction: the point source's text (photon.f90:311-359), isotropic.
__host__ __device__ inline V3 volsrc_dir(double u4, double u5) {
  const double phi = u4 * 6.283185307179586;
  double sinp, cosp;
  det_sincos(phi, &sinp, &cosp);
  const double cost = 2.0 * u5 - 1.0;
  const double sint = sqrt(1.0 - cost * cost);
  return v3(sint * cosp, sint * sinp, cost);
}

}  // namespace smcrt
