// phasor.h — the complex phasor tally of transport_kernel's PHAS instantiations
// (SMCRT_FLAG_PHASOR; the reference's phase tracking: photon%phase / photon%fact, update_grids'
// `packet%phase = packet%phase + dcell`, inttau2.f90:425,432, and iarray's phasor(:,:,:), which
// the reference allocates, reduces and never accumulates into).
//
// A lane carries its photon's phase (a length: the emitter's start phase plus every voxel piece
// walked since) and wavenumber k (PhasLane, transport.h). Every piece of update_grids adds its
// fp64 length; a piece that ends on a voxel wall then adds weight * exp(i k phase) to the voxel
// it leaves. Pieces that end inside a voxel (where the sphere trace happened to stop) are not
// sampled, so the tally does not depend on the step pattern.
//
// Cost: one det_sincos_any and two non-returning fp64 atomics per wall crossing, next to the
// crossing's jmean deposit. Only the PHAS instantiations contain them: a run without the flag
// never launches this code.
//
// The voxel index is the deposit's (dda_step_r's dep_vox, inside the grid whenever `dep` is
// true); it is bounded against the grid once more before the two stores.
#pragma once
#include "transport.h"

namespace smcrt {

// One voxel piece of lane state P: `dep`, `vox` as dda_step_r handed them out, `pc` its DdaPiece.
__device__ __forceinline__ void phasor_piece(const KParams& K, const KCold* __restrict__ C, PhasLane& P,
                                             const DdaPiece& pc, bool dep, uint32_t vox, double weight) {
  if (!dep) return;
  P.phase = P.phase + pc.dc;
  if (!pc.wall) return;
  double* const g = C->phasor;
  const uint32_t nvox = (uint32_t)K.nx * (uint32_t)K.ny * (uint32_t)K.nz;  // (< 2^32: scene_create)
  if (!g || vox >= nvox) return;
  double sn, cs;
  det_sincos_any(P.k * P.phase, &sn, &cs);
  atomic_add_nr(g + 2ull * vox, weight * cs);
  atomic_add_nr(g + 2ull * vox + 1ull, weight * sn);
}

}  // namespace smcrt
