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
//
// Optical path length (SMCRT_PHASOR_OPTICAL_PATH, KCold::phasor_optical): a piece adds n * dc, n
// the refractive index of the layer the lane carries while the piece is walked (phas_index).
//
// Field screens (smcrt_scene_set_screens, KCold::screens): screen_hits runs at P5 of the kernel,
// next to record_hits, on the leg the detectors receive, with the hit rule of screen.h. The
// phase of a hit is taken forward from the leg's start point (the fourth row of the kernel's
// startp), so a leg that leaves the grid, where the pieces stop, still gives the right phase, and
// the value does not depend on where the sphere trace stopped. Cost per leg and screen: the
// rule's three dot products and three divisions; per hit one det_sincos_any and two atomics.
#pragma once
#include "transport.h"

namespace smcrt {

// What a PHAS instantiation reads from KCold once, wave-uniform: the screen count and the
// optical-path option guard their code at run time. (An empty type in the other instantiations.)
struct PhasWave {
  uint32_t n_scr = 0, optical = 0;
};
struct NoPhasWave {};

// With the optical-path option: the refractive index that multiplies the lengths of a lane in
// `layer` (1 for a lane that needs none, `want`; the layer is bounded once more before the load).
// The kernel asks only when the option is on, so without it a piece and its phase are untouched.
__device__ __forceinline__ double phas_index(const KParams& K, const TopProps* __restrict__ props, bool want,
                                             int32_t layer) {
  if (!want || layer < 1 || layer > K.n_top) return 1.0;
  return props[layer - 1].n;
}

// One voxel piece of lane state P: `dep`, `vox` as dda_step_r handed them out, `pc` its DdaPiece
// (its length already times the lane's index when the optical-path option is on).
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

// One leg (start, dir, sep) of a lane against the launch's screens: `phase0` the lane's phase at
// the leg's start, `n_leg` its phas_index, `k` its wavenumber. The screen table is wave-uniform.
// The pixel is bounded against the screen's size once more before the two stores.
__device__ __forceinline__ void screen_hits(const KCold* __restrict__ C, uint32_t n_scr, const V3 start, const V3 dir,
                                            double sep, double phase0, double n_leg, double k, double weight) {
  const ScreenDev* __restrict__ const S = C->screens;
  double* const f = C->screen_field;
  if (!S || !f) return;
  if (n_scr > (uint32_t)SCREEN_MAX) n_scr = (uint32_t)SCREEN_MAX;
  for (uint32_t i = 0; i < n_scr; ++i) {
    double t = 0.0;
    int32_t px = 0;
    if (!screen_hit(S[i], start, dir, sep, t, px)) continue;
    const int32_t nu = S[i].nu, nv = S[i].nv;
    if (nu < 1 || nv < 1 || nu > SCREEN_MAX_PIXELS || nv > SCREEN_MAX_PIXELS || px < 0 || px >= nu * nv) continue;
    double sn, cs;
    det_sincos_any(k * (phase0 + n_leg * t), &sn, &cs);
    double* const p = f + S[i].offset + 2ull * (uint64_t)px;
    atomic_add_nr(p, weight * cs);
    atomic_add_nr(p + 1, weight * sn);
  }
}

}  // namespace smcrt
