// ppath.h — partial path lengths of voxel_kernel's and mesh_kernel's PPL instantiations
// (SMCRT_FLAG_PARTIAL_PATHS; include/smcrt.h "partial path lengths").
//
// A lane keeps len[m], the length its photon has walked in medium m since emission, in dynamic
// LDS after the kernel's deposit words, laid out len[m][threadIdx.x]: one lane owns one slot of
// each row, so an add is a plain read-modify-write without atomics, and the 64 lanes of a wave
// touch 64 consecutive doubles of a row (no bank conflict beyond the two passes a 64-bit access
// of a wave takes anyway). It is LDS and not device memory because the walk stage adds once per
// piece: a vector load there would wait for all of the wave's outstanding deposit stores and
// atomics (lanekit.h, voxel.h). It is not a register array because the number of media is a
// run-time number.
//
// A trigger (a detector hit, or the end of a photon of the tracked range) files a record: one
// returning atomic claims an arena slot, the n_media doubles are copied from LDS into it and a
// smcrt_ppath header is written. As in paths.h, the returning atomic waits for the wave's
// outstanding deposits; that is acceptable only because records are rare next to pieces and
// because only the PPL instantiations contain this code: a run without the flag never launches it.
//
// Every index is bounded before its store: medium < n_media (the rows the launch's LDS holds),
// slot < ppl_max. A wrong size drops a record or skips an add; it never writes outside.
#pragma once
#include "transport.h"

namespace smcrt {

constexpr uint32_t PPL_ROW = 256;  // lanes of a block: the stride between two media of one lane

// (The rows are addressed as an index into the kernel's dynamic LDS array, which every function
// here takes as `lds`: a pointer kept in the lane's state would become a generic one, and its
// accesses flat instructions instead of LDS ones.)
struct PplLane {
  uint32_t at = 0;       // index of len[0][threadIdx.x] in the dynamic LDS; medium m at lds[at + m * PPL_ROW]
  uint32_t n_media = 0;  // rows the launch's LDS holds
  uint32_t hit = 0;      // records filed since emission
};

struct NoPplLane {};  // what the instantiations without the accumulator hold in its place

// The rows start C->ppl_lds_off doubles into the kernel's dynamic LDS (the host sizes the launch's
// LDS from the same number, sceneplan.h launch_choice).
__device__ __forceinline__ void ppl_init(const KCold* __restrict__ C, PplLane& P) {
  P.at = C->ppl_lds_off + threadIdx.x;
  P.n_media = C->ppl_n_media;
  P.hit = 0;
}

// a new photon: emission clears the lengths and the record ordinal
__device__ __forceinline__ void ppl_clear(PplLane& P, double* lds) {
  for (uint32_t m = 0; m < P.n_media; ++m) lds[P.at + m * PPL_ROW] = 0.0;
  P.hit = 0;
}

// one walked piece of fp64 length dc in the medium of `layer` (1-based)
__device__ __forceinline__ void ppl_add(const PplLane& P, double* lds, int32_t layer, double dc) {
  const uint32_t m = (uint32_t)(layer - 1);
  if (m < P.n_media) lds[P.at + m * PPL_ROW] += dc;
}

// File the lane's lengths so far as one record.
__device__ __forceinline__ void ppl_file(const KCold* __restrict__ C, PplLane& P, const double* lds, uint64_t photon, int32_t detector,
                                         uint32_t status, V3 start, V3 dir, double point_sep, int32_t layer,
                                         double weight, uint32_t nscatt) {
  const uint32_t hit = P.hit++;
  unsigned long long* const ctl = C->ppl_ctl;
  if (!ctl) return;
  double* const arena = C->ppl_lengths;
  smcrt_ppath* const headers = C->ppl_headers;
  if (!arena || !headers) {
    atomicAdd(ctl + 1, 1ull);
    return;
  }
  const unsigned long long slot = atomicAdd(ctl + 0, 1ull);
  if (slot >= C->ppl_max) {  // the arena is full
    atomicAdd(ctl + 1, 1ull);
    return;
  }
  double* dst = arena + slot * (uint64_t)P.n_media;
  for (uint32_t m = 0; m < P.n_media; ++m) dst[m] = lds[P.at + m * PPL_ROW];
  smcrt_ppath* H = headers + slot;
  H->photon = photon;
  H->detector = detector;
  H->hit = hit;
  H->status = status;
  H->layer = layer;
  H->nscatt = nscatt;
  H->reserved = 0;
  H->start[0] = start.x; H->start[1] = start.y; H->start[2] = start.z;
  H->dir[0] = dir.x; H->dir[1] = dir.y; H->dir[2] = dir.z;
  H->point_sep = point_sep;
  H->weight = weight;
}

}  // namespace smcrt
