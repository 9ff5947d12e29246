// paths.h — photon path recording of transport_kernel's HIST instantiations
// (SMCRT_FLAG_TRACK_PATHS; the reference's history stack, detector_base.f90:37).
//
// A lane keeps the vertices of its photon so far in its own run of device memory
// (KCold::hist_scratch: hist_max_vertices x 4 doubles per lane, so a push is one full 32-byte
// sector however the lanes diverge). A trigger (a hit of a tracking detector, or the end of a
// photon of the tracked range) files the path: one returning atomic claims an arena slot, the
// vertices are copied into it and a smcrt_path header is written.
//
// Cost: the flush's returning atomic and the vector loads of its copy wait for all of the
// wave's outstanding deposit atomics (kernels.h: the notes at the LDS staging and at the photon
// fetch). That is acceptable only because flushes are rare next to deposits and because only
// the HIST instantiations contain them: a run without the flag never launches this code.
//
// Every index is bounded before its store: lane < hist_lanes, slot < path_max, vertex <
// hist_max_vertices. A wrong size drops or truncates a path; it never writes outside.
#pragma once
#include <type_traits>

#include "transport.h"

namespace smcrt {

struct PathLane {
  uint32_t n = 0;    // vertices pushed since emission (all of them, stored or not)
  uint32_t hit = 0;  // records filed since emission
};

struct NoPathLane {};  // what the instantiations without the recorder hold in its place

__device__ __forceinline__ uint64_t hist_lane_index() {
  return (uint64_t)blockIdx.x * (uint64_t)blockDim.x + (uint64_t)threadIdx.x;
}

// historyStack push of vec4(pos, step), kernelsMod.f90:1954,1959 / 2032,2037
__device__ __forceinline__ void hist_push(const KCold* __restrict__ C, PathLane& H, V3 pos, double step) {
  const uint64_t lane = hist_lane_index();
  double* const scratch = C->hist_scratch;
  const uint32_t maxv = C->hist_max_vertices;
  if (scratch && lane < C->hist_lanes && H.n < maxv) {
    double* v = scratch + (lane * (uint64_t)maxv + (uint64_t)H.n) * 4ull;
    v[0] = pos.x; v[1] = pos.y; v[2] = pos.z; v[3] = step;
  }
  ++H.n;
}

// File the lane's path so far as one record.
__device__ __forceinline__ void hist_flush(const KCold* __restrict__ C, PathLane& H, uint64_t photon, int32_t detector,
                                           uint32_t status, V3 start, V3 dir, double point_sep, int32_t layer,
                                           double weight) {
  const uint32_t hit = H.hit++;
  unsigned long long* const ctl = C->path_ctl;
  const uint64_t lane = hist_lane_index();
  const uint32_t maxv = C->hist_max_vertices;
  if (!ctl) return;
  if (!C->hist_scratch || !C->path_vertices || !C->path_headers || lane >= C->hist_lanes) {
    atomicAdd(ctl + 1, 1ull);
    return;
  }
  const unsigned long long slot = atomicAdd(ctl + 0, 1ull);
  if (slot >= C->path_max) {  // the arena is full
    atomicAdd(ctl + 1, 1ull);
    return;
  }
  const uint32_t stored = H.n < maxv ? H.n : maxv;
  if (stored < H.n) atomicAdd(ctl + 2, 1ull);
  const double* src = C->hist_scratch + lane * (uint64_t)maxv * 4ull;
  double* dst = C->path_vertices + slot * (uint64_t)maxv * 4ull;
  for (uint32_t i = 0; i < 4u * stored; ++i) dst[i] = src[i];
  smcrt_path* P = C->path_headers + slot;
  P->photon = photon;
  P->detector = detector;
  P->hit = hit;
  P->n_vertices = H.n;
  P->n_stored = stored;
  P->status = status;
  P->layer = layer;
  P->offset = (int64_t)slot;  // (the arena slot; smcrt_scene_read_paths replaces it)
  P->start[0] = start.x; P->start[1] = start.y; P->start[2] = start.z;
  P->dir[0] = dir.x; P->dir[1] = dir.y; P->dir[2] = dir.z;
  P->point_sep = point_sep;
  P->weight = weight;
}

}  // namespace smcrt
