// mesh.h — mesh_kernel: transport through closed triangle surfaces ("Mesh media").
//
// The scene is a set of closed, consistently oriented triangle surfaces, each triangle naming the
// medium on either side, a table of media (an ordinary TopProps array, K.props / K.n_top) and the
// ambient medium. There is no SDF: a leg of a flight is one ray cast through the threaded
// hierarchy (meshcast.h), which says how far the next surface is; the leg is then walked voxel by
// voxel with the SDF kernels' crossing (dda_step) for the path-length deposits, and ends in an
// interaction or on a triangle, where the triangle's own normal decides reflection or refraction.
//
// Scheduling is the photon-lane scaffold of lanekit.h, as in voxel_kernel: a persistent grid,
// wave-aggregated fetch from C->queue, one lane per photon refilled as photons end, per-block
// counters flushed at the end, deposits through the plan's regime. A trip has two stages: every
// walking lane walks one piece, then the events (emission, flight start, cast, surface,
// interaction, completion) run together once enough lanes wait for one. The cast is an event, so
// its divergent traversal runs with as many lanes as wait for one. What is here is the kernel's own:
// the walk stage, the end of a leg, the cast and the surface.
//
// Media and faces are staged in LDS. Nodes and triangles are read from device memory, in the event
// stage. That stage follows the walk stage in the same trip of the same wave, so the cast's loads
// can still wait on the counters of that trip's deposit stores and atomics (voxel.h); how much they
// do has not been measured.
//
// PPL: the partial path lengths (ppath.h, SMCRT_FLAG_PARTIAL_PATHS), as in voxel_kernel: every
// line of it is under `if constexpr (PPL)` and the lane's state is an empty type otherwise, so the
// other instantiations are what they were without it.
//
// Included by kinst.hip's parts 7 and 9 only (after kernels.h), so no other kernel sees this file.
#pragma once
#include "kernels.h"
#include "ppath.h"

namespace smcrt {

#ifndef SMCRT_WAVES_PER_EU_MESH
#define SMCRT_WAVES_PER_EU_MESH 4  // no SDF evaluator, no per-lane stack: <= 128 VGPRs
#endif

enum : uint32_t {
  MS_IDLE = 0,  // no photon and the queue is empty
  MS_FETCH,     // needs a photon index
  MS_EMIT,      // emission (+ re-emission while the start cell is outside the grid)
  MS_FLIGHT,    // flight start: tau_left = -log(ran), bounces = 0, skip = none
  MS_CAST,      // a leg opens: one cast, dlen = min(s_max, t_hit), start_segment
  MS_WALK,      // one piece per trip
  MS_LEGEND,    // the leg is walked (or was jumped): detectors, the new position
  MS_SURFACE,   // stands on a triangle: medium bookkeeping, reflect or refract
  MS_INTERACT,  // the leg ended inside the medium: scatter or absorb
  MS_DONE,      // photon finished: tallies, record, next photon
};

template <int GM, bool XSRC, bool PPL = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SMCRT_WAVES_PER_EU_MESH))) void mesh_kernel(
    KParams K, const smcrt_sdf_node* __restrict__ nodes, const ProgOp* __restrict__ prog,
    const smcrt_detector* __restrict__ dets, const int64_t* __restrict__ det_off, const KCold* __restrict__ C) {
  (void)nodes; (void)prog;  // (transport_kernel's argument list; a mesh scene has no SDF)
  __shared__ LaneCounters shm;
  LaneCounters* sh = &shm;
  const bool survival = (K.flags & SMCRT_FLAG_SURVIVAL_BIAS) != 0;
  const bool pathlen = (K.flags & SMCRT_FLAG_PATHLENGTH) != 0;
  const int lane_id = threadIdx.x & 63;

  // [media | faces] | deposit words, as voxel_kernel lays them out
  extern __shared__ double sh_dyn[];
  const StagedMedia M = stage_media_faces(K, sh_dyn);
  const TopProps* const props = M.props;
  const double *const xf = M.xf, *const yf = M.yf, *const zf = M.zf;
  DepositState D;
  D.init(K, C, sh_dyn + M.doubles);
  zero_counters(sh);
  // PPL: this photon's length in every medium, in LDS after the deposit words (ppath.h). An empty
  // type otherwise.
  [[maybe_unused]] std::conditional_t<PPL, PplLane, NoPplLane> P;
  if constexpr (PPL) {
    ppl_init(C, P);
    ppl_clear(P, sh_dyn);
  }
  __syncthreads();

  const MeshNode* __restrict__ const bvh = C->mesh_nodes;
  const MeshTri* __restrict__ const tris = C->mesh_tris;
  const MeshFace* __restrict__ const faces = C->mesh_faces;
  const uint32_t n_bvh = C->mesh_n_nodes;
  // Lane fields under other names: L.d the leg's length dlen, L.Ls the triangle the leg ends on (or
  // MESH_NONE), L.old_layer the triangle to skip, L.hop the legs of the flight, L.pend "the medium
  // comes from this cast" (the first cast after an emission).
  Lane L;
  lane_reset(L, MS_FETCH);
  L.old_layer = L.Ls = MESH_NONE;
  uint32_t w_iters = 0;     // wave total (a scalar register)
  uint32_t visits = 0;      // nodes this lane's casts visited
  uint64_t chunk_base = 0;  // wave-uniform photon chunk
  uint32_t chunk_left = 0;

  for (;; ++w_iters) {
    if (!fetch_photons<MS_FETCH, MS_IDLE>(C, lane_id, L, chunk_base, chunk_left, [&](uint64_t g) {
          L.rng.init(g);
          L.st = MS_EMIT;
        }))
      break;

    // ---- walk: one piece (one iteration of update_grids) per walking lane ------------------
    if (__ballot(L.st == MS_WALK)) {  // wave-uniform, so deposit records can be wave-compacted
      const bool walk = L.st == MS_WALK;
      bool dep = false;
      uint32_t vox = 0;
      double val = 0.0;
      if constexpr (PPL) {  // the piece the tally sees, unrounded, in the leg's medium
        DdaPiece pc;
        if (walk) dda_step<GM>(K, L, L.dir, xf, yf, zf, dep, vox, val, L.weight, &pc);
        if (walk && dep) ppl_add(P, sh_dyn, L.layer, pc.dc);
      } else {
        if (walk) dda_step<GM>(K, L, L.dir, xf, yf, zf, dep, vox, val, L.weight);
      }
      D.file(K, C, dep, vox, val);
      if (walk && !L.seg) L.st = MS_LEGEND;
    }

    // ---- the end of a leg: detectors from its start to where the photon stands, the new position
    if (L.st == MS_LEGEND) {
      // where it stands: start + dir * dlen, or, for a leg that left the grid on its walk, where
      // the walk stood
      if (L.fault) {  // an error stop of the crossing, or the MAX_DDA_ITERS cap: it ends at the leg's start
        L.st = MS_DONE;
      } else {
        V3 end = v3(L.pos.x + L.dir.x * L.d, L.pos.y + L.dir.y * L.d, L.pos.z + L.dir.z * L.d);
        if (L.tflag && pathlen) end = v3(L.old.x - K.xmax, L.old.y - K.ymax, L.old.z - K.zmax);
        if (K.n_dets) {
          const double sep = pointsep(end, L.pos);
          if (sep < __builtin_huge_val()) {  // (a leg to infinity without a walk has no end to measure to)
            if constexpr (PPL) {  // every hit files the lengths up to the end of the leg
              auto file = [&](int32_t di, const smcrt_detector*) {
                ppl_file(C, P, sh_dyn, ((uint64_t)L.rng.pid_hi << 32) | L.rng.pid_lo, di, 0u, L.pos, L.dir, sep, L.layer, L.weight,
                         LU(LU_NSCATT));
              };
              LCTR(LC_HITS) += record_hits(K, C->det_bins, dets, det_off, L.pos, L.dir, sep, L.layer, L.weight, nullptr, file);
            } else {
              LCTR(LC_HITS) += record_hits(K, C->det_bins, dets, det_off, L.pos, L.dir, sep, L.layer, L.weight);
            }
          }
        }
        L.pos = end;
        if (L.tflag) L.st = MS_DONE;  // escaped
        else if (L.Ls != MESH_NONE) L.st = MS_SURFACE;
        else { L.tau = 0.0; L.st = MS_INTERACT; }
      }
    }

    // ---- events: rare and expensive, run together (events_due, lanekit.h) --------------------
    {
      const bool ev = L.st == MS_EMIT || L.st == MS_FLIGHT || L.st == MS_CAST || L.st == MS_SURFACE ||
                      L.st == MS_INTERACT || L.st == MS_DONE;
      if (events_due(ev, L.st != MS_IDLE && L.st != MS_FETCH)) {
        if (L.st == MS_INTERACT) L.st = interact_event(K, C, L, sh, props, survival) ? MS_FLIGHT : MS_DONE;
        if (L.st == MS_SURFACE) {
          const int32_t f = L.Ls;
          const MeshFace* const F = faces + f;
          const V3 N = v3(F->N[0], F->N[1], F->N[2]);
          const int32_t m = L.layer - 1;
          const int32_t out = (int32_t)F->outside, ins = (int32_t)F->inside;
          L.tau = dmax(L.tau - props[m].kappa * L.d, 0.0);
          const bool entering = dot(L.dir, N) < 0.0;
          const int32_t expect = entering ? out : ins, m2 = entering ? ins : out;
          L.old_layer = f;  // the next cast skips the triangle it starts on
          if (m != expect) {  // a leaky or intersecting mesh, or a ray through a crack
            L.fault = true; L.st = MS_DONE;
          } else if (props[m2].n == props[m].n) {
            L.layer = m2 + 1;  // index-matched: no draw
            L.st = MS_CAST;
          } else {
            const double n1 = props[m].n, n2 = props[m2].n;
            LCTR(LC_FRES)++;
            const double Rf = fresnel(L.dir, N, n1, n2);
            L.st = MS_CAST;
            if (L.rng.next(K.key0, K.key1) <= Rf) {  // reflect, surfaces.f90:42-55
              L.dir = reflect_dir(L.dir, N);
              if (!count_bounce(L, sh)) L.st = MS_DONE;
            } else {  // refract, surfaces.f90:57-84
              L.dir = refract_dir(L.dir, N, n1, n2);
              L.layer = m2 + 1;
            }
          }
        }
        if (L.st == MS_EMIT) {  // (no medium until the first cast)
          const bool ok = emit_event<GM, XSRC>(K, C, L, sh);
          if constexpr (PPL) ppl_clear(P, sh_dyn);  // a new photon (a faulted emission files zeros)
          if (ok) L.pend = true;
          L.st = ok ? MS_FLIGHT : MS_DONE;
        }
        if (L.st == MS_FLIGHT) {
          LCTR(LC_TAU)++;
          L.tau = -det_log(L.rng.next(K.key0, K.key1));
          LU(LU_BOUNCES) = 0;
          L.old_layer = MESH_NONE;
          L.hop = 0;
          L.st = MS_CAST;
        }
        if (L.st == MS_CAST) {
          if (++L.hop > (uint32_t)MAX_HOP_ITERS) {  // the cap on the legs of one flight
            L.fault = true; L.st = MS_DONE;
          } else {
            const double o[3] = {L.pos.x, L.pos.y, L.pos.z}, d[3] = {L.dir.x, L.dir.y, L.dir.z};
            const MeshHit h = mesh_cast(bvh, n_bvh, tris, o, d, L.old_layer);
            visits += h.visits;
            if (L.pend) {  // the medium of a fresh photon: the side of the first surface it faces
              L.pend = false;
              uint32_t m = C->mesh_ambient;
              if (h.tri != MESH_NONE) {
                const MeshFace* const F = faces + h.tri;
                m = (d[0] * F->N[0] + d[1] * F->N[1] + d[2] * F->N[2]) > 0.0 ? F->inside : F->outside;
              }
              L.layer = (int32_t)m + 1;
            }
            const double kap = props[L.layer - 1].kappa;
            const double s_max = kap > 0.0 ? L.tau / kap : __builtin_huge_val();
            const bool surf = h.tri != MESH_NONE && !(s_max < h.t);
            L.Ls = surf ? h.tri : MESH_NONE;
            L.d = surf ? h.t : s_max;
            // update_grids' entry for the leg. A leg that starts outside the grid leaves start_segment
            // before it has stored the start, which MS_LEGEND reads as the end of such a leg.
            L.seg = false;
            L.old = v3(L.pos.x + K.xmax, L.pos.y + K.ymax, L.pos.z + K.zmax);
            start_segment<GM>(K, L, sh, L.pos, L.d);
            L.st = L.seg ? MS_WALK : MS_LEGEND;
          }
        }
        if (L.st == MS_DONE) {  // photon finished
          close_photon(L, sh);
          write_record(K, C, L, sh, L.pos);
          if constexpr (PPL) {  // the range trigger: the final lengths of a photon of the tracked range
            const uint64_t pid = ((uint64_t)L.rng.pid_hi << 32) | L.rng.pid_lo;
            if (pid - C->range_first < C->range_count)
              ppl_file(C, P, sh_dyn, pid, -1, LU(LU_STATUS), L.pos, L.dir, 0.0, L.layer, L.weight, LU(LU_NSCATT));
          }
          L.tflag = false; L.fault = false; L.pend = false; L.seg = false;
          L.st = MS_FETCH;
        }
      }
    }
  }

  D.close(K, C);
  flush_counters(C, sh, lane_id, D.w_dep, w_iters);
  // the casts' node visits: the far march's running total, which a mesh scene has no other use for
  // (smcrt_kernel_times::far_steps)
  {
    const uint32_t s = wave_sum_u32(visits);
    unsigned long long* const fs = C->far_steps;
    if (lane_id == 0 && s && fs) atomicAdd(fs, (unsigned long long)s);
  }
}

}  // namespace smcrt
