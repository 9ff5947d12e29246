// voxel.h — voxel_kernel: transport through a label volume ("Voxel media").
//
// The scene is the grid, one uint8 label per voxel (x fastest, the order of jmean: lin() indexes
// both) and a table of media (an ordinary TopProps array, K.props / K.n_top). There is no SDF: a
// photon walks voxel by voxel with the exact DDA crossing of the SDF kernels (dda_step_r with
// sd = 0 and slen = tau_left / kappa), looks up the label of each voxel it enters and meets an
// interface wherever the refractive index changes, with the normal of the crossed voxel wall.
//
// Scheduling is the photon-lane scaffold of lanekit.h, which transport_kernel uses too: a persistent
// grid, wave-aggregated fetch from C->queue, one lane per photon refilled as photons end, per-block
// counters flushed at the end, deposits through the plan's regime (buckets, sorted records or fp64
// atomics). A lane does one piece or one event per trip; the rare events (emission, flight start,
// Fresnel decision, interaction, completion) run together once enough lanes wait for one. What is
// here is the kernel's own: the walk stage, the Fresnel wall and the flight start.
//
// PPL: the partial path lengths (ppath.h, SMCRT_FLAG_PARTIAL_PATHS), done as HIST is done in
// transport_kernel: every line of it is under `if constexpr (PPL)` and the lane's state is an
// empty type otherwise, so the other instantiations are what they were without it.
//
// Included by kinst.hip's parts 4 and 8 only (after kernels.h), so no other kernel sees this file.
#pragma once
#include "kernels.h"
#include "ppath.h"

namespace smcrt {

#ifndef SMCRT_WAVES_PER_EU_VOXEL
#define SMCRT_WAVES_PER_EU_VOXEL 4  // no SDF evaluator, no nested-node frame: <= 128 VGPRs
#endif

enum : uint32_t {
  VS_IDLE = 0,  // no photon and the queue is empty
  VS_FETCH,     // needs a photon index
  VS_EMIT,      // emission (+ re-emission while the start cell is outside the grid)
  VS_FLIGHT,    // flight start: tau_left = -log(ran), bounces = 0
  VS_WALK,      // one piece per trip
  VS_FRESNEL,   // entered a voxel of another refractive index: one draw, reflect or refract
  VS_INTERACT,  // the piece ended inside the voxel: scatter or absorb
  VS_DONE,      // photon finished: tallies, record, next photon
};

template <int GM, bool XSRC, bool PPL = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SMCRT_WAVES_PER_EU_VOXEL))) void voxel_kernel(
    KParams K, const smcrt_sdf_node* __restrict__ nodes, const ProgOp* __restrict__ prog,
    const smcrt_detector* __restrict__ dets, const int64_t* __restrict__ det_off, const KCold* __restrict__ C) {
  (void)nodes; (void)prog;  // (transport_kernel's argument list; a voxel scene has no SDF)
  __shared__ LaneCounters shm;
  LaneCounters* sh = &shm;
  const bool survival = (K.flags & SMCRT_FLAG_SURVIVAL_BIAS) != 0;
  const bool pathlen = (K.flags & SMCRT_FLAG_PATHLENGTH) != 0;
  const int lane_id = threadIdx.x & 63;

  // [media | faces] | deposit words. Everything a lane looks up per crossing but the label is in
  // LDS: a vector load would wait for the wave's outstanding record stores and atomics.
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

  const uint8_t* __restrict__ const labels = C->vox_labels;
  Lane L;
  lane_reset(L, VS_FETCH);
  uint32_t w_iters = 0;     // wave total (a scalar register)
  uint64_t chunk_base = 0;  // wave-uniform photon chunk
  uint32_t chunk_left = 0;

  for (;; ++w_iters) {
    if (!fetch_photons<VS_FETCH, VS_IDLE>(C, lane_id, L, chunk_base, chunk_left, [&](uint64_t g) {
          L.rng.init(g);
          L.st = VS_EMIT;
        }))
      break;

    // ---- walk: one piece (one iteration of update_grids) per walking lane ------------------
    bool leg_end = false;  // the leg's last piece was walked: detectors
    if (__ballot(L.st == VS_WALK)) {  // wave-uniform, so deposit records can be wave-compacted
      const bool walk = L.st == VS_WALK;
      bool dep = false;
      uint32_t vox = 0;
      double val = 0.0, kap = 0.0;
      DdaPieceAxis pc;
      const V3 stood = L.old;
      const int32_t ci = L.xcell, cj = L.ycell, ck = L.zcell;  // the voxel being left
      if (walk) {
        kap = props[L.layer - 1].kappa;
        L.sd = 0.0;
        L.slen = kap > 0.0 ? L.tau / kap : __builtin_huge_val();
        L.seg = true;
        dda_step<GM>(K, L, L.dir, xf, yf, zf, dep, vox, val, L.weight, &pc);
      }
      // the label of the voxel entered: issued before the piece's deposit is filed
      const bool entered = walk && pc.wall && !L.tflag;
      uint32_t lab = 0;
      if (entered) lab = labels[lin(K, L.xcell, L.ycell, L.zcell)];
      if constexpr (PPL) {  // the piece the tally sees, unrounded, in the medium of the voxel being left
        if (walk && dep) ppl_add(P, sh_dyn, L.layer, pc.dc);
      }
      dep = dep && pathlen;
      D.file(K, C, dep, vox, val);
      if (walk) {
        if (L.fault) {  // an error stop of the crossing, or the MAX_DDA_ITERS cap: it ends where it stood
          L.old = stood;
          L.st = VS_DONE;
        } else if (!pc.wall) {  // ended inside the voxel: update_pos(.false.) advances all three
          // (dda_step_r leaves the position of a segment's last piece undefined: transport_kernel
          // never reads it)
          L.old = v3(stood.x + L.dir.x * pc.dc, stood.y + L.dir.y * pc.dc, stood.z + L.dir.z * pc.dc);
          L.tau = 0.0;
          leg_end = true;
          L.st = VS_INTERACT;
        } else {
          L.tau = dmax(L.tau - kap * pc.dc, 0.0);
          if (L.tflag) {  // left the grid: escaped
            leg_end = true;
            L.st = VS_DONE;
          } else if ((int32_t)lab + 1 != L.layer) {
            if (props[lab].n == props[L.layer - 1].n) {
              L.layer = (int32_t)lab + 1;  // index-matched: the leg continues
            } else {
              L.new_layer = (int32_t)lab + 1;
              L.Ls = pc.axis;  // the crossed axis and the cell index it had before the crossing
              L.old_layer = pc.axis == 0 ? ci : (pc.axis == 1 ? cj : ck);
              leg_end = true;
              L.st = VS_FRESNEL;
            }
          }
        }
      }
    }

    // ---- detectors: once per leg, from its start to where the photon stands ------------------
    if (K.n_dets && leg_end) {
      const V3 start = v3(L.ssp.x - K.xmax, L.ssp.y - K.ymax, L.ssp.z - K.zmax);
      const V3 end = v3(L.old.x - K.xmax, L.old.y - K.ymax, L.old.z - K.zmax);
      if constexpr (PPL) {  // every hit files the lengths up to where the photon stands
        const double sep = pointsep(end, start);
        auto file = [&](int32_t di, const smcrt_detector*) {
          ppl_file(C, P, sh_dyn, ((uint64_t)L.rng.pid_hi << 32) | L.rng.pid_lo, di, 0u, start, L.dir, sep, L.layer, L.weight,
                   LU(LU_NSCATT));
        };
        LCTR(LC_HITS) += record_hits(K, C->det_bins, dets, det_off, start, L.dir, sep, L.layer, L.weight, nullptr, file);
      } else {
        LCTR(LC_HITS) += record_hits(K, C->det_bins, dets, det_off, start, L.dir, pointsep(end, start), L.layer, L.weight);
      }
    }

    // ---- events: rare and expensive, run together (events_due, lanekit.h) --------------------
    {
      const bool ev = L.st == VS_EMIT || L.st == VS_FLIGHT || L.st == VS_FRESNEL || L.st == VS_INTERACT || L.st == VS_DONE;
      if (events_due(ev, L.st != VS_IDLE && L.st != VS_FETCH)) {
        if (L.st == VS_INTERACT) L.st = interact_event(K, C, L, sh, props, survival) ? VS_FLIGHT : VS_DONE;
        if (L.st == VS_FRESNEL) {
          // The crossed axis is the one update_pos snapped (inttau2.f90:538-582: the first of x, y, z
          // with ldir set), handed out by the crossing; its wall is the face of the voxel left that
          // the photon moved towards.
          const double delta = 1e-8;
          const bool ax = L.Ls == 0, ay = L.Ls == 1, az = L.Ls == 2;
          const double da = ax ? L.dir.x : (ay ? L.dir.y : L.dir.z);
          const bool pos_a = da > 0.0;
          {
            // the outward normal of the voxel being left (reflect_refract does not depend on its sign)
            const double sn = pos_a ? 1.0 : -1.0;
            const V3 N = v3(ax ? sn : 0.0, ay ? sn : 0.0, az ? sn : 0.0);
            const double n1 = props[L.layer - 1].n, n2 = props[L.new_layer - 1].n;
            LCTR(LC_FRES)++;
            const double Rf = fresnel(L.dir, N, n1, n2);
            if (L.rng.next(K.key0, K.key1) <= Rf) {  // reflect, surfaces.f90:42-55
              L.dir = reflect_dir(L.dir, N);
              // back on the side it came from: the wall minus the signed delta, the crossed axis'
              // cell index as it was
              const int32_t pc_a = L.old_layer, k = pos_a ? pc_a : pc_a - 1;
              const double back = pos_a ? -delta : delta;
              if (ax) { L.old.x = face<GM>(xf, k, K.fex) + back; L.xcell = pc_a; }
              if (ay) { L.old.y = face<GM>(yf, k, K.fey) + back; L.ycell = pc_a; }
              if (az) { L.old.z = face<GM>(zf, k, K.fez) + back; L.zcell = pc_a; }
              if (!count_bounce(L, sh)) L.st = VS_DONE;
            } else {  // refract, surfaces.f90:57-84
              L.dir = refract_dir(L.dir, N, n1, n2);
              L.layer = L.new_layer;
            }
            if (L.st == VS_FRESNEL) {  // the next leg of the same flight
              L.ssp = L.old;
              LCTR(LC_UPD)++;
              L.st = VS_WALK;
            }
          }
        }
        if (L.st == VS_EMIT) {
          const bool ok = emit_event<GM, XSRC>(K, C, L, sh);
          if constexpr (PPL) ppl_clear(P, sh_dyn);  // a new photon (a faulted emission files zeros)
          // the position is carried in corner coordinates from here on
          L.old = v3(L.pos.x + K.xmax, L.pos.y + K.ymax, L.pos.z + K.zmax);
          if (ok) L.layer = (int32_t)labels[lin(K, L.xcell, L.ycell, L.zcell)] + 1;
          L.st = ok ? VS_FLIGHT : VS_DONE;  // (a faulted emission has no start cell, so no medium)
        }
        if (L.st == VS_FLIGHT) {
          LCTR(LC_TAU)++;
          L.tau = -det_log(L.rng.next(K.key0, K.key1));
          LU(LU_BOUNCES) = 0;
          L.dda_it = 0;
          L.ssp = L.old;
          LCTR(LC_UPD)++;
          L.st = VS_WALK;
        }
        if (L.st == VS_DONE) {  // photon finished
          close_photon(L, sh);
          write_record(K, C, L, sh, v3(L.old.x - K.xmax, L.old.y - K.ymax, L.old.z - K.zmax));
          if constexpr (PPL) {  // the range trigger: the final lengths of a photon of the tracked range
            const uint64_t pid = ((uint64_t)L.rng.pid_hi << 32) | L.rng.pid_lo;
            if (pid - C->range_first < C->range_count)
              ppl_file(C, P, sh_dyn, pid, -1, LU(LU_STATUS), v3(L.old.x - K.xmax, L.old.y - K.ymax, L.old.z - K.zmax), L.dir, 0.0,
                       L.layer, L.weight, LU(LU_NSCATT));
          }
          L.tflag = false; L.fault = false;
          L.st = VS_FETCH;
        }
      }
    }
  }

  D.close(K, C);
  flush_counters(C, sh, lane_id, D.w_dep, w_iters);
}

}  // namespace smcrt
