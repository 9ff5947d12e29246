// voxel.h — voxel_kernel: transport through a label volume ("Voxel media").
//
// The scene is the grid, one uint8 label per voxel (x fastest, the order of jmean: lin() indexes
// both) and a table of media (an ordinary TopProps array, K.props / K.n_top). There is no SDF: a
// photon walks voxel by voxel with the exact DDA crossing of the SDF kernels (dda_step_r with
// sd = 0 and slen = tau_left / kappa), looks up the label of each voxel it enters and meets an
// interface wherever the refractive index changes, with the normal of the crossed voxel wall.
//
// Scheduling is transport_kernel's: a persistent grid, wave-aggregated fetch from C->queue, one
// lane per photon refilled as photons end, per-block counters flushed at the end, deposits
// through the plan's regime (buckets, sorted records or fp64 atomics). A lane does one piece or
// one event per trip; the rare events (emission, flight start, Fresnel decision, interaction,
// completion) run together once enough lanes wait for one.
//
// Included by kinst.hip's part 4 only (after kernels.h), so no other kernel sees this file.
#pragma once
#include "kernels.h"

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

// LDS-resident per-lane counters and per-photon fields (transport.h LCTR / LU index them)
struct VoxShared {
  uint32_t ctr[LC_N][256];
  uint32_t u[LU_N][256];
};

template <int GM, bool XSRC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SMCRT_WAVES_PER_EU_VOXEL))) void voxel_kernel(
    KParams K, const smcrt_sdf_node* __restrict__ nodes, const ProgOp* __restrict__ prog,
    const smcrt_detector* __restrict__ dets, const int64_t* __restrict__ det_off, const KCold* __restrict__ C) {
  (void)nodes; (void)prog;  // (transport_kernel's argument list; a voxel scene has no SDF)
  __shared__ VoxShared shm;
  VoxShared* sh = &shm;
  const bool survival = (K.flags & SMCRT_FLAG_SURVIVAL_BIAS) != 0;
  const bool pathlen = (K.flags & SMCRT_FLAG_PATHLENGTH) != 0;
  const int lane_id = threadIdx.x & 63;

  // [media | faces] | deposit words. Everything a lane looks up per crossing but the label is in
  // LDS: a vector load would wait for the wave's outstanding record stores and atomics.
  extern __shared__ double sh_dyn[];
  const int np = 4 * K.n_top;
  const int nf = (K.nx + 1) + (K.ny + 1) + (K.nz + 2);
  {
    const double* gp = (const double*)K.props;
    for (int i = threadIdx.x; i < np; i += blockDim.x) sh_dyn[i] = gp[i];
    for (int i = threadIdx.x; i < nf; i += blockDim.x) sh_dyn[np + i] = K.xface[i];  // faces are contiguous
  }
  const TopProps* const props = (const TopProps*)sh_dyn;
  const double* const xf = sh_dyn + np;
  const double* const yf = xf + (K.nx + 1);
  const double* const zf = yf + (K.ny + 1);
  const int hist_off = np + nf;
  const uint32_t wave_words = K.bucket_tiles ? 0u : K.hist_tiles;
  uint32_t* const whist = (uint32_t*)(sh_dyn + hist_off) + (threadIdx.x >> 6) * wave_words;
  unsigned long long* const bstate = (unsigned long long*)(sh_dyn + hist_off);
  if (K.bucket_tiles) init_buckets(K, C, bstate);
  else
    for (uint32_t i = threadIdx.x; i < 4 * K.hist_tiles; i += blockDim.x) ((uint32_t*)(sh_dyn + hist_off))[i] = 0;
#pragma unroll
  for (int c = 0; c < LC_N; ++c) sh->ctr[c][threadIdx.x] = 0;
#pragma unroll
  for (int c = 0; c < LU_N; ++c) sh->u[c][threadIdx.x] = 0;
  __syncthreads();

  const uint8_t* __restrict__ const labels = C->vox_labels;
  Lane L;
  L.st = VS_FETCH; L.pend = false; L.seg = false; L.fault = false; L.tflag = false;
  L.pos = L.dir = L.ssp = L.old = v3(0.0, 0.0, 0.0);
  L.weight = 1.0; L.tau = L.taurun = L.d = L.minabs = 0.0;
  L.xcell = L.ycell = L.zcell = L.layer = L.old_layer = L.new_layer = L.Ls = 0;
  L.hop = L.loopc = L.dda_it = 0;
  L.sd = L.slen = 0.0;
  L.rng.init(0);
  const bool binned = K.rec_pool != nullptr;  // (set only when jmean is tallied)
  RecLog W;
  W.chunk = LOG_NONE; W.fill = 0;
  BucketLog WB;
  WB.next = WB.end = 0;
  uint32_t overflow = 0;
  uint32_t w_dep = 0, w_iters = 0;  // wave totals (scalar registers)
  uint64_t chunk_base = 0;          // wave-uniform photon chunk
  uint32_t chunk_left = 0;

  for (;; ++w_iters) {
    // ---- photon fetch (wave-aggregated work queue; transport_kernel's) --------------------
    {
      uint64_t need = __ballot(L.st == VS_FETCH);
      while (need) {
        if (chunk_left == 0) {
          unsigned long long base = 0;
          if (lane_id == 0) base = atomicAdd(C->queue, (unsigned long long)SMCRT_FETCH_CHUNK);
          chunk_base = __shfl(base, 0, 64);
          const uint64_t n_photons = C->n_photons;
          chunk_left = (chunk_base < n_photons)
                           ? (uint32_t)((n_photons - chunk_base) < SMCRT_FETCH_CHUNK ? (n_photons - chunk_base)
                                                                                       : SMCRT_FETCH_CHUNK)
                           : 0u;
          if (chunk_left == 0) {  // queue exhausted
            if (L.st == VS_FETCH) L.st = VS_IDLE;
            break;
          }
        }
        const uint32_t n = __popcll(need);
        const uint32_t take = n < chunk_left ? n : chunk_left;
        const uint64_t rank = __popcll(need & ((1ull << lane_id) - 1ull));
        if (L.st == VS_FETCH && rank < take) {
          L.rng.init(C->first_photon + chunk_base + rank);
          L.st = VS_EMIT;
        }
        chunk_base += take;
        chunk_left -= take;
        need = __ballot(L.st == VS_FETCH);
      }
      if (__ballot(L.st != VS_IDLE) == 0) break;
    }

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
      dep = dep && pathlen;
      w_dep += __popcll(__ballot(dep));
      if (binned) {
        if (K.bucket_tiles) emit_bucketed(K, C, WB, dep, vox, val, overflow, bstate);
        else emit_deposits(K, C, W, dep, vox, val, overflow, whist);
      } else if (dep) {
        double* const jm = C->jmean;
        if (jm) atomic_add_nr(jm + vox, val);
      }
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
      LCTR(LC_HITS) += record_hits(K, C->det_bins, dets, det_off, start, L.dir, pointsep(end, start), L.layer, L.weight);
    }

    // ---- events: rare and expensive, run together (transport_kernel's P7 rule) -------------
    {
      const bool ev = L.st == VS_EMIT || L.st == VS_FLIGHT || L.st == VS_FRESNEL || L.st == VS_INTERACT || L.st == VS_DONE;
      const uint64_t evm = __ballot(ev);
      const uint64_t busy = __ballot(L.st != VS_IDLE && L.st != VS_FETCH);
      const uint32_t nev = __popcll(evm);
      if (nev && (nev >= SMCRT_EVENT_LANES || evm == busy)) {
        if (L.st == VS_INTERACT) {  // kernelsMod.f90:1958-1975 / 2036-2065
          if (++LU(LU_INTER) > (uint32_t)MAX_INTERACTIONS) {
            L.fault = true; L.st = VS_DONE;
          } else {
            const double ran = L.rng.next(K.key0, K.key1);
            const TopProps pr = props[L.layer - 1];
            bool sc = false;
            if (survival) {
              const double w_abs = L.weight * (1.0 - pr.albedo);
              L.weight = L.weight - w_abs;
              add_cell(K, C->absorb, L, w_abs);
              sc = true;
              if (L.weight < 0.01) {
                if (ran < 0.1) L.weight = L.weight / 0.1;
                else { LU(LU_STATUS) = 1; LCTR(LC_ABSORBED)++; sc = false; }
              }
            } else if (ran < pr.albedo) {
              sc = true;
            } else {
              LU(LU_STATUS) = 1; LCTR(LC_ABSORBED)++;
              add_cell(K, C->absorb, L, 1.0);
            }
            if (sc) {
              scatter(K, L, pr.hgg);
              ++LU(LU_NSCATT);
              LCTR(LC_SCATTERS)++;
            }
            L.st = (sc && !L.fault) ? VS_FLIGHT : VS_DONE;
          }
        }
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
              const double s2 = 2.0 * dot(N, L.dir);
              L.dir = L.dir - smul(s2, N);
              // back on the side it came from: the wall minus the signed delta, the crossed axis'
              // cell index as it was
              const int32_t pc_a = L.old_layer, k = pos_a ? pc_a : pc_a - 1;
              const double back = pos_a ? -delta : delta;
              if (ax) { L.old.x = face<GM>(xf, k, K.fex) + back; L.xcell = pc_a; }
              if (ay) { L.old.y = face<GM>(yf, k, K.fey) + back; L.ycell = pc_a; }
              if (az) { L.old.z = face<GM>(zf, k, K.fez) + back; L.zcell = pc_a; }
              LCTR(LC_REFL)++;
              if (++LU(LU_BOUNCES) > 1000) {  // a lossless trap never ends otherwise (deviation)
                LCTR(LC_BABORT)++;
                L.fault = true; L.st = VS_DONE;
              }
            } else {  // refract, surfaces.f90:57-84
              const double eta = n1 / n2;
              V3 Nt = N;
              double c1 = dot(Nt, L.dir);
              if (c1 < 0.0) c1 = -c1;
              else Nt = smul(-1.0, N);
              const double c2 = sqrt(1.0 - (eta * eta) * (1.0 - c1 * c1));
              L.dir = smul(eta, L.dir) + smul(eta * c1 - c2, Nt);
              L.layer = L.new_layer;
            }
            if (L.st == VS_FRESNEL) {  // the next leg of the same flight
              L.ssp = L.old;
              LCTR(LC_UPD)++;
              L.st = VS_WALK;
            }
          }
        }
        if (L.st == VS_EMIT) {  // kernelsMod.f90:1937-1945
          L.fault = false; L.layer = 0;
          LU(LU_STATUS) = 0; LU(LU_NSCATT) = 0; LU(LU_INTER) = 0; LU(LU_BOUNCES) = 0;
          L.xcell = L.ycell = L.zcell = 0;
          emit<GM, XSRC>(K, C, L, 0u);
          int64_t tries = 0;
          while (cell_out(K, L)) {
            if (++tries > MAX_EMIT_TRIES) { L.fault = true; break; }
            LCTR(LC_RETRIES)++;
            emit<GM, XSRC>(K, C, L, 0u);
          }
          L.tflag = false;
          // the position is carried in corner coordinates from here on
          L.old = v3(L.pos.x + K.xmax, L.pos.y + K.ymax, L.pos.z + K.zmax);
          if (L.fault) {
            L.layer = 0;  // (no start cell, so no medium)
            L.st = VS_DONE;
          } else {
            if (K.flags & SMCRT_FLAG_RENDER_SOURCE) add_cell(K, C->emission, L, 1.0);
            L.layer = (int32_t)labels[lin(K, L.xcell, L.ycell, L.zcell)] + 1;
            L.st = VS_FLIGHT;
          }
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
          if (L.fault) { LU(LU_STATUS) = 3; LCTR(LC_FAULTS)++; }
          else if (LU(LU_STATUS) == 0) { LU(LU_STATUS) = 2; LCTR(LC_ESCAPED)++; }
          LCTR(LC_PHOTONS)++;
          LCTR(LC_DRAWS) += L.rng.draws;
          smcrt_photon_record* const records = C->records;
          if ((K.flags & SMCRT_FLAG_RECORD_PHOTONS) && records) {
            const uint64_t pid = ((uint64_t)L.rng.pid_hi << 32) | L.rng.pid_lo;
            smcrt_photon_record* r = records + (pid - C->first_photon);
            r->pos[0] = L.old.x - K.xmax; r->pos[1] = L.old.y - K.ymax; r->pos[2] = L.old.z - K.zmax;
            r->dir[0] = L.dir.x; r->dir[1] = L.dir.y; r->dir[2] = L.dir.z;
            r->weight = L.weight;
            r->cell[0] = L.xcell; r->cell[1] = L.ycell; r->cell[2] = L.zcell;
            r->layer = L.layer;
            r->nscatt = LU(LU_NSCATT);
            r->bounces = LU(LU_BOUNCES);
            r->draws = L.rng.draws;
            r->status = LU(LU_STATUS);
          }
          L.tflag = false; L.fault = false;
          L.st = VS_FETCH;
        }
      }
    }
  }

  if (binned) {
    if (K.bucket_tiles) {
      close_buckets(K, C, WB, w_dep - overflow, overflow);
      __syncthreads();  // every wave of the block is done depositing
      close_block_buckets(K, C, bstate);
    } else {
      close_log(K, C, W, overflow, whist);
    }
  }

  // ---- per-wave counter reduction ------------------------------------------------------
  unsigned long long* const counters = C->counters;
  if (counters) {
    uint32_t c[SMCRT_NCOUNTERS];
    c[SMCRT_CTR_PHOTONS] = LCTR(LC_PHOTONS);
    c[SMCRT_CTR_EMIT_RETRIES] = LCTR(LC_RETRIES);
    c[SMCRT_CTR_SCATTERS] = LCTR(LC_SCATTERS);
    c[SMCRT_CTR_ABSORBED] = LCTR(LC_ABSORBED);
    c[SMCRT_CTR_SDF_EVALS] = 0u;
    c[SMCRT_CTR_DEPOSITS] = lane_id == 0 ? w_dep : 0u;
    c[SMCRT_CTR_GRID_UPDATES] = LCTR(LC_UPD);
    c[SMCRT_CTR_TAUINT] = LCTR(LC_TAU);
    c[SMCRT_CTR_FRESNEL] = LCTR(LC_FRES);
    c[SMCRT_CTR_REFLECTIONS] = LCTR(LC_REFL);
    c[SMCRT_CTR_BOUNCE_ABORTS] = LCTR(LC_BABORT);
    c[SMCRT_CTR_FAULTS] = LCTR(LC_FAULTS);
    c[SMCRT_CTR_RNG_DRAWS] = LCTR(LC_DRAWS);
    c[SMCRT_CTR_DETECTOR_HITS] = LCTR(LC_HITS);
    c[SMCRT_CTR_ESCAPED] = LCTR(LC_ESCAPED);
    c[SMCRT_CTR_WAVE_ITERS] = lane_id == 0 ? w_iters : 0u;
#pragma unroll
    for (int i = 0; i < SMCRT_NCOUNTERS; ++i) {
      const uint32_t s = wave_sum_u32(c[i]);
      if (lane_id == 0 && s) atomicAdd(counters + i, (unsigned long long)s);
    }
  }
  double* const nscatt = C->nscatt;
  if (nscatt) {
    const uint32_t s = wave_sum_u32(LCTR(LC_SCATTERS));
    if (lane_id == 0 && s) atomic_add_nr(nscatt, (double)s);
  }
}

}  // namespace smcrt
