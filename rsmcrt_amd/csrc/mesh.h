// mesh.h — mesh_kernel: transport through closed triangle surfaces ("Mesh media").
//
// The scene is a set of closed, consistently oriented triangle surfaces, each triangle naming the
// medium on either side, a table of media (an ordinary TopProps array, K.props / K.n_top) and the
// ambient medium. There is no SDF: a leg of a flight is one ray cast through the threaded
// hierarchy (meshcast.h), which says how far the next surface is; the leg is then walked voxel by
// voxel with the SDF kernels' crossing (dda_step) for the path-length deposits, and ends in an
// interaction or on a triangle, where the triangle's own normal decides reflection or refraction.
//
// Scheduling is voxel_kernel's: a persistent grid, wave-aggregated fetch from C->queue, one lane
// per photon refilled as photons end, per-block counters flushed at the end, deposits through the
// plan's regime. A trip has two stages: every walking lane walks one piece, then the events
// (emission, flight start, cast, surface, interaction, completion) run together once enough
// lanes wait for one. The cast is an event, so its divergent traversal runs with as many lanes as
// wait for one.
//
// Media and faces are staged in LDS. Nodes and triangles are read from device memory, in the event
// stage. That stage follows the walk stage in the same trip of the same wave, so the cast's loads
// can still wait on the counters of that trip's deposit stores and atomics (voxel.h); how much they
// do has not been measured.
//
// Included by kinst.hip's part 7 only (after kernels.h), so no other kernel sees this file.
#pragma once
#include "kernels.h"

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

// LDS-resident per-lane counters and per-photon fields (transport.h LCTR / LU index them)
struct MeshShared {
  uint32_t ctr[LC_N][256];
  uint32_t u[LU_N][256];
};

// start_segment (transport.h) for a kernel whose LDS is not a LaneShared: the same text, the
// caller counts LC_UPD.
template <int GM>
__device__ __forceinline__ void mesh_start_segment(const KParams& K, Lane& L, V3 p, double dlen) {
  V3 old = v3(p.x + K.xmax, p.y + K.ymax, p.z + K.zmax);
  int32_t ci = cell_of<GM>(old.x, K.nx, K.xmax, K.inv2x, K.fex), cj = cell_of<GM>(old.y, K.ny, K.ymax, K.inv2y, K.fey),
          ck = cell_of<GM>(old.z, K.nz, K.zmax, K.inv2z, K.fez);
  L.xcell = ci; L.ycell = cj; L.zcell = ck;
  L.seg = false;
  if (!(K.flags & SMCRT_FLAG_PATHLENGTH)) {  // inttau2.f90:446-463
    old.x = old.x + L.dir.x * dlen;
    old.y = old.y + L.dir.y * dlen;
    old.z = old.z + L.dir.z * dlen;
    ci = cell_of<GM>(old.x, K.nx, K.xmax, K.inv2x, K.fex); cj = cell_of<GM>(old.y, K.ny, K.ymax, K.inv2y, K.fey);
    ck = cell_of<GM>(old.z, K.nz, K.zmax, K.inv2z, K.fez);
    if (ci == -1 || cj == -1 || ck == -1) L.tflag = true;
    L.xcell = ci; L.ycell = cj; L.zcell = ck;
    return;
  }
  L.old = old;
  if (ci == -1 || cj == -1 || ck == -1) { L.tflag = true; return; }
  L.sd = 0.0; L.slen = dlen; L.dda_it = 0;
  L.seg = true;
}

template <int GM, bool XSRC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SMCRT_WAVES_PER_EU_MESH))) void mesh_kernel(
    KParams K, const smcrt_sdf_node* __restrict__ nodes, const ProgOp* __restrict__ prog,
    const smcrt_detector* __restrict__ dets, const int64_t* __restrict__ det_off, const KCold* __restrict__ C) {
  (void)nodes; (void)prog;  // (transport_kernel's argument list; a mesh scene has no SDF)
  __shared__ MeshShared shm;
  MeshShared* sh = &shm;
  const bool survival = (K.flags & SMCRT_FLAG_SURVIVAL_BIAS) != 0;
  const bool pathlen = (K.flags & SMCRT_FLAG_PATHLENGTH) != 0;
  const int lane_id = threadIdx.x & 63;

  // [media | faces] | deposit words, as voxel_kernel lays them out
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

  const MeshNode* __restrict__ const bvh = C->mesh_nodes;
  const MeshTri* __restrict__ const tris = C->mesh_tris;
  const MeshFace* __restrict__ const faces = C->mesh_faces;
  const uint32_t n_bvh = C->mesh_n_nodes;
  // Lane fields under other names: L.d the leg's length dlen, L.Ls the triangle the leg ends on (or
  // MESH_NONE), L.old_layer the triangle to skip, L.hop the legs of the flight, L.pend "the medium
  // comes from this cast" (the first cast after an emission).
  Lane L;
  L.st = MS_FETCH; L.pend = false; L.seg = false; L.fault = false; L.tflag = false;
  L.pos = L.dir = L.ssp = L.old = v3(0.0, 0.0, 0.0);
  L.weight = 1.0; L.tau = L.taurun = L.d = L.minabs = 0.0;
  L.xcell = L.ycell = L.zcell = L.layer = L.new_layer = 0;
  L.old_layer = L.Ls = MESH_NONE;
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
  uint32_t visits = 0;              // nodes this lane's casts visited
  uint64_t chunk_base = 0;          // wave-uniform photon chunk
  uint32_t chunk_left = 0;

  for (;; ++w_iters) {
    // ---- photon fetch (wave-aggregated work queue; transport_kernel's) --------------------
    {
      uint64_t need = __ballot(L.st == MS_FETCH);
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
            if (L.st == MS_FETCH) L.st = MS_IDLE;
            break;
          }
        }
        const uint32_t n = __popcll(need);
        const uint32_t take = n < chunk_left ? n : chunk_left;
        const uint64_t rank = __popcll(need & ((1ull << lane_id) - 1ull));
        if (L.st == MS_FETCH && rank < take) {
          L.rng.init(C->first_photon + chunk_base + rank);
          L.st = MS_EMIT;
        }
        chunk_base += take;
        chunk_left -= take;
        need = __ballot(L.st == MS_FETCH);
      }
      if (__ballot(L.st != MS_IDLE) == 0) break;
    }

    // ---- walk: one piece (one iteration of update_grids) per walking lane ------------------
    if (__ballot(L.st == MS_WALK)) {  // wave-uniform, so deposit records can be wave-compacted
      const bool walk = L.st == MS_WALK;
      bool dep = false;
      uint32_t vox = 0;
      double val = 0.0;
      if (walk) dda_step<GM>(K, L, L.dir, xf, yf, zf, dep, vox, val, L.weight);
      w_dep += __popcll(__ballot(dep));
      if (binned) {
        if (K.bucket_tiles) emit_bucketed(K, C, WB, dep, vox, val, overflow, bstate);
        else emit_deposits(K, C, W, dep, vox, val, overflow, whist);
      } else if (dep) {
        double* const jm = C->jmean;
        if (jm) atomic_add_nr(jm + vox, val);
      }
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
          if (sep < __builtin_huge_val())  // (a leg to infinity without a walk has no end to measure to)
            LCTR(LC_HITS) += record_hits(K, C->det_bins, dets, det_off, L.pos, L.dir, sep, L.layer, L.weight);
        }
        L.pos = end;
        if (L.tflag) L.st = MS_DONE;  // escaped
        else if (L.Ls != MESH_NONE) L.st = MS_SURFACE;
        else { L.tau = 0.0; L.st = MS_INTERACT; }
      }
    }

    // ---- events: rare and expensive, run together (transport_kernel's P7 rule) -------------
    {
      const bool ev = L.st == MS_EMIT || L.st == MS_FLIGHT || L.st == MS_CAST || L.st == MS_SURFACE ||
                      L.st == MS_INTERACT || L.st == MS_DONE;
      const uint64_t evm = __ballot(ev);
      const uint64_t busy = __ballot(L.st != MS_IDLE && L.st != MS_FETCH);
      const uint32_t nev = __popcll(evm);
      if (nev && (nev >= SMCRT_EVENT_LANES || evm == busy)) {
        if (L.st == MS_INTERACT) {  // voxel_kernel's block; kernelsMod.f90:1958-1975 / 2036-2065
          if (++LU(LU_INTER) > (uint32_t)MAX_INTERACTIONS) {
            L.fault = true; L.st = MS_DONE;
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
            L.st = (sc && !L.fault) ? MS_FLIGHT : MS_DONE;
          }
        }
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
              const double s2 = 2.0 * dot(N, L.dir);
              L.dir = L.dir - smul(s2, N);
              LCTR(LC_REFL)++;
              if (++LU(LU_BOUNCES) > 1000) {  // a lossless trap never ends otherwise (voxel.h)
                LCTR(LC_BABORT)++;
                L.fault = true; L.st = MS_DONE;
              }
            } else {  // refract, surfaces.f90:57-84
              const double eta = n1 / n2;
              V3 Nt = N;
              double c1 = dot(Nt, L.dir);
              if (c1 < 0.0) c1 = -c1;
              else Nt = smul(-1.0, N);
              const double c2 = sqrt(1.0 - (eta * eta) * (1.0 - c1 * c1));
              L.dir = smul(eta, L.dir) + smul(eta * c1 - c2, Nt);
              L.layer = m2 + 1;
            }
          }
        }
        if (L.st == MS_EMIT) {  // kernelsMod.f90:1937-1945
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
          L.layer = 0;  // (no medium until the first cast)
          if (L.fault) {
            L.st = MS_DONE;
          } else {
            if (K.flags & SMCRT_FLAG_RENDER_SOURCE) add_cell(K, C->emission, L, 1.0);
            L.pend = true;
            L.st = MS_FLIGHT;
          }
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
            LCTR(LC_UPD)++;
            mesh_start_segment<GM>(K, L, L.pos, L.d);
            L.st = L.seg ? MS_WALK : MS_LEGEND;
          }
        }
        if (L.st == MS_DONE) {  // photon finished
          if (L.fault) { LU(LU_STATUS) = 3; LCTR(LC_FAULTS)++; }
          else if (LU(LU_STATUS) == 0) { LU(LU_STATUS) = 2; LCTR(LC_ESCAPED)++; }
          LCTR(LC_PHOTONS)++;
          LCTR(LC_DRAWS) += L.rng.draws;
          smcrt_photon_record* const records = C->records;
          if ((K.flags & SMCRT_FLAG_RECORD_PHOTONS) && records) {
            const uint64_t pid = ((uint64_t)L.rng.pid_hi << 32) | L.rng.pid_lo;
            smcrt_photon_record* r = records + (pid - C->first_photon);
            r->pos[0] = L.pos.x; r->pos[1] = L.pos.y; r->pos[2] = L.pos.z;
            r->dir[0] = L.dir.x; r->dir[1] = L.dir.y; r->dir[2] = L.dir.z;
            r->weight = L.weight;
            r->cell[0] = L.xcell; r->cell[1] = L.ycell; r->cell[2] = L.zcell;
            r->layer = L.layer;
            r->nscatt = LU(LU_NSCATT);
            r->bounces = LU(LU_BOUNCES);
            r->draws = L.rng.draws;
            r->status = LU(LU_STATUS);
          }
          L.tflag = false; L.fault = false; L.pend = false; L.seg = false;
          L.st = MS_FETCH;
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
  // the casts' node visits: the far march's running total, which a mesh scene has no other use for
  // (smcrt_kernel_times::far_steps)
  {
    const uint32_t s = wave_sum_u32(visits);
    unsigned long long* const fs = C->far_steps;
    if (lane_id == 0 && s && fs) atomicAdd(fs, (unsigned long long)s);
  }
  double* const nscatt = C->nscatt;
  if (nscatt) {
    const uint32_t s = wave_sum_u32(LCTR(LC_SCATTERS));
    if (lane_id == 0 && s) atomic_add_nr(nscatt, (double)s);
  }
}

}  // namespace smcrt
