// lanekit.h — what the one-lane-per-photon kernels share: transport_kernel (kernels.h), voxel_kernel
// (voxel.h) and mesh_kernel (mesh.h).
//
// All three are a persistent grid of waves that take photon indices from C->queue, keep one photon
// per lane, run the rare events together, file path-length deposits through the plan's regime and
// flush per-lane LDS counters at the end. That scaffold is here, once, as forceinline functions
// and small structs; a kernel passes its own state constants and keeps only its physics. `sh` is
// the kernel's LaneCounters (LCTR / LU index it). ws_kernel (ws.h) keeps its photons in scratch
// slots and has a scaffold of its own.
//
// transport_kernel's device code is held unchanged from before this header existed (its speed is
// tuned to the percent and its register allocation moves with the order in which locals become
// registers), so it calls only the pieces that leave it so: the counter and lane resets, the
// photon's close and record. It keeps its own text for the LDS staging, the fetch, the events_due
// rule, the deposit state (plain locals there) and the counter flush; its interaction and
// emission differ anyway. A change to one of those pieces here has to be made there too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "transport.h"
#include "deposit.h"

namespace smcrt {

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- LDS staging ---------------------------------------------------------------------------
// Media and faces at the head of dynamic LDS: per-lane (divergent) lookups go to LDS, never to
// vector memory, since a vector load would make the wave wait for all of its outstanding deposit
// stores and atomics. The caller's __syncthreads publishes the copy.
struct StagedMedia {
  const TopProps* props;
  const double *xf, *yf, *zf;
  int doubles;  // of sh_dyn used
};
__device__ __forceinline__ StagedMedia stage_media_faces(const KParams& K, double* sh_dyn) {
  const int np = 4 * K.n_top;
  const double* gp = (const double*)K.props;
  for (int i = threadIdx.x; i < np; i += blockDim.x) sh_dyn[i] = gp[i];
  const int nf = (K.nx + 1) + (K.ny + 1) + (K.nz + 2);
  double* sh_faces = sh_dyn + np;
  for (int i = threadIdx.x; i < nf; i += blockDim.x) sh_faces[i] = K.xface[i];  // faces are contiguous
  StagedMedia M;
  M.props = (const TopProps*)sh_dyn;
  M.xf = sh_faces;
  M.yf = sh_faces + (K.nx + 1);
  M.zf = M.yf + (K.ny + 1);
  M.doubles = np + nf;
  return M;
}

__device__ __forceinline__ void zero_counters(LaneCounters* sh) {
#pragma unroll
  for (int c = 0; c < LC_N; ++c) sh->ctr[c][threadIdx.x] = 0;
#pragma unroll
  for (int c = 0; c < LU_N; ++c) sh->u[c][threadIdx.x] = 0;
}

// ---- deposits ------------------------------------------------------------------------------
// A wave's deposit state in whichever regime the plan chose (deposit.h): the sorted path's log and
// per-wave tile histogram (hist_tiles words), the bucketed path's log and per-block word per tile
// (cur | next | fill: 2 * bucket_tiles words), or neither (fp64 atomics on jmean).
struct DepositState {
  RecLog W;
  BucketLog WB;
  uint32_t overflow;
  uint32_t w_dep;  // deposits of this wave (a scalar register)
  uint32_t* whist;
  unsigned long long* bstate;  // shared by the block's waves; sh_dyn is 8-byte aligned, so they are too
  bool binned;                 // (set only when jmean is tallied)

  // `words`: where the kernel's deposit words start in dynamic LDS
  __device__ __forceinline__ void init(const KParams& K, const KCold* __restrict__ C, double* words) {
    const uint32_t wave_words = K.bucket_tiles ? 0u : K.hist_tiles;
    whist = (uint32_t*)words + (threadIdx.x >> 6) * wave_words;
    bstate = (unsigned long long*)words;
    if (K.bucket_tiles) init_buckets(K, C, bstate);
    else
      for (uint32_t i = threadIdx.x; i < 4 * K.hist_tiles; i += blockDim.x) ((uint32_t*)words)[i] = 0;
    binned = K.rec_pool != nullptr;
    W.chunk = LOG_NONE; W.fill = 0;
    WB.next = WB.end = 0;
    overflow = 0;
    w_dep = 0;
  }
  // one deposit per lane with `dep` set; every lane of the wave calls it (records are wave-compacted)
  __device__ __forceinline__ void file(const KParams& K, const KCold* __restrict__ C, bool dep, uint32_t vox, double val) {
    w_dep += __popcll(__ballot(dep));
    if (binned) {
      if (K.bucket_tiles) emit_bucketed(K, C, WB, dep, vox, val, overflow, bstate);
      else emit_deposits(K, C, W, dep, vox, val, overflow, whist);
    } else if (dep) {
      double* const jm = C->jmean;
      if (jm) atomic_add_nr(jm + vox, val);
    }
  }
  __device__ __forceinline__ void close(const KParams& K, const KCold* __restrict__ C) {
    if (binned) {
      if (K.bucket_tiles) {
        close_buckets(K, C, WB, w_dep - overflow, overflow);
        __syncthreads();  // every wave of the block is done depositing
        close_block_buckets(K, C, bstate);
      } else {
        close_log(K, C, W, overflow, whist);
      }
    }
  }
};

// ---- lanes ---------------------------------------------------------------------------------
__device__ __forceinline__ void lane_reset(Lane& L, uint32_t st) {
  L.st = st; L.pend = false; L.seg = false; L.fault = false; L.tflag = false;
  L.pos = L.dir = L.ssp = L.old = v3(0.0, 0.0, 0.0);
  L.weight = 1.0; L.tau = L.taurun = L.d = L.minabs = 0.0;
  L.xcell = L.ycell = L.zcell = L.layer = L.old_layer = L.new_layer = L.Ls = 0;
  L.hop = L.loopc = L.dda_it = 0;
  L.sd = L.slen = 0.0;
  L.rng.init(0);
}

// Photon fetch: the wave-aggregated work queue. A wave takes FETCH_CHUNK photon indices per
// (returning) queue atomic and hands them to its lanes as they free up: a returning atomic waits
// for all of the wave's outstanding deposits, so it must be rare. A lane in FETCH that gets an
// index runs on_take(index), which seeds its generator and sets its emission state; once the queue
// is empty the others go to IDLE. chunk_base / chunk_left: the wave's chunk (wave-uniform).
// Returns false once no lane of the wave has a photon.
template <uint32_t FETCH, uint32_t IDLE, class F>
__device__ __forceinline__ bool fetch_photons(const KCold* __restrict__ C, int lane_id, Lane& L, uint64_t& chunk_base,
                                              uint32_t& chunk_left, F on_take) {
  uint64_t need = __ballot(L.st == FETCH);
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
        if (L.st == FETCH) L.st = IDLE;
        break;
      }
    }
    const uint32_t n = __popcll(need);
    const uint32_t take = n < chunk_left ? n : chunk_left;
    const uint64_t rank = __popcll(need & ((1ull << lane_id) - 1ull));
    if (L.st == FETCH && rank < take) on_take(C->first_photon + chunk_base + rank);
    chunk_base += take;
    chunk_left -= take;
    need = __ballot(L.st == FETCH);
  }
  return __ballot(L.st != IDLE) != 0;
}

// The events (emission, interaction, completion, ...) are the expensive, rare program points; a
// wave runs them together once enough lanes wait for one (or nothing else is left), instead of
// paying for them every trip. ev: this lane waits for one; busy: it has a photon.
__device__ __forceinline__ bool events_due(bool ev, bool busy) {
  const uint64_t evm = __ballot(ev);
  const uint64_t busym = __ballot(busy);
  const uint32_t nev = __popcll(evm);
  if (nev && (nev >= SMCRT_EVENT_LANES || evm == busym)) return true;  // (branches, not a combined flag)
  return false;
}

// ---- events of the kernels without an SDF (voxel.h, mesh.h) -----------------------------------
// Interaction, kernelsMod.f90:1958-1975 / 2036-2065: albedo roulette or survival bias, then the
// scatter. Returns whether the photon flies on; otherwise it was absorbed or faulted. (transport_kernel's
// differs: the photon's end travels in tflag there, and it has test_kernel's moments and the path recorder.)
__device__ __forceinline__ bool interact_event(const KParams& K, const KCold* __restrict__ C, Lane& L, LaneCounters* sh,
                                               const TopProps* props, bool survival) {
  if (++LU(LU_INTER) > (uint32_t)MAX_INTERACTIONS) {
    L.fault = true;
    return false;
  }
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
  return sc && !L.fault;
}

// Emission, kernelsMod.f90:1937-1945: a fresh photon, emitted again while its start cell is outside
// the grid, and the source image's deposit. It leaves the photon without a medium (L.layer = 0).
// Returns false when no emission landed in the grid (L.fault is set).
template <int GM, bool XSRC>
__device__ __forceinline__ bool emit_event(const KParams& K, const KCold* __restrict__ C, Lane& L, LaneCounters* sh) {
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
  L.layer = 0;
  if (L.fault) return false;
  if (K.flags & SMCRT_FLAG_RENDER_SOURCE) add_cell(K, C->emission, L, 1.0);
  return true;
}

// A Fresnel reflection counts towards the cap on the bounces of one flight: a lossless trap never
// ends otherwise (a deviation from the reference). Returns false when the cap is
// passed (L.fault is set).
__device__ __forceinline__ bool count_bounce(Lane& L, LaneCounters* sh) {
  LCTR(LC_REFL)++;
  if (++LU(LU_BOUNCES) > 1000) {
    LCTR(LC_BABORT)++;
    L.fault = true;
    return false;
  }
  return true;
}

// ---- completion ----------------------------------------------------------------------------
// A finished photon's status (3 fault, else what an event set, else 2 escaped) and its tallies.
__device__ __forceinline__ void close_photon(const Lane& L, LaneCounters* sh) {
  if (L.fault) { LU(LU_STATUS) = 3; LCTR(LC_FAULTS)++; }
  else if (LU(LU_STATUS) == 0) { LU(LU_STATUS) = 2; LCTR(LC_ESCAPED)++; }
  LCTR(LC_PHOTONS)++;
  LCTR(LC_DRAWS) += L.rng.draws;
}
// Its record, at its index in the launch; `pos` is where the kernel says it ended (centred).
__device__ __forceinline__ void write_record(const KParams& K, const KCold* __restrict__ C, const Lane& L,
                                             LaneCounters* sh, V3 pos) {
  smcrt_photon_record* const records = C->records;
  if ((K.flags & SMCRT_FLAG_RECORD_PHOTONS) && records) {
    const uint64_t pid = ((uint64_t)L.rng.pid_hi << 32) | L.rng.pid_lo;
    smcrt_photon_record* r = records + (pid - C->first_photon);
    r->pos[0] = pos.x; r->pos[1] = pos.y; r->pos[2] = pos.z;
    r->dir[0] = L.dir.x; r->dir[1] = L.dir.y; r->dir[2] = L.dir.z;
    r->weight = L.weight;
    r->cell[0] = L.xcell; r->cell[1] = L.ycell; r->cell[2] = L.zcell;
    r->layer = L.layer;
    r->nscatt = LU(LU_NSCATT);
    r->bounces = LU(LU_BOUNCES);
    r->draws = L.rng.draws;
    r->status = LU(LU_STATUS);
  }
}

// ---- the end of the launch -------------------------------------------------------------------
// Per-wave reduction of the lanes' counters into C->counters, and nscatt = number of scatters
// (kernelsMod.f90:1966), for the kernels without an SDF. w_*: the wave's own totals.
__device__ __forceinline__ void flush_counters(const KCold* __restrict__ C, LaneCounters* sh, int lane_id, uint32_t w_dep,
                                               uint32_t w_iters) {
  unsigned long long* const counters = C->counters;
  if (counters) {
    uint32_t c[SMCRT_NCOUNTERS];
    c[SMCRT_CTR_PHOTONS] = LCTR(LC_PHOTONS);
    c[SMCRT_CTR_EMIT_RETRIES] = LCTR(LC_RETRIES);
    c[SMCRT_CTR_SCATTERS] = LCTR(LC_SCATTERS);
    c[SMCRT_CTR_ABSORBED] = LCTR(LC_ABSORBED);
    c[SMCRT_CTR_SDF_EVALS] = 0u;  // (these kernels have no SDF)
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
