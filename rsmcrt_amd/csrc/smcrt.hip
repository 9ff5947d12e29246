// smcrt.hip — host side of the transport kernels (kernels.h, instantiated by kinst.hip),
// the fold kernels (deposit.h) and the C ABI of include/smcrt.h.
//
// Replaces the body of run_MCRT (kernelsMod.f90:1790-1898): the
// OpenMP `parallel do` over photons becomes a persistent grid whose waves pull 64 photon
// indices at a time from a device work queue; the `!$omp atomic` tally updates
// (inttau2.f90:426,433; kernelsMod.f90:2198,2218; detector_base.f90:156,228) become
// no-return fp64 atomics into device-resident tallies; the nscatt `reduction(+:...)` and
// the debug counters are reduced across each wave and added once per wave.
//
// What a scene is and which kernels it gets is decided without a device in sceneplan.cpp
// (plan_scene, the SMCRT_* knob readers, the pool and launch rules). This file uploads the
// plan, owns the device state through the handles of devmem.h, and enqueues the launches:
// launch() sizes the batches, enqueue_transport and enqueue_fold put one of them on the streams.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#define SMCRT_FOLD_KERNELS  // deposit.h: the fold kernels are defined in this translation unit
#include "../../include/smcrt.h"
#include "scene_internal.h"
#include "transport.h"
#include "deposit.h"
#include "devmem.h"
#include "hosterr.h"
#include "hostrng.h"
#include "sceneplan.h"

using namespace smcrt;

#include "kernel_ptrs.h"


// The top-level SDF containing each point: maxloc(ds, mask=ds<0), 0 outside every SDF
// (kernelsMod.f90:589-595, 1027-1032: the escape function's launch-cell test). One lane per
// point; the SDF program is walked wave-uniformly as in the transport kernel.
__global__ __launch_bounds__(256) void classify_kernel(const smcrt_sdf_node* __restrict__ nodes,
                                                       const ProgOp* __restrict__ prog, int32_t n_prog,
                                                       const double* __restrict__ pts, int64_t n, int32_t* layer) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i - threadIdx.x < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = i < n ? i : n - 1;  // whole waves walk the program together
    const V3 q = v3(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]);
    const EvalOut r = eval_sdfs<true>(nodes, prog, n_prog, q, false, 0, 0);
    if (i < n) layer[i] = r.maxloc;
  }
}

// ------------------------------------------------------------------ host side ------
thread_local std::string smcrt::g_last_error;

namespace {

int fail(int code, const std::string& msg) { return set_error(code, msg); }

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(SMCRT_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_));         \
  } while (0)

template <class T>
int dalloc(DevBuf<T>& b, size_t n) {
  const hipError_t e = b.alloc(n ? n : 1);
  if (e == hipErrorOutOfMemory) return fail(SMCRT_ERR_OOM, "hipMalloc: out of memory");
  if (e != hipSuccess) return fail(SMCRT_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  return SMCRT_OK;
}

// dalloc, then copy the n elements from the host (`what` names the step in the error)
template <class T>
int upload(DevBuf<T>& b, const T* src, size_t n, const char* what) {
  if (const int st = dalloc(b, n)) return st;
  const hipError_t e = n ? hipMemcpy(b, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  return e == hipSuccess ? SMCRT_OK : fail(SMCRT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

// The plan (sceneplan.h: what the scene is and which kernels it gets) plus the device state
// that serves it. Every device resource is an owner of devmem.h: `delete` releases them all.
struct smcrt_scene : ScenePlan {
  int device = 0;
  DevBuf<smcrt_sdf_node> d_nodes;
  DevBuf<ProgOp> d_prog;
  DevBuf<double> d_ctab;  // the cooperative EVAL's primitive table (transport.h), or NULL
  unsigned long long far_reported = 0, fold_ticks_reported = 0, hazards_reported = 0;  // d_queue totals already reported
  int wall_khz = 100000, n_cus = 256;  // s_memrealtime's rate; the fold's time is reported per CU
  DevBuf<CullGrid> d_cull;  // exact SDF culling (cull.h): the grid, and its lists in one allocation
  DevBuf<unsigned char> d_cull_data;
  DevBuf<TopProps> d_props;
  DevBuf<uint8_t> d_labels;  // a voxel scene's labels (voxel.h), or NULL
  DevBuf<MeshNode> d_mesh_nodes;  // a mesh scene's hierarchy, triangles and faces (mesh.h), or NULL
  DevBuf<MeshTri> d_mesh_tris;
  DevBuf<MeshFace> d_mesh_faces;
  DevBuf<double> d_faces;
  DevBuf<smcrt_detector> d_dets;
  DevBuf<int64_t> d_det_off;
  DevBuf<unsigned long long> d_queue;  // QueueWord (sceneplan.h): work-queue heads, running totals, watchdog
  // SMCRT_FLAG_OVERLAP: launches rotate over n_slots internal streams (lstream), so the next
  // launches' blocks fill the CUs their predecessors' tails leave idle
  Stream lstream[MAX_SLOTS];
  Event lev[MAX_SLOTS];  // the last launch on lstream[i] is done
  Event ev_in;           // the caller's work before an overlapped call
  bool lpending[MAX_SLOTS] = {};
  int lturn = 0;
  DevBuf<KCold> d_cold;  // launch parameters: COLD_PER_STREAM ring slots per launch stream
  uint64_t cold_seq[N_QUEUES] = {};
  // tallies owned by the scene for the synchronous smcrt_run
  DevBuf<double> d_grids;  // jmean | absorb | emission
  DevBuf<double> d_small;  // det bins | nscatt | moments(24)
  DevBuf<unsigned long long> d_counters;
  DevBuf<smcrt_photon_record> d_records;
  size_t records_cap = 0;
  Stream stream;
  int grid_table[N_GRID_KEYS] = {};  // blocks_for: the persistent grid per LaunchChoice::grid_key(); 0: not asked for yet
  // ws_kernel's lane scratch (ws.h WX_*) for scenes with Fresnel interfaces or detectors: one
  // region per launch stream (queue index), lscratch_stride bytes apart
  DevBuf<char> d_lscratch;
  size_t lscratch_stride = 0;
  bool lean_ok = false;  // lean_candidate, and the lane scratch (if needed) could be allocated
  int64_t lean_launches = 0;  // since the last smcrt_scene_kernel_times
#ifdef SMCRT_DIAG
  DevBuf<unsigned long long> d_done;  // per-photon completion times of the last run (SMCRT_DIAG_DONE)
  uint64_t n_done = 0;
#endif
  // source spectrum tables of the last general-emitter run (srcplan.h), device copy
  std::vector<double> h_spec;
  DevBuf<double> d_spec;
  size_t spec_cap = 0;
  // record-log slots in use (2, or MAX_SLOTS when a slot's pool is small: ensure_pool), and as
  // many internal launch streams; a launch's fold frees its slot: the fold of launch k (on
  // fstream) reads its slot while launch k+1's transport kernel fills another
  int n_slots = 2;
  DevBuf<unsigned long long> d_pool[MAX_SLOTS];  // record log, cap records
  DevBuf<unsigned long long> d_sorted;  // tile-sorted records (folds are serial on fstream)
  // bucketed path: per slot the tile of each bucket id (bucket fills use d_chunk_fill, the
  // per-tile bucket counts d_bin_counts); shared by the serial folds: ids in tile order
  DevBuf<uint32_t> d_bucket_tile[MAX_SLOTS];
  DevBuf<uint2> d_order;  // {id, fill} per bucket in tile order (bk_place)
  DevBuf<uint32_t> d_chunk_fill[MAX_SLOTS];
  DevBuf<uint32_t> d_dep_ctl[MAX_SLOTS];  // [0] chunks taken [1] overflow [2] pieces [3] records
  DevBuf<uint32_t> d_tile_count;  // n_tiles
  DevBuf<uint32_t> d_tile_start;  // n_tiles
  DevBuf<uint32_t> d_bin_counts[MAX_SLOTS];  // [n_tiles][BIN_BLOCKS]
  Stream fstream;           // the deposit folds
  Event ev_t;               // a transport launch finished (fstream waits on it)
  Event ev_f[MAX_SLOTS];    // the fold of slot i finished
  bool f_pending[MAX_SLOTS] = {};
  int slot = 0, last_slot = -1;
  size_t scatter_lds = 0;
  DevBuf<Piece> d_pieces;
  uint64_t pool_chunks = 0, max_pieces = 0;
  double rpp_est = 1024.0;           // deposit records per photon, refined from past launches
  bool rpp_measured = false;
  PinnedBuf<uint32_t> h_ctl;         // pinned copies of dep_ctl, 8 words per slot ([4] = photons)
  Event ctl_ev[MAX_SLOTS];
  bool ctl_pending[MAX_SLOTS] = {};
  // smcrt_scene_kernel_times: event quads (before / after transport on the launch stream,
  // before / after the deposit fold on fstream) of the launches since the last harvest
  bool timing = false;
  std::vector<Event> tev;
  size_t tev_used = 0;
  double t_transport = 0.0, t_deposit = 0.0;
  int64_t t_launches = 0;
  // photon paths (smcrt_scene_set_path_tracking; paths.h): the lanes' vertex scratch, sized for
  // the largest grid of a tracking launch (a tracking run's launches are serial on s->stream),
  // the arena of path_cfg.max_paths slots with its headers, and the counters
  // [claimed, dropped, truncated]
  bool path_on = false;
  smcrt_path_config path_cfg{};
  DevBuf<double> d_hist_scratch, d_path_vertices;
  DevBuf<smcrt_path> d_path_headers;
  DevBuf<unsigned long long> d_path_ctl;
  uint64_t hist_lanes = 0;
  // partial path lengths (smcrt_scene_set_partial_paths; ppath.h): the arena of ppath_cfg.max_records
  // slots of n_top doubles with its headers, and the counters [claimed, dropped]
  bool ppath_on = false;
  smcrt_ppath_config ppath_cfg{};
  DevBuf<double> d_ppl_lengths;
  DevBuf<smcrt_ppath> d_ppl_headers;
  DevBuf<unsigned long long> d_ppl_ctl;
  // the phasor tally (smcrt_scene_set_phasor; phasor.h): the grid, 2 doubles per voxel
  bool phasor_on = false;
  smcrt_phasor_config phasor_cfg{};
  DevBuf<double> d_phasor;
  // field screens (smcrt_scene_set_screens; screen.h): the table and the field buffer, tallied by
  // phasor launches only; such a launch holds a fourth row of start-point LDS, hence grids of its own
  std::vector<ScreenDev> screens;
  int64_t screen_doubles = 0;
  DevBuf<ScreenDev> d_screens;
  DevBuf<double> d_screen_field;
  // the volume source (smcrt_scene_set_volume_source; volsrc.h): the running sums of the weights
  // and what the pick and smcrt_scene_volume_source_info read; d_vs_cdf null: no table
  DevBuf<double> d_vs_cdf;
  int64_t vs_last = 0, vs_positive = 0, vs_reachable = 0;
  double vs_total = 0.0;
  std::mutex mu;
};

constexpr size_t MAX_TIMED = 256;  // launches kept before the events are harvested
constexpr uint64_t COLD_PER_STREAM = 16;  // in-flight launches per stream before a KCold slot is reused
constexpr uint64_t COLD_SLOTS = COLD_PER_STREAM * N_QUEUES;  // a ring per launch stream
constexpr uint64_t CALIB_PHOTONS = 1ull << 18;  // first binned launch of a scene above this size

// Fold the recorded event triples into the sums (waits for them).
static hipError_t harvest_times(smcrt_scene* s) {
  for (size_t i = 0; i < s->tev_used; ++i) {
    const Event* e = &s->tev[4 * i];
    hipError_t err = hipEventSynchronize(e[1]);
    if (err == hipSuccess) err = hipEventSynchronize(e[3]);
    if (err != hipSuccess) return err;
    float a = 0.f, b = 0.f;
    if ((err = hipEventElapsedTime(&a, e[0], e[1])) != hipSuccess) return err;
    if ((err = hipEventElapsedTime(&b, e[2], e[3])) != hipSuccess) return err;
    s->t_transport += a; s->t_deposit += b; s->t_launches += 1;
  }
  s->tev_used = 0;
  return hipSuccess;
}

// The persistent grid of a launch choice: CUs x the blocks of its kernel, block and LDS per CU.
static int blocks_for(smcrt_scene* s, LaunchChoice c) {
  int& blocks = s->grid_table[c.grid_key()];
  if (!blocks) {
    c.tk = false;  // (the test_kernel instantiation has the same block, LDS and register cap: one grid for both)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_ptr(c), kernel_threads(c), c.lds) != hipSuccess ||
        per_cu < 1)
      per_cu = 1;
    blocks = s->n_cus * per_cu;
  }
  return blocks;
}
// The larger of the scene's plain and XSRC grids of transport_kernel (or voxel_kernel, mesh_kernel):
// what the pool rules (sceneplan.h pool_slack_records) count as a launch's blocks, for every family.
static int transport_blocks(smcrt_scene* s) {
  return std::max(blocks_for(s, launch_choice(*s, false, false, 0, 0, false, false, 0)),
                  blocks_for(s, launch_choice(*s, false, true, 0, 0, false, false, 0)));
}

// Wait for the scene's stream, copy the n elements at d to the host and add them into out. Caller holds s->mu.
template <class T, class U>
static hipError_t read_add(smcrt_scene* s, const T* d, size_t n, U* out) {
  std::vector<T> h(n);
  hipError_t e = hipSetDevice(s->device);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e == hipSuccess) e = hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost);
  for (size_t i = 0; e == hipSuccess && i < n; ++i) out[i] += h[i];
  return e;
}
// Wait for the scene's stream and zero the n doubles at d. Caller holds s->mu.
static int zero_tally(smcrt_scene* s, double* d, size_t n) {
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  HIPCHK(hipMemset(d, 0, n * sizeof(double)));
  return SMCRT_OK;
}

// ---- the watchdog (transport.h watchdog_expired): d_queue[Q_WATCHDOG] holds the first
// expired wait of the scene's launches, site | (block + 1) << 8
static uint32_t* watchdog_word(smcrt_scene* s) { return (uint32_t*)(s->d_queue + Q_WATCHDOG); }
static const char* watchdog_site(uint32_t site) {
  switch (site) {
    case WDOG_PHOTON_WAVE: return "ws_kernel photon wave (every live lane waited for an event, a segment or a slot)";
    case WDOG_RING: return "ws_kernel ring producer (the token word's previous lap was never consumed)";
    case WDOG_EVENT_QUEUE: return "ws_kernel event-queue producer (the entry's previous lap was never consumed)";
    case WDOG_BUCKET: return "bucket wait (deposit.h: the pending claim never rebased the tile word)";
    default: return "unknown site";
  }
}
// After the scene's launches have finished: SMCRT_ERR_DEVICE_FAULT naming the first expired
// wait, if any (the word is cleared, so the scene stays usable).
static int take_watchdog(smcrt_scene* s) {
  uint32_t w = 0;
  HIPCHK(hipMemcpy(&w, watchdog_word(s), sizeof w, hipMemcpyDeviceToHost));
  if (!w) return SMCRT_OK;
  HIPCHK(hipMemset(watchdog_word(s), 0, sizeof w));
  return fail(SMCRT_ERR_DEVICE_FAULT, std::string("watchdog: a wait exceeded SMCRT_WATCHDOG_MS at ") +
                                          watchdog_site(w & 0xFFu) + " in block " + std::to_string((w >> 8) - 1u) +
                                          "; the run's tallies are incomplete");
}

extern "C" {

int smcrt_abi_version(void) { return SMCRT_ABI_VERSION; }

const char* smcrt_last_error(void) { return g_last_error.c_str(); }

int smcrt_device_count(int32_t* count) {
  if (!count) return fail(SMCRT_ERR_INVALID_ARG, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e == hipErrorNoDevice) n = 0;
  else if (e != hipSuccess) return fail(SMCRT_ERR_HIP, hipGetErrorString(e));
  *count = n;
  return SMCRT_OK;
}

void smcrt_scene_destroy(smcrt_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  if (s->fstream) (void)hipStreamSynchronize(s->fstream);
  for (int i = 0; i < MAX_SLOTS; ++i)
    if (s->lstream[i]) (void)hipStreamSynchronize(s->lstream[i]);
  delete s;  // every member releases what it owns (devmem.h)
}

// The plan's arrays in device memory, the queue words, and the launch streams with their events.
static int upload_plan(smcrt_scene* s) {
  int st;
  if ((st = upload(s->d_nodes, s->h_nodes.data(), s->h_nodes.size(), "scene upload")) ||
      (st = upload(s->d_prog, s->prog.data(), s->prog.size(), "scene upload")) ||
      (st = upload(s->d_props, s->h_props.data(), s->h_props.size(), "scene upload")) ||
      (st = upload(s->d_faces, s->faces.data(), s->faces.size(), "scene upload")) ||
      (st = upload(s->d_dets, s->h_dets.data(), s->h_dets.size(), "scene upload")) ||
      (st = upload(s->d_det_off, s->h_det_off.data(), s->h_det_off.size(), "scene upload")) ||
      (!s->ctab.empty() && (st = upload(s->d_ctab, s->ctab.data(), s->ctab.size(), "scene upload"))) ||
      (st = dalloc(s->d_queue, Q_COUNT)) || (st = dalloc(s->d_cold, COLD_SLOTS)) ||
      (st = dalloc(s->d_counters, SMCRT_NCOUNTERS)) || (st = dalloc(s->d_small, (size_t)s->det_total + 1 + 24)))
    return st;
  hipError_t e = hipMemset(s->d_queue, 0, Q_COUNT * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipStreamCreateWithFlags(s->stream.out(), hipStreamNonBlocking);
  for (int i = 0; i < MAX_SLOTS && e == hipSuccess; ++i) {
    e = hipStreamCreateWithFlags(s->lstream[i].out(), hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(s->lev[i].out(), hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(s->ev_in.out(), hipEventDisableTiming);
  if (e != hipSuccess) return fail(SMCRT_ERR_HIP, std::string("scene upload: ") + hipGetErrorString(e));
  return SMCRT_OK;
}

// The culling grid as one blob [ProgOp always | u32 off | u32 list | double lb | float elb],
// each 16-B aligned, and the CullGrid that points into it.
static int upload_cull(smcrt_scene* s) {
  const CullHost& cull = s->cull;
  std::vector<ProgOp> pa;
  for (int32_t t : cull.always)
    for (int32_t ip = s->top_first[t]; ip < s->top_first[t + 1]; ++ip) pa.push_back(s->prog[ip]);
  auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t b_pa = al(pa.size() * sizeof(ProgOp)), b_off = al(cull.off.size() * 4),
               b_list = al(std::max<size_t>(1, cull.list.size()) * 4), b_lb = al(cull.lb.size() * 8),
               b_elb = al(std::max<size_t>(1, cull.elb.size()) * 4);
  std::vector<unsigned char> blob(b_pa + b_off + b_list + b_lb + b_elb, 0);
  std::memcpy(blob.data(), pa.data(), pa.size() * sizeof(ProgOp));
  std::memcpy(blob.data() + b_pa, cull.off.data(), cull.off.size() * 4);
  std::memcpy(blob.data() + b_pa + b_off, cull.list.data(), cull.list.size() * 4);
  std::memcpy(blob.data() + b_pa + b_off + b_list, cull.lb.data(), cull.lb.size() * 8);
  std::memcpy(blob.data() + b_pa + b_off + b_list + b_lb, cull.elb.data(), cull.elb.size() * 4);
  int st;
  if ((st = upload(s->d_cull_data, blob.data(), blob.size(), "cull upload"))) return st;
  const unsigned char* base = s->d_cull_data;
  CullGrid G;
  for (int a = 0; a < 3; ++a) { G.lo[a] = cull.lo[a]; G.n[a] = cull.n[a]; }
  G.cell = cull.cell;
  G.inv_cell = 1.0 / cull.cell;
  G.n_prog_always = (int32_t)pa.size();
  G.prog_always = base;
  G.off = (const uint32_t*)(base + b_pa);
  G.list = (const uint32_t*)(base + b_pa + b_off);
  G.lb = (const double*)(base + b_pa + b_off + b_list);
  G.elb = (const float*)(base + b_pa + b_off + b_list + b_lb);
  if ((st = upload(s->d_cull, &G, 1, "cull upload"))) return st;
  if (s->cull_log)  // diagnostics
    std::fprintf(stderr, "[cull] %d tops, %zu always, %d x %d x %d cells of %.4g, %.1f tops per cell\n",
                 s->n_top, cull.always.size(), cull.n[0], cull.n[1], cull.n[2], cull.cell, cull.mean_list);
  s->cull.off = {}; s->cull.list = {}; s->cull.elb = {}; s->cull.lb = {};  // (the host copy is not needed again)
  return SMCRT_OK;
}

// Binned deposition (deposit.h): the per-tile and per-slot state, the fold stream and its events.
static int create_fold_state(smcrt_scene* s) {
  int st;
  if ((st = dalloc(s->d_tile_count, s->n_tiles)) || (st = dalloc(s->d_tile_start, s->n_tiles))) return st;
  for (int i = 0; i < MAX_SLOTS; ++i)
    if ((st = dalloc(s->d_dep_ctl[i], 8)) || (st = dalloc(s->d_bin_counts[i], (size_t)s->n_tiles * BIN_BLOCKS))) return st;
  s->scatter_lds = scatter_lds_bytes(s->n_tiles);
  if (hipFuncSetAttribute((const void*)bin_scatter, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)s->scatter_lds) != hipSuccess)
    return fail(SMCRT_ERR_HIP, "bin_scatter LDS attribute");
  // The fold stream gets the highest priority (SMCRT_FOLD_PRIO=0: normal). At the default
  // priority HIP maps it onto one of the process's shared hardware queues (4 by default),
  // behind a launch stream's persistent transport kernels, and a fold waited ~60 ms for
  // them; a high-priority stream has its own queue, and its
  // workgroups are dispatched first when a CU frees.
  int prio_least = 0, prio_greatest = 0;
  const bool fold_prio = s->fold_prio &&
                         hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) == hipSuccess &&
                         prio_greatest != prio_least;
  bool ok = s->h_ctl.alloc(8 * MAX_SLOTS) == hipSuccess &&
            hipEventCreateWithFlags(s->ev_t.out(), hipEventDisableTiming) == hipSuccess &&
            (fold_prio ? hipStreamCreateWithPriority(s->fstream.out(), hipStreamNonBlocking, prio_greatest)
                       : hipStreamCreateWithFlags(s->fstream.out(), hipStreamNonBlocking)) == hipSuccess;
  for (int i = 0; ok && i < MAX_SLOTS; ++i)
    ok = hipEventCreateWithFlags(s->ctl_ev[i].out(), hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(s->ev_f[i].out(), hipEventDisableTiming) == hipSuccess;
  if (!ok) return fail(SMCRT_ERR_HIP, "pinned/event/stream allocation failed");
  std::memset(s->h_ctl, 0, 8 * MAX_SLOTS * sizeof(uint32_t));
  return SMCRT_OK;
}

// The grids sized at creation: ws_kernel's, for the lean path's lane scratch (without it the scene
// keeps transport_kernel, which needs none), and transport_blocks for the pool rules.
static void size_grids(smcrt_scene* s) {
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || cus < 1) cus = 256;
  s->n_cus = cus;
  int khz = 0;  // s_memrealtime's rate
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, s->device) == hipSuccess && khz > 0) s->wall_khz = khz;
  s->lean_ok = s->lean_candidate;
  if (s->lean_ok) {
    const int ws_blocks = blocks_for(s, launch_choice(*s, true, false, 1, SMCRT_FLAG_PATHLENGTH, false, false, 0));
    if (plan_xf(*s)) {  // the lane scratch, per launch stream
      s->lscratch_stride = (kinst_ws_scratch_bytes((size_t)ws_blocks * kinst_ws_photon_lanes()) + 255) & ~(size_t)255;
      if (s->d_lscratch.alloc(s->lscratch_stride * N_QUEUES) != hipSuccess) {
        (void)hipGetLastError();
        s->lean_ok = false;
      }
    }
  }
  if (s->verbose)  // (the transport grid is sized after this line: it has always read 0)
    std::fprintf(stderr, "[smcrt] scene: lean %d (ws slots %d, blocks/CU %d, static LDS %zu + dynamic %zu B), transport grid %d\n",
                 (int)s->lean_ok, s->ws_slots, s->grid_table[GRID_KEY_WS] / std::max(1, cus), kinst_ws_shared_bytes(s->ws_slots),
                 lean_lds(*s), s->grid_table[0]);
  (void)transport_blocks(s);
}

// What the scene-creation functions share once their planner has succeeded: the device checks, the
// scene with the plan moved in, the uploads (`upload_kind`: the kind's own), the fold state, the grids.
static int create_scene(ScenePlan&& plan, int32_t device, int (*upload_kind)(smcrt_scene*), smcrt_scene** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SMCRT_ERR_NO_DEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(SMCRT_ERR_INVALID_ARG, "device ordinal out of range");
  std::unique_ptr<smcrt_scene, void (*)(smcrt_scene*)> s(new smcrt_scene(), smcrt_scene_destroy);
  static_cast<ScenePlan&>(*s) = std::move(plan);
  s->device = device;
  if (hipSetDevice(device) != hipSuccess) return fail(SMCRT_ERR_HIP, "hipSetDevice failed");
  int st;
  if ((st = upload_plan(s.get())) || (st = upload_kind(s.get())) || (s->n_tiles && (st = create_fold_state(s.get()))))
    return st;
  size_grids(s.get());
  *out = s.release();
  return SMCRT_OK;
}

int smcrt_scene_create(const smcrt_sdf_node* nodes, int32_t n_nodes, const int32_t* top, int32_t n_top,
                       const smcrt_grid* grid, const smcrt_detector* dets, int32_t n_dets, int32_t device,
                       smcrt_scene** out) {
  g_last_error.clear();
  if (!out) return fail(SMCRT_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  const PlanLimits lim{kinst_ws_shared_bytes(2), kinst_ws_shared_bytes(3)};
  ScenePlan plan;
  if (const int st = plan_scene(nodes, n_nodes, top, n_top, grid, dets, n_dets, read_knobs(), lim, &plan)) return st;
  return create_scene(std::move(plan), device, [](smcrt_scene* s) { return s->cull.enabled ? upload_cull(s) : SMCRT_OK; }, out);
}

int smcrt_voxel_scene_create(const uint8_t* labels, const smcrt_medium* media, int32_t n_media, const smcrt_grid* grid,
                             const smcrt_detector* dets, int32_t n_dets, int32_t device, smcrt_scene** out) {
  g_last_error.clear();
  if (!out) return fail(SMCRT_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  ScenePlan plan;
  if (const int st = plan_voxel_scene(labels, media, n_media, grid, dets, n_dets, read_knobs(), &plan)) return st;
  return create_scene(std::move(plan), device,
                      [](smcrt_scene* s) { return upload(s->d_labels, s->labels.data(), s->labels.size(), "label upload"); }, out);
}

int smcrt_mesh_scene_create(const double* verts, int32_t nv, const int32_t* tris, const uint8_t* tri_media, int32_t nt,
                            const smcrt_medium* media, int32_t n_media, int32_t ambient, const smcrt_grid* grid,
                            const smcrt_detector* dets, int32_t n_dets, int32_t device, smcrt_scene** out) {
  g_last_error.clear();
  if (!out) return fail(SMCRT_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  ScenePlan plan;
  if (const int st = plan_mesh_scene(verts, nv, tris, tri_media, nt, media, n_media, ambient, grid, dets, n_dets,
                                     read_knobs(), &plan))
    return st;
  return create_scene(std::move(plan), device, [](smcrt_scene* s) {
    int st;
    if ((st = upload(s->d_mesh_nodes, s->mesh_nodes.data(), s->mesh_nodes.size(), "mesh node upload")) ||
        (st = upload(s->d_mesh_tris, s->mesh_tris.data(), s->mesh_tris.size(), "mesh triangle upload")))
      return st;
    return upload(s->d_mesh_faces, s->mesh_faces.data(), s->mesh_faces.size(), "mesh face upload");
  }, out);
}

int smcrt_scene_det_bins(const smcrt_scene* s, int64_t* n) {
  if (!s || !n) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  *n = s->det_total;
  return SMCRT_OK;
}

int smcrt_scene_set_optprops(smcrt_scene* s, int32_t i, double mus, double mua, double hgg, double n) {
  return smcrt::scene_set_node_props(s, i, mus, mua, hgg, n, 0);  // a mono: init_mono's rules
}

int smcrt_scene_get_optprops(const smcrt_scene* s, int32_t i, int32_t* layer, double* mus, double* mua, double* hgg,
                             double* n) {
  if (!s || i < 0 || i >= s->n_top) return fail(SMCRT_ERR_INVALID_ARG, "bad scene or index");
  const smcrt_sdf_node& nd = s->h_nodes[s->h_top[i]];
  if (layer) *layer = nd.layer;
  if (mua) *mua = nd.mua;
  if (mus) *mus = s->h_props[i].kappa - nd.mua;  // getKappa() - getMua(), kernelsMod.f90:1574-1575
  if (hgg) *hgg = nd.hgg;
  if (n) *n = nd.n;
  return SMCRT_OK;
}

}  // extern "C"

int smcrt::scene_node_optprops(const smcrt_scene* s, int32_t i, double out[4]) {
  if (!s || i < 0 || i >= s->n_top) return fail(SMCRT_ERR_INVALID_ARG, "bad scene or index");
  const smcrt_sdf_node& nd = s->h_nodes[s->h_top[i]];
  out[0] = nd.mus; out[1] = nd.mua; out[2] = nd.hgg; out[3] = nd.n;
  return SMCRT_OK;
}

int smcrt::scene_set_node_props(smcrt_scene* s, int32_t i, double mus, double mua, double hgg, double n,
                                int32_t flags) {
  if (!s || i < 0 || i >= s->n_top) return fail(SMCRT_ERR_INVALID_ARG, "bad scene or index");
  std::lock_guard<std::mutex> g(s->mu);
  smcrt_sdf_node& nd = s->h_nodes[s->h_top[i]];
  nd.mus = mus; nd.mua = mua; nd.hgg = hgg; nd.n = n;
  nd.flags = flags;
  s->h_props[i] = make_props(nd);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemcpyAsync(s->d_props + i, &s->h_props[i], sizeof(TopProps), hipMemcpyHostToDevice, s->stream));
  HIPCHK(hipStreamSynchronize(s->stream));
  return SMCRT_OK;
}

int smcrt::scene_node_flags(const smcrt_scene* s, int32_t i, int32_t* flags) {
  if (!s || i < 0 || i >= s->n_top) return fail(SMCRT_ERR_INVALID_ARG, "bad scene or index");
  *flags = s->h_nodes[s->h_top[i]].flags;
  return SMCRT_OK;
}

int smcrt::scene_needs_sdf(const smcrt_scene* s, const char* what) {
  if (!s || !(s->voxel || s->mesh)) return SMCRT_OK;
  return fail(SMCRT_ERR_UNSUPPORTED, std::string(what) + (s->voxel ? " is not supported on voxel scenes (smcrt_voxel_scene_create)"
                                                                  : " is not supported on mesh scenes (smcrt_mesh_scene_create)"));
}

// The LDS that a launch with partial path lengths adds on this scene (launch_choice's ppl_lds): 0
// while they are not configured.
static size_t ppl_lds_of(const smcrt_scene* s) { return s->ppath_on ? ppl_lds_bytes(*s) : 0; }

// SMCRT_FLAG_PARTIAL_PATHS needs a voxel or a mesh scene (ppath.h: transport_kernel and ws_kernel
// have no accumulator).
static int ppl_flag_scene_ok(const smcrt_scene* s, uint32_t flags) {
  if (!(flags & SMCRT_FLAG_PARTIAL_PATHS) || s->voxel || s->mesh) return SMCRT_OK;
  return fail(SMCRT_ERR_UNSUPPORTED, "SMCRT_FLAG_PARTIAL_PATHS is not supported on SDF scenes (smcrt_scene_create): "
                                     "partial path lengths are kept by voxel and mesh scenes only");
}

// The run flags a voxel or a mesh scene has no code for (voxel.h, mesh.h).
static int sdfless_flags_ok(const smcrt_scene* s, uint32_t flags) {
  if (!s->voxel && !s->mesh) return SMCRT_OK;
  if (flags & SMCRT_FLAG_TEST_KERNEL) return smcrt::scene_needs_sdf(s, "SMCRT_FLAG_TEST_KERNEL");
  if (flags & SMCRT_FLAG_END_EARLY) return smcrt::scene_needs_sdf(s, "SMCRT_FLAG_END_EARLY");
  if (flags & SMCRT_FLAG_TRACK_PATHS) return smcrt::scene_needs_sdf(s, "SMCRT_FLAG_TRACK_PATHS");
  if (flags & SMCRT_FLAG_PHASOR) return smcrt::scene_needs_sdf(s, "SMCRT_FLAG_PHASOR");
  return SMCRT_OK;
}

int smcrt::scene_device(const smcrt_scene* s) { return s->device; }
void* smcrt::scene_stream(const smcrt_scene* s) { return (void*)s->stream; }

int smcrt::scene_inflight(smcrt_scene* s) {
  std::lock_guard<std::mutex> g(s->mu);
  int n = 0;
  for (int i = 0; i < MAX_SLOTS; ++i) {
    if (s->lpending[i] && hipEventQuery(s->lev[i]) == hipSuccess) s->lpending[i] = false;
    n += s->lpending[i] ? 1 : 0;
  }
  return n;
}
int smcrt::scene_depth(const smcrt_scene* s) { return s->n_slots; }

int smcrt::scene_det_size(const smcrt_scene* s, int32_t d, int64_t* n) {
  if (!s || d < 0 || d >= s->n_dets) return fail(SMCRT_ERR_INVALID_ARG, "bad scene or detector");
  *n = (d + 1 < s->n_dets ? s->h_det_off[d + 1] : s->det_total) - s->h_det_off[d];
  return SMCRT_OK;
}

extern "C" {

// Refine the records-per-photon estimate from the last binned launch, if it has landed.
static void refine_rpp(smcrt_scene* s) {
  for (int i = 0; i < s->n_slots; ++i) {
    const int sl = s->last_slot < 0 ? i : (s->last_slot + 1 + i) % s->n_slots;  // the oldest slot first
    if (s->ctl_pending[sl] && hipEventQuery(s->ctl_ev[sl]) == hipSuccess) {
      s->ctl_pending[sl] = false;
      const uint32_t* h = s->h_ctl + 8 * sl;
      if (pool_log_knob())
        std::fprintf(stderr, "[pool] slot %d: %u photons, %u records, %u overflowed, %u of %llu chunks\n", sl, h[4],
                     h[3], h[1], h[0], (unsigned long long)s->pool_chunks);
      if (h[4] > 0) {
        const double rpp = (double)(h[3] + h[1]) / (double)h[4];
        s->rpp_est = std::max(1.0, rpp);
        s->rpp_measured = true;
      }
    }
  }
}

// Wait (host) for every fold in flight: before the shared fold buffers are reallocated.
static hipError_t drain_folds(smcrt_scene* s) {
  if (!s->fstream) return hipSuccess;
  const hipError_t e = hipStreamSynchronize(s->fstream);
  for (bool& f : s->f_pending) f = false;
  return e;
}

// Make sure the record pool holds `records` (grow only). Returns false if it cannot.
static bool ensure_pool(smcrt_scene* s, uint64_t records) {
  // (the pool is counted in CHUNK_RECORDS units on both paths: a chunk is 64 buckets)
  uint64_t chunks = (records + CHUNK_RECORDS - 1) / CHUNK_RECORDS;
  if (s->pool_cap_chunks) chunks = std::min(chunks, s->pool_cap_chunks);
  if (chunks <= s->pool_chunks) return true;
  // grow with 25% headroom so launch-to-launch jitter of the estimate never reallocates
  // (a reallocation synchronises the device)
  chunks = std::min<uint64_t>(chunks + chunks / 4, MAX_POOL_RECORDS / CHUNK_RECORDS);
  if (s->pool_cap_chunks) chunks = std::min(chunks, s->pool_cap_chunks);
  // the launches and folds in flight (on any stream) use these buffers
  (void)hipDeviceSynchronize();
  (void)drain_folds(s);
  auto release = [&]() {
    s->d_sorted.reset(); s->d_pieces.reset(); s->d_order.reset();
    for (int i = 0; i < MAX_SLOTS; ++i) { s->d_pool[i].reset(); s->d_chunk_fill[i].reset(); s->d_bucket_tile[i].reset(); }
    s->pool_chunks = 0;
  };
  release();
  const uint64_t cap = chunks * CHUNK_RECORDS;
  // The slot depth (sceneplan.h slot_depth): tail-bound scenes (M4, M5) need it to fill the
  // CUs a launch's last photons leave idle; scenes of the lean kernel and of the far-field
  // march keep two (with eight hardware queues, i.e. launches really four deep, two slots
  // measured M1 211 vs 194-202 M photons/s and M2 15.5-16.4 vs 14.3-14.8 M, same box,
  // profiles/r03_s3/hwq_slots_ab.txt).
  size_t mfree = 0, mtotal = 0;
  if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess) mtotal = 0;
  s->n_slots = slot_depth(read_pool_knobs(), s->lean_ok || s->fm_err > 0.0, cap * 8, mtotal);
  s->slot = 0;  // (the device is idle here: every slot and stream is free)
  s->lturn = 0;
  s->last_slot = -1;
  // pieces <= records / piece size + one partial piece per tile (deposit.h bin_scan, bk_scan)
  const uint64_t pieces = std::min<uint64_t>(cap / MIN_PIECE_RECORDS, REDUCE_PIECES + 1) + s->n_tiles + 1;
  const uint64_t buckets = cap / BUCKET_RECORDS;
  bool ok = s->d_pieces.alloc(pieces) == hipSuccess;
  for (int i = 0; ok && i < s->n_slots; ++i) {
    ok = s->d_pool[i].alloc(cap) == hipSuccess;
    if (ok && s->bucketed)  // bucket fills and bucket tiles, per slot
      ok = s->d_chunk_fill[i].alloc(buckets) == hipSuccess && s->d_bucket_tile[i].alloc(buckets) == hipSuccess;
    else if (ok)  // chunk fills, per slot
      ok = s->d_chunk_fill[i].alloc(chunks) == hipSuccess;
  }
  if (ok && s->bucketed)  // the tile-ordered list of bucket ids and fills (folds are serial)
    ok = s->d_order.alloc(buckets) == hipSuccess;
  else if (ok)  // the tile-sorted copy of the records
    ok = s->d_sorted.alloc(cap) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    release();
    return false;
  }
  s->pool_chunks = chunks;
  s->max_pieces = pieces;
  return true;
}


// The next event quad of a timed scene (smcrt_scene_kernel_times), or null.
static int next_timing_events(smcrt_scene* s, Event** ev) {
  *ev = nullptr;
  if (!s->timing) return SMCRT_OK;
  if (s->tev_used == MAX_TIMED) HIPCHK(harvest_times(s));
  while (4 * (s->tev_used + 1) > s->tev.size()) {
    Event e;
    HIPCHK(hipEventCreate(e.out()));
    s->tev.push_back(std::move(e));
  }
  *ev = &s->tev[4 * s->tev_used++];
  return SMCRT_OK;
}

// One transport launch on `stream` (queue index qi) into record slot `sl` (binned): the
// launch's cold parameters, the cleared queue head and deposit state, then the kernel.
static int enqueue_transport(smcrt_scene* s, const KParams& K, KCold Ch, const LaunchChoice& c, hipStream_t stream,
                             int sl, int qi, Event** ev_out) {
  const bool binned = K.rec_pool != nullptr;
  if (binned && s->f_pending[sl]) HIPCHK(hipStreamWaitEvent(stream, s->ev_f[sl], 0));  // slot free
  Ch.queue = s->d_queue + qi;  // (a queue head per stream: overlapped launches run concurrently)
  Ch.lane_scratch = s->d_lscratch ? (double*)(s->d_lscratch + (size_t)qi * s->lscratch_stride) : nullptr;
  HIPCHK(hipMemsetAsync(Ch.queue, 0, sizeof(unsigned long long), stream));
  // this launch's cold parameters: a ring slot, written in stream order before the kernel.
  // (Each stream has its own ring of slots, so a slot is only ever rewritten in stream order
  // after the launch that read it.)
  const KCold* C = s->d_cold + (size_t)qi * COLD_PER_STREAM + (s->cold_seq[qi]++ % COLD_PER_STREAM);
  HIPCHK(hipMemcpyAsync((void*)C, &Ch, sizeof(KCold), hipMemcpyHostToDevice, stream));
  if (binned) {
    HIPCHK(hipMemsetAsync(s->d_dep_ctl[sl], 0, 8 * sizeof(uint32_t), stream));
    if (K.bucket_tiles)  // per-tile bucket counts
      HIPCHK(hipMemsetAsync(s->d_bin_counts[sl], 0, (size_t)s->n_tiles * sizeof(uint32_t), stream));
    else if (K.hist_tiles)
      HIPCHK(hipMemsetAsync(s->d_bin_counts[sl], 0, (size_t)s->n_tiles * BIN_BLOCKS * sizeof(uint32_t), stream));
  }
  if (const int st = next_timing_events(s, ev_out)) return st;
  Event* ev = *ev_out;
  if (ev) HIPCHK(hipEventRecord(ev[0], stream));
  // as many blocks as the photons need: waves of 64 in blocks of 4, or ws_kernel's photon lanes per block
  const bool ws = c.family == KF_WS;
  const uint64_t per_block = ws ? (uint64_t)kinst_ws_photon_lanes() : 256;
  const int blocks = (int)std::min<uint64_t>((uint64_t)blocks_for(s, c),
                                             std::max<uint64_t>(1, (Ch.n_photons + per_block - 1) / per_block));
  if (ws) ++s->lean_launches;
  // ws_kernel takes (K, nodes, prog, C); transport_kernel, voxel_kernel and mesh_kernel the detectors too
  const smcrt_sdf_node* a_nodes = K.nodes;
  const ProgOp* a_prog = K.prog;
  const smcrt_detector* a_dets = K.dets;
  const int64_t* a_off = K.det_off;
  void* args_ws[] = {(void*)&K, (void*)&a_nodes, (void*)&a_prog, (void*)&C};
  void* args[] = {(void*)&K, (void*)&a_nodes, (void*)&a_prog, (void*)&a_dets, (void*)&a_off, (void*)&C};
  HIPCHK(hipLaunchKernel(kernel_ptr(c), dim3(blocks), dim3(kernel_threads(c)), ws ? args_ws : args, c.lds, stream));
  HIPCHK(hipGetLastError());
  if (ev) HIPCHK(hipEventRecord(ev[1], stream));
  return SMCRT_OK;
}

// The deposit fold of the launch just enqueued on `stream`, on s->fstream, ordered after it
// by an event. The fold of the previous launch may still run while this transport kernel
// does: they touch different slots (and jmean is only written by folds, which are serial on
// fstream).
static int enqueue_fold(smcrt_scene* s, const KParams& K, double* jmean, hipStream_t stream, int sl, Event* ev) {
  if (!K.rec_pool) {  // no fold: an empty interval
    if (ev) {
      HIPCHK(hipEventRecord(ev[2], stream));
      HIPCHK(hipEventRecord(ev[3], stream));
    }
    return SMCRT_OK;
  }
  hipStream_t fs = s->fstream;
  HIPCHK(hipEventRecord(s->ev_t, stream));
  HIPCHK(hipStreamWaitEvent(fs, s->ev_t, 0));
  if (ev) HIPCHK(hipEventRecord(ev[2], fs));
  const uint32_t nch = (uint32_t)s->pool_chunks;
  const uint64_t nv = (uint64_t)s->grid.nx * s->grid.ny * s->grid.nz;
  if (K.bucket_tiles) {  // bucketed: list each tile's buckets, then sum them
    hipLaunchKernelGGL(bk_scan, dim3(1), dim3(1024), 0, fs, s->d_bin_counts[sl], s->n_tiles, s->d_tile_start,
                       s->d_tile_count, s->d_pieces, s->d_dep_ctl[sl]);
    hipLaunchKernelGGL(bk_place, dim3(BIN_BLOCKS), dim3(BIN_THREADS), 0, fs, s->d_bucket_tile[sl], s->d_chunk_fill[sl],
                       s->d_dep_ctl[sl], K.n_buckets, s->n_tiles, s->d_tile_count, s->d_order);
#ifndef SMCRT_ABL_NO_FOLD  // timing ablation only: records are never summed (not exact)
    hipLaunchKernelGGL(bk_reduce, dim3(1024), dim3(RED_THREADS), 0, fs, s->d_pool[sl], s->d_order, s->d_pieces,
                       s->d_dep_ctl[sl], nv, jmean, s->d_queue + Q_FOLD_TICKS);
#endif
  } else {
    if (!K.hist_tiles)  // else the transport kernel built the counts
      hipLaunchKernelGGL(bin_hist, dim3(BIN_BLOCKS), dim3(BIN_THREADS), 0, fs, s->d_pool[sl], s->d_chunk_fill[sl],
                         s->d_dep_ctl[sl], nch, s->n_tiles, s->d_bin_counts[sl]);
    hipLaunchKernelGGL(bin_rowscan, dim3(s->n_tiles), dim3(BIN_BLOCKS), 0, fs, s->d_bin_counts[sl],
                       s->d_tile_count);
    hipLaunchKernelGGL(bin_scan, dim3(1), dim3(1024), 0, fs, s->d_tile_count, s->n_tiles, s->d_tile_start,
                       s->d_pieces, s->d_dep_ctl[sl]);
    hipLaunchKernelGGL(bin_scatter, dim3(BIN_BLOCKS), dim3(BIN_THREADS), s->scatter_lds, fs, s->d_pool[sl],
                       s->d_chunk_fill[sl], s->d_dep_ctl[sl], nch, s->n_tiles, s->d_tile_start, s->d_bin_counts[sl],
                       s->d_sorted, (uint64_t)s->pool_chunks * CHUNK_RECORDS);
    hipLaunchKernelGGL(bin_reduce, dim3(1024), dim3(1024), 0, fs, s->d_sorted, s->d_pieces, s->d_dep_ctl[sl], nv,
                       jmean);
  }
  HIPCHK(hipGetLastError());
  // remember how many records this launch produced (read back lazily, never waited for)
  HIPCHK(hipMemcpyAsync(s->h_ctl + 8 * sl, s->d_dep_ctl[sl], 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, fs));
  HIPCHK(hipMemcpyAsync(s->h_ctl + 8 * sl + 5, s->d_dep_ctl[sl] + 5, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, fs));
  HIPCHK(hipEventRecord(s->ctl_ev[sl], fs));
  s->ctl_pending[sl] = true;
  if (ev) HIPCHK(hipEventRecord(ev[3], fs));
  HIPCHK(hipEventRecord(s->ev_f[sl], fs));
  s->f_pending[sl] = true;
  s->last_slot = sl;
  return SMCRT_OK;
}

#ifdef SMCRT_DIAG
// Diagnostic builds: wait for the launch and print the kernels' schedule tallies.
static int diag_report(hipStream_t stream, bool lean) {
  unsigned long long h[72], ht[9], hc[6];
  HIPCHK(hipStreamSynchronize(stream));
  kinst_diag_gather(h, ht, hc);
  if (lean) {  // ws_kernel's tallies (ws.h WD_*)
    const double wi = (double)std::max(1ull, h[20]), pt = (double)std::max(1ull, h[24]);
    std::fprintf(stderr, "[diag-ws] walker iters %llu: idle %.3f, busy lanes/iter %.1f, pending lanes/iter %.1f | "
                 "photon trips %llu: sleep %.3f, idle lanes %.1f, sync-waiting %.2f, slot-blocked %.2f, EVAL lanes "
                 "%.1f, pushes %.2f, P7 runs %.3f (lanes/run %.1f), event-waiting %.2f | producer waits %llu | event "
                 "iters %llu, lanes/iter %.1f | emissions waiting for a slot %llu lane-trips | out-of-order hand-outs "
                 "%llu (%.3f of the pushes)\n",
                 h[20], h[21] / wi, h[22] / wi, h[23] / wi, h[24], h[25] / pt, h[30] / pt, h[27] / pt, h[26] / pt,
                 h[31] / pt, h[32] / pt, h[28] / pt, (double)h[29] / (double)std::max(1ull, h[28]), h[36] / pt, h[33],
                 h[34], (double)h[35] / (double)std::max(1ull, h[34]), h[51], h[52],
                 (double)h[52] / (double)std::max(1ull, h[32]));
    // region times (ws.h WST): shares of each role's wave time
    const char* np[8] = {"fetch", "poll", "eval", "p3p4", "handout", "p5p6", "p7", "p8"};
    double tp = 0, tw = 0, te = 0;
    for (int i = 0; i < 8; ++i) tp += (double)h[37 + i];
    for (int i = 0; i < 4; ++i) tw += (double)h[45 + i];
    te = (double)h[49] + (double)h[50];
    std::fprintf(stderr, "[diag-ws-time] photon:");
    for (int i = 0; i < 8; ++i) std::fprintf(stderr, " %s=%.3f", np[i], (double)h[37 + i] / std::max(1.0, tp));
    std::fprintf(stderr, " | walker: claim=%.3f idle=%.3f walk=%.3f finish=%.3f | event: run=%.3f idle=%.3f | "
                 "ticks photon/walker/event %.3g/%.3g/%.3g\n", h[45] / std::max(1.0, tw), h[46] / std::max(1.0, tw),
                 h[47] / std::max(1.0, tw), h[48] / std::max(1.0, tw), h[49] / std::max(1.0, te),
                 h[50] / std::max(1.0, te), tp, tw, te);
  }
  unsigned long long lt = 0;
  for (int i = 0; i < 64; ++i) lt += h[i];
  std::fprintf(stderr, "[diag] waves %llu, longest wave %llu trips %llu ticks\n", h[70], h[68], h[69]);
  std::fprintf(stderr, "[diag] trips %llu dda %llu eval %llu p7 %llu | lane-trips %llu:", h[64], h[65], h[66],
               h[67], lt);
  for (int i = 0; i < 64; ++i)
    if (h[i]) std::fprintf(stderr, " %s%d=%.3f", i >= 32 ? "seg:" : "", i & 31, (double)h[i] / (double)lt);
  std::fprintf(stderr, "\n");

  double tt = 0;
  for (int i = 1; i < 9; ++i) tt += (double)ht[i];
  const char* nm_t[9] = {"", "fetch", "eval", "p3", "p4", "dda", "p5p6", "p7", "p8"};
  const char* nm_l[9] = {"", "fetch", "eval", "p3p4", "push", "walk", "p5p6", "p7", "p8"};
  const char* const* nm = lean ? nm_l : nm_t;
  std::fprintf(stderr, "[diag-time]");
  for (int i = 1; i < 9; ++i) std::fprintf(stderr, " %s=%.3f", nm[i], (double)ht[i] / tt);
  std::fprintf(stderr, "\n");

  if (hc[0] + hc[2])
    std::fprintf(stderr, "[diag-cull] culled lane-EVALs %llu, bound fallbacks %llu (%.4f), capture/outside %llu, "
                 "mean list %.1f, wave-EVALs %llu with a full fallback %.3f\n", hc[0], hc[1],
                 (double)hc[1] / (double)std::max(1ull, hc[0]), hc[2], (double)hc[3] / (double)std::max(1ull, hc[0]),
                 hc[4], (double)hc[5] / (double)std::max(1ull, hc[4]));
  return SMCRT_OK;
}
#endif

// One launch: the transport kernel on `stream`, then its fold on s->fstream.
static int launch_one(smcrt_scene* s, const KParams& K, const KCold& Ch, bool xsrc, hipStream_t stream, int sl, int qi) {
  const LaunchChoice c = launch_choice(*s, s->lean_ok, xsrc, K.bucket_tiles, K.flags, s->path_on, s->phasor_on, s->screens.size(),
                                       ppl_lds_of(s));
  Event* ev = nullptr;
  int st = enqueue_transport(s, K, Ch, c, stream, sl, qi, &ev);
  if (!st) st = enqueue_fold(s, K, Ch.jmean, stream, sl, ev);
#ifdef SMCRT_DIAG
  if (!st) st = diag_report(stream, c.family == KF_WS);
#endif
  return st;
}

// Batched point sources (smcrt_run_origins): device origin table and per-origin detector totals.
struct OriginRun {
  const double* d_origins;
  double* d_totals;
  uint64_t per_origin, first;
};

// The parameters every batch of a launch shares (launch() sets the per-batch pool fields).
static int fill_params(smcrt_scene* s, const smcrt_source* src, const smcrt_run_config* cfg,
                       const smcrt_device_tallies& dt, const SrcPlan& plan, hipStream_t stream, bool diag_done_ok,
                       const LaunchChoice& run, KParams& K, KCold& Ch) {
  const LaunchKnobs knobs = read_launch_knobs();
  K.nodes = s->d_nodes;
  K.prog = s->d_prog;
  K.n_prog = s->n_prog;
  K.coop_lanes = s->coop_lanes;
  K.cull = s->d_cull;
  K.ctab = s->d_ctab;
  const bool far = s->fm_err > 0.0 && (cfg->flags & SMCRT_FLAG_PATHLENGTH);
  K.fm_err = far ? s->fm_err : 0.0;
  K.fm_step = s->fm_step;
  K.inv2x = s->inv2[0]; K.inv2y = s->inv2[1]; K.inv2z = s->inv2[2];
  K.fex = s->fe[0]; K.fey = s->fe[1]; K.fez = s->fe[2];
  K.props = s->d_props;
  K.xface = s->d_faces;
  K.yface = s->d_faces + (s->grid.nx + 1);
  K.zface = s->d_faces + (s->grid.nx + 1) + (s->grid.ny + 1);
  K.dets = s->d_dets;
  K.det_off = s->d_det_off;
  K.n_top = s->n_top;
  K.n_dets = s->n_dets;
  K.nx = s->grid.nx; K.ny = s->grid.ny; K.nz = s->grid.nz;
  K.xmax = s->grid.xmax; K.ymax = s->grid.ymax; K.zmax = s->grid.zmax;
  K.flags = cfg->flags;
  Ch.src = *src;
  Ch.plan = plan;
  K.key0 = (uint32_t)cfg->seed;
  K.key1 = (uint32_t)(cfg->seed >> 32);
  Ch.jmean = dt.jmean; Ch.absorb = dt.absorb; Ch.emission = dt.emission;
  Ch.chunk_fill = nullptr; Ch.dep_ctl = nullptr; Ch.bin_counts = nullptr;  // (per slot: launch)
  Ch.bucket_tile = nullptr; Ch.bucket_fill = nullptr; Ch.tile_nb = nullptr;
  Ch.det_bins = dt.det_bins; Ch.nscatt = dt.nscatt; Ch.moments = dt.moments;
  Ch.counters = (unsigned long long*)dt.counters;
  Ch.queue = nullptr;  // (set per launch: enqueue_transport)
  Ch.far_steps = s->d_queue + Q_FAR_STEPS;
  Ch.lean_hazards = s->d_queue + Q_LEAN_HAZARDS;
  Ch.invoxel_segs = s->d_queue + Q_INVOXEL;
  Ch.ooo_handouts = s->d_queue + Q_OOO_HANDOUTS;
  Ch.lane_scratch = nullptr;  // (per launch stream: enqueue_transport)
  Ch.watchdog = watchdog_word(s);
  const bool hist = run.hist, phas = run.phas, scr = run.scr;  // (the run's launch choice)
  Ch.hist_scratch = hist ? (double*)s->d_hist_scratch : nullptr;
  Ch.path_vertices = hist ? (double*)s->d_path_vertices : nullptr;
  Ch.path_headers = hist ? (smcrt_path*)s->d_path_headers : nullptr;
  Ch.path_ctl = hist ? (unsigned long long*)s->d_path_ctl : nullptr;
  Ch.hist_lanes = hist ? s->hist_lanes : 0;
  Ch.path_max = hist ? (uint64_t)s->path_cfg.max_paths : 0;
  const bool ppl = run.ppl;
  Ch.range_first = hist ? s->path_cfg.range_first : ppl ? s->ppath_cfg.range_first : 0;
  Ch.range_count = hist ? s->path_cfg.range_count : ppl ? s->ppath_cfg.range_count : 0;
  // partial path lengths: the arena, and where the lanes' lengths start in the launch's LDS (what
  // launch_choice sizes it with: media and faces, then the plan's deposit words)
  Ch.ppl_lengths = ppl ? (double*)s->d_ppl_lengths : nullptr;
  Ch.ppl_headers = ppl ? (smcrt_ppath*)s->d_ppl_headers : nullptr;
  Ch.ppl_ctl = ppl ? (unsigned long long*)s->d_ppl_ctl : nullptr;
  Ch.ppl_max = ppl ? (uint64_t)s->ppath_cfg.max_records : 0;
  Ch.ppl_lds_off = ppl ? (uint32_t)((s->face_bytes + (size_t)dep_words(*s) * sizeof(uint32_t)) / sizeof(double)) : 0u;
  Ch.ppl_n_media = ppl ? (uint32_t)s->n_top : 0u;
  Ch.hist_max_vertices = hist ? (uint32_t)s->path_cfg.max_vertices : 0;
  // the phasor tally: the wavenumber of photons that sample no wavelength of their own is the
  // fixed one, or 2 pi / the constant spectrum's value (NULL spectrum: 500.0, smcrt.h)
  Ch.phasor = phas ? (double*)s->d_phasor : nullptr;
  Ch.phasor_fixed = phas && s->phasor_cfg.fixed_k ? 1u : 0u;
  Ch.phasor_k = !phas ? 0.0
                : s->phasor_cfg.fixed_k ? s->phasor_cfg.wavenumber
                                        : 6.283185307179586 / (src->spectrum ? src->spectrum->wavelength : 500.0);
  // field screens and the optical-path option: a phasor launch only (a voxel or a mesh scene
  // has neither: smcrt_scene_set_phasor and smcrt_scene_set_screens refuse them)
  Ch.screens = scr ? (const ScreenDev*)s->d_screens : nullptr;
  Ch.screen_field = scr ? (double*)s->d_screen_field : nullptr;
  Ch.n_screens = scr ? (uint32_t)s->screens.size() : 0u;
  Ch.phasor_optical = phas && (s->phasor_cfg.reserved & SMCRT_PHASOR_OPTICAL_PATH) ? 1u : 0u;
  // the volume source's table (emit_ext reads it for SMCRT_SRC_VOLUME only; launch() has checked it)
  const bool vsrc = src->kind == SMCRT_SRC_VOLUME && s->d_vs_cdf;
  Ch.vs_cdf = vsrc ? (const double*)s->d_vs_cdf : nullptr;
  Ch.vs_xface = vsrc ? K.xface : nullptr;
  Ch.vs_yface = vsrc ? K.yface : nullptr;
  Ch.vs_zface = vsrc ? K.zface : nullptr;
  Ch.vs_total = vsrc ? s->vs_total : 0.0;
  Ch.vs_nvox = vsrc ? (uint32_t)((int64_t)s->grid.nx * s->grid.ny * s->grid.nz) : 0u;
  Ch.vs_last = vsrc ? (uint32_t)s->vs_last : 0u;
  Ch.vox_labels = s->d_labels;
  Ch.vox_n_media = s->voxel ? (uint32_t)s->n_top : 0u;
  Ch.vox_reserved = 0;
  Ch.mesh_nodes = s->d_mesh_nodes;
  Ch.mesh_tris = s->d_mesh_tris;
  Ch.mesh_faces = s->d_mesh_faces;
  Ch.mesh_n_nodes = (uint32_t)s->mesh_nodes.size();
  Ch.mesh_ambient = (uint32_t)s->mesh_ambient;
#ifdef SMCRT_DIAG
  Ch.done_time = nullptr;
  Ch.done_base = cfg->first_photon;
  if (knobs.diag_done && diag_done_ok) {  // (diagnostic builds: completion times)
    s->n_done = cfg->n_photons;
    HIPCHK(s->d_done.alloc(s->n_done));
    HIPCHK(hipMemsetAsync(s->d_done, 0, sizeof(unsigned long long) * s->n_done, stream));
    Ch.done_time = s->d_done;
  }
#else
  (void)stream; (void)diag_done_ok;
#endif
  // every cross-wave wait is bounded (transport.h watchdog_expired); 0 ms: unbounded
  Ch.watchdog_ticks = knobs.watchdog_ms > 0.0 ? (uint64_t)(knobs.watchdog_ms * (double)s->wall_khz) : 0ull;
  K.rec_pool = nullptr; K.n_chunks = 0; K.hist_tiles = 0; K.bucket_tiles = 0; K.n_buckets = 0;
  K.claim_delay = knobs.claim_delay;
  K.lean_debug = s->lean_debug | (knobs.drop_event ? 4u : 0u) | (knobs.eval_loop ? 8u : 0u);
  K.ws_invoxel = ws_invoxel_on(s->ws_invoxel, plan_xf(*s)) ? 1u : 0u;  // (read by ws_kernel only)
  lean_margins(K.lean_debug, s->grid, K.lean_lo, K.lean_hi);
  return SMCRT_OK;
}

static int launch(smcrt_scene* s, const smcrt_source* src, const smcrt_run_config* cfg,
                  const smcrt_device_tallies& dt, hipStream_t stream, const OriginRun* orun = nullptr) {
  if (src->kind < SMCRT_SRC_POINT || src->kind > SMCRT_SRC_VOLUME) return fail(SMCRT_ERR_INVALID_ARG, "bad source kind");
  if (src->kind == SMCRT_SRC_VOLUME) {
    if (orun) return fail(SMCRT_ERR_UNSUPPORTED, "smcrt_run_origins: a volume source has no origin to batch");
    if (!s->d_vs_cdf)
      return fail(SMCRT_ERR_INVALID_ARG, "a volume source needs smcrt_scene_set_volume_source first (the scene holds no table)");
  }
  if (const int pst = ppl_flag_scene_ok(s, cfg->flags)) return pst;  // (every driver ends here)
  if (cfg->n_photons == 0) return SMCRT_OK;
  // sources other than point/uniform/pencil, a sampled spectrum or batched origins: the
  // general emitter
  const bool xsrc = src_needs_plan(src) || orun || s->nested;
  SrcPlan plan;
  std::memset(&plan, 0, sizeof plan);
  if (xsrc) {
    std::vector<double> px, py, pc;
    const char* perr = "";
    const int pst = build_src_plan(src, &s->grid, &plan, px, py, pc, &perr);
    if (pst) return fail(pst, perr);
    std::vector<double> tab;
    tab.reserve(px.size() + py.size() + pc.size());
    tab.insert(tab.end(), px.begin(), px.end());
    tab.insert(tab.end(), py.begin(), py.end());
    tab.insert(tab.end(), pc.begin(), pc.end());
    if (!tab.empty()) {
      if (tab != s->h_spec) {  // new tables: wait for launches that may still read the old ones
        HIPCHK(hipStreamSynchronize(stream));
        if (s->stream != stream) HIPCHK(hipStreamSynchronize(s->stream));
        if (tab.size() > s->spec_cap) {
          s->spec_cap = 0;
          HIPCHK(s->d_spec.alloc(tab.size()));
          s->spec_cap = tab.size();
        }
        HIPCHK(hipMemcpy(s->d_spec, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        s->h_spec = tab;
      }
      plan.spec_x = px.empty() ? nullptr : s->d_spec;
      plan.spec_y = py.empty() ? nullptr : s->d_spec + px.size();
      plan.cdf = s->d_spec + px.size() + py.size();
    }
    if (orun) {
      plan.origins = orun->d_origins;
      plan.det_totals = orun->d_totals;
      plan.per_origin = orun->per_origin;
      plan.first = orun->first;
    }
  }
  KParams K;
  KCold Ch;
  // (hist, phas and scr are those of every batch: a batch that runs ws_kernel has none of the three)
  const LaunchChoice run = launch_choice(*s, false, xsrc, 0, cfg->flags, s->path_on, s->phasor_on, s->screens.size(),
                                         ppl_lds_of(s));
  if (const int st = fill_params(s, src, cfg, dt, plan, stream, !orun, run, K, Ch)) return st;
  const bool binned = launch_binned(*s, dt.jmean != nullptr, cfg->flags);
  const bool overlap = (cfg->flags & SMCRT_FLAG_OVERLAP) != 0;
  if (overlap) {  // the internal streams start after the caller's earlier work
    HIPCHK(hipEventRecord(s->ev_in, stream));
    for (int i = 0; i < MAX_SLOTS; ++i) HIPCHK(hipStreamWaitEvent(s->lstream[i], s->ev_in, 0));
  } else {  // a plain launch runs after every overlapped one (same tallies, same buffers)
    for (int i = 0; i < MAX_SLOTS; ++i)
      if (s->lpending[i]) HIPCHK(hipStreamWaitEvent(stream, s->lev[i], 0));
  }
  for (int i = 0; i < MAX_SLOTS; ++i)  // launches known to have finished need no more waits
    if (s->lpending[i] && hipEventQuery(s->lev[i]) == hipSuccess) s->lpending[i] = false;
  for (uint64_t done = 0; done < cfg->n_photons;) {
    refine_rpp(s);
    uint64_t n = cfg->n_photons - done;
    K.rec_pool = nullptr; K.n_chunks = 0; K.hist_tiles = 0; K.bucket_tiles = 0; K.n_buckets = 0;
    bool calibrate = false;
    if (binned) {
      // records per photon are scene-dependent: the scene's first large launch starts with a
      // small calibration batch whose count is waited for once, then batches are sized to it
      if (!s->rpp_measured && n > CALIB_PHOTONS) { n = CALIB_PHOTONS; calibrate = true; }
      const uint64_t want = pool_records_for(*s, transport_blocks(s), n, s->rpp_est);
      if (!ensure_pool(s, want)) (void)ensure_pool(s, want / 4);  // smaller pool, more batches
      if (s->pool_chunks) {
        const double usable = (double)(s->pool_chunks * CHUNK_RECORDS) - pool_slack_records(*s, transport_blocks(s));
        n = std::min<uint64_t>(n, (uint64_t)std::max(65536.0, usable / (s->rpp_est * POOL_SLACK)));
        // (taken after ensure_pool: it may have reallocated the pool)
        K.rec_pool = s->d_pool[s->slot];
        Ch.chunk_fill = s->d_chunk_fill[s->slot];  // (ensure_pool may have reallocated them)
        Ch.dep_ctl = s->d_dep_ctl[s->slot];
        Ch.bin_counts = s->d_bin_counts[s->slot];
        K.n_chunks = (uint32_t)s->pool_chunks;
        K.hist_tiles = s->hist_tiles;
        if (s->bucketed) {
          Ch.bucket_fill = s->d_chunk_fill[s->slot];
          Ch.bucket_tile = s->d_bucket_tile[s->slot];
          Ch.tile_nb = s->d_bin_counts[s->slot];
          K.bucket_tiles = s->n_tiles;
          K.n_buckets = (uint32_t)(s->pool_chunks * (CHUNK_RECORDS / BUCKET_RECORDS));
        }
      }
    }
    Ch.n_photons = n;
    Ch.first_photon = orun ? done : cfg->first_photon + done;  // (origins: the global queue index)
    Ch.records = dt.records ? dt.records + done : nullptr;
    const int sl = s->slot;
    if (K.rec_pool) {
      // (the slot's previous readback must land before its photon count is replaced)
      if (s->ctl_pending[sl]) { HIPCHK(hipEventSynchronize(s->ctl_ev[sl])); refine_rpp(s); }
      s->h_ctl[8 * sl + 4] = (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull);
    }
    int st;
    if (overlap) {
      const int q = s->lturn;
      s->lturn = (s->lturn + 1) % s->n_slots;
      st = launch_one(s, K, Ch, xsrc, s->lstream[q], sl, q);
      if (!st && hipEventRecord(s->lev[q], s->lstream[q]) != hipSuccess) st = fail(SMCRT_ERR_HIP, "event record failed");
      s->lpending[q] = true;
    } else {
      st = launch_one(s, K, Ch, xsrc, stream, sl, Q_CALLER);
    }
    if (st) return st;
    if (K.rec_pool) s->slot = (s->slot + 1) % s->n_slots;
    if (calibrate && K.rec_pool) {
      HIPCHK(hipEventSynchronize(s->ctl_ev[sl]));
      refine_rpp(s);
    }
    done += n;
  }
  // the tallies are complete in `stream` order at return, unless the caller defers the folds
  if (!(cfg->flags & (SMCRT_FLAG_ASYNC_FOLD | SMCRT_FLAG_OVERLAP)) && s->last_slot >= 0 && s->f_pending[s->last_slot])
    HIPCHK(hipStreamWaitEvent(stream, s->ev_f[s->last_slot], 0));
  return SMCRT_OK;
}

int smcrt_run_device(smcrt_scene* s, const smcrt_source* src, const smcrt_run_config* cfg,
                     smcrt_device_tallies* dev, void* stream) {
  g_last_error.clear();
  if (!s || !src || !cfg || !dev) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  if (const int vst = sdfless_flags_ok(s, cfg->flags)) return vst;
  if (const int pst = ppl_flag_scene_ok(s, cfg->flags)) return pst;
  if (cfg->flags & SMCRT_FLAG_TRACK_PATHS)
    return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_TRACK_PATHS: paths are recorded by smcrt_run only");
  if (cfg->flags & SMCRT_FLAG_PHASOR)
    return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_PHASOR: the phasor grid is tallied by smcrt_run only");
  if (cfg->flags & SMCRT_FLAG_PARTIAL_PATHS)
    return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_PARTIAL_PATHS: partial path lengths are recorded by smcrt_run only");
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  return launch(s, src, cfg, *dev, (hipStream_t)stream);
}

}  // extern "C"

// smcrt_run's body; `orun` (batched origins) is set by smcrt_run_origins. Caller holds s->mu.
static int run_sync(smcrt_scene* s, const smcrt_source* src, const smcrt_run_config* cfg_in, smcrt_tallies* io,
                    const OriginRun* orun) {
  // A synchronous run returns complete tallies: its folds always join s->stream before the
  // copies, whatever the caller's flags say (SMCRT_FLAG_ASYNC_FOLD is for smcrt_run_device).
  smcrt_run_config cfg_local = *cfg_in;
  cfg_local.flags &= ~(uint32_t)(SMCRT_FLAG_ASYNC_FOLD | SMCRT_FLAG_OVERLAP);
  const smcrt_run_config* cfg = &cfg_local;
  const int64_t nv = (int64_t)s->grid.nx * s->grid.ny * s->grid.nz;
  const bool want[3] = {io->jmean || io->jmean_f64, io->absorb || io->absorb_f64, io->emission || io->emission_f64};
  if (!s->d_grids && (want[0] || want[1] || want[2])) {
    int st = dalloc(s->d_grids, (size_t)nv * 3);
    if (st) return st;
  }
  const bool rec = (cfg->flags & SMCRT_FLAG_RECORD_PHOTONS) && io->records;
  if (rec && s->records_cap < cfg->n_photons) {
    s->records_cap = 0;
    int st = dalloc(s->d_records, cfg->n_photons);
    if (st) return st;
    s->records_cap = cfg->n_photons;
  }
  smcrt_device_tallies dt{};
  for (int t = 0; t < 3; ++t) {
    if (!want[t]) continue;
    double* p = s->d_grids + (size_t)t * nv;
    HIPCHK(hipMemsetAsync(p, 0, sizeof(double) * nv, s->stream));
    if (t == 0) dt.jmean = p;
    if (t == 1) dt.absorb = p;
    if (t == 2) dt.emission = p;
  }
  HIPCHK(hipMemsetAsync(s->d_small, 0, sizeof(double) * (s->det_total + 25), s->stream));
  HIPCHK(hipMemsetAsync(s->d_counters, 0, sizeof(unsigned long long) * SMCRT_NCOUNTERS, s->stream));
  dt.det_bins = s->det_total ? s->d_small : nullptr;
  dt.nscatt = s->d_small + s->det_total;
  dt.moments = s->d_small + s->det_total + 1;
  dt.counters = (uint64_t*)s->d_counters.h;
  dt.records = rec ? s->d_records : nullptr;
  int st = launch(s, src, cfg, dt, s->stream, orun);
  if (st) return st;
  hipError_t e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return fail(SMCRT_ERR_DEVICE_FAULT, std::string("transport kernel: ") + hipGetErrorString(e));
  if ((st = take_watchdog(s))) return st;
  // copy back and accumulate
  std::vector<double> h;
  float* gf[3] = {io->jmean, io->absorb, io->emission};
  double* gd[3] = {io->jmean_f64, io->absorb_f64, io->emission_f64};
  for (int t = 0; t < 3; ++t) {
    if (!want[t]) continue;
    h.resize((size_t)nv);
    HIPCHK(hipMemcpy(h.data(), s->d_grids + (size_t)t * nv, sizeof(double) * nv, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < nv; ++i) {
      if (gf[t]) gf[t][i] = (float)((double)gf[t][i] + h[i]);
      if (gd[t]) gd[t][i] += h[i];
    }
  }
  const double* small = s->d_small;  // det bins | nscatt | moments(24)
  if (io->det_bins) HIPCHK(read_add(s, small, (size_t)s->det_total, io->det_bins));
  if (io->nscatt) HIPCHK(read_add(s, small + s->det_total, 1, io->nscatt));
  if (io->moments) HIPCHK(read_add(s, small + s->det_total + 1, 24, io->moments));
  if (io->counters) HIPCHK(read_add(s, (const unsigned long long*)s->d_counters, SMCRT_NCOUNTERS, io->counters));
  if (rec)
    HIPCHK(hipMemcpy(io->records, s->d_records, sizeof(smcrt_photon_record) * cfg->n_photons, hipMemcpyDeviceToHost));
  return SMCRT_OK;
}

extern "C" {

int smcrt_run(smcrt_scene* s, const smcrt_source* src, const smcrt_run_config* cfg, smcrt_tallies* io) {
  g_last_error.clear();
  if (!s || !src || !cfg || !io) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  if (const int vst = sdfless_flags_ok(s, cfg->flags)) return vst;
  if (const int pst = ppl_flag_scene_ok(s, cfg->flags)) return pst;
  std::lock_guard<std::mutex> g(s->mu);
  const bool ppl = (cfg->flags & SMCRT_FLAG_PARTIAL_PATHS) != 0;
  if (ppl && !(cfg->flags & SMCRT_FLAG_PATHLENGTH))
    return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_PARTIAL_PATHS needs SMCRT_FLAG_PATHLENGTH (the lengths are those of the voxel walk)");
  if (ppl && !s->ppath_on)
    return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_PARTIAL_PATHS needs smcrt_scene_set_partial_paths first");
  const bool track = (cfg->flags & SMCRT_FLAG_TRACK_PATHS) != 0;
  if (track && !s->path_on)
    return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_TRACK_PATHS needs smcrt_scene_set_path_tracking first");
  if (cfg->flags & SMCRT_FLAG_PHASOR) {
    if (!s->phasor_on) return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_PHASOR needs smcrt_scene_set_phasor first");
    if (track) return fail(SMCRT_ERR_UNSUPPORTED, "SMCRT_FLAG_PHASOR and SMCRT_FLAG_TRACK_PATHS do not combine");
    if (!(cfg->flags & SMCRT_FLAG_PATHLENGTH))
      return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_PHASOR needs SMCRT_FLAG_PATHLENGTH (the tally lives in the voxel walk)");
  }
  HIPCHK(hipSetDevice(s->device));
  if (track)  // a tracking run starts with an empty arena
    HIPCHK(hipMemsetAsync(s->d_path_ctl, 0, 3 * sizeof(unsigned long long), s->stream));
  if (ppl) HIPCHK(hipMemsetAsync(s->d_ppl_ctl, 0, 2 * sizeof(unsigned long long), s->stream));  // likewise
  return run_sync(s, src, cfg, io, nullptr);
}

int smcrt_run_origins(smcrt_scene* s, const smcrt_source* src, const double* origins, int64_t n_origins,
                      const smcrt_run_config* cfg, double* det_totals, smcrt_tallies* io) {
  g_last_error.clear();
  if (!s || !cfg || !io || (n_origins > 0 && !origins)) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  if (src && src->kind == SMCRT_SRC_VOLUME)
    return fail(SMCRT_ERR_UNSUPPORTED, "smcrt_run_origins: a volume source has no origin to batch (the batch is a point source)");
  if (const int vst = smcrt::scene_needs_sdf(s, "smcrt_run_origins")) return vst;
  if (n_origins < 0) return fail(SMCRT_ERR_INVALID_ARG, "n_origins < 0");
  if (cfg->flags & SMCRT_FLAG_TRACK_PATHS)
    return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_TRACK_PATHS: paths are recorded by smcrt_run only");
  if (cfg->flags & SMCRT_FLAG_PHASOR)
    return fail(SMCRT_ERR_INVALID_ARG, "SMCRT_FLAG_PHASOR: the phasor grid is tallied by smcrt_run only");
  if (const int pst = ppl_flag_scene_ok(s, cfg->flags)) return pst;
  if (cfg->flags & SMCRT_FLAG_RECORD_PHOTONS) return fail(SMCRT_ERR_INVALID_ARG, "photon records are not kept for batched origins");
  if (n_origins > 0xFFFFFFFFll) return fail(SMCRT_ERR_INVALID_ARG, "more than 2^32 origins");
  if (n_origins == 0 || cfg->n_photons == 0) return SMCRT_OK;
  if (cfg->n_photons > UINT64_MAX / (uint64_t)n_origins) return fail(SMCRT_ERR_INVALID_ARG, "photon count overflows");
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  smcrt_source p;  // the escape function's packet = photon("point") (kernelsMod.f90:162-166)
  if (src) p = *src;
  else std::memset(&p, 0, sizeof p);
  p.kind = SMCRT_SRC_POINT;
  const size_t nt = (size_t)n_origins * (size_t)std::max(s->n_dets, 1);
  DevBuf<double> d_org, d_tot;
  int st = dalloc(d_org, (size_t)n_origins * 3);
  if (!st) st = dalloc(d_tot, nt);
  if (!st) {
    OriginRun orun{d_org, s->n_dets ? d_tot : nullptr, cfg->n_photons, cfg->first_photon};
    smcrt_run_config c = *cfg;
    c.n_photons = cfg->n_photons * (uint64_t)n_origins;
    hipError_t e = hipMemcpy(d_org, origins, sizeof(double) * 3 * (size_t)n_origins, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_tot, 0, sizeof(double) * nt);
    if (e != hipSuccess) st = fail(SMCRT_ERR_HIP, std::string("origin upload: ") + hipGetErrorString(e));
    if (!st) st = run_sync(s, &p, &c, io, &orun);
    if (!st && det_totals && s->n_dets && (e = read_add(s, (const double*)d_tot, nt, det_totals)) != hipSuccess)
      st = fail(SMCRT_ERR_HIP, std::string("totals: ") + hipGetErrorString(e));
  }
  return st;
}

#ifdef SMCRT_DIAG
// Diagnostic builds only (not in include/smcrt.h): read and clear the kernel's lane-state
// occupancy (72) and per-phase s_memtime sums (9).
int smcrt_diag_read(unsigned long long* out) {
  HIPCHK(hipDeviceSynchronize());
  unsigned long long hc[6];
  kinst_diag_gather(out, out + 72, hc);
  return SMCRT_OK;
}
// The completion time (s_memrealtime ticks) of each photon of the scene's last run made with
// SMCRT_DIAG_DONE=1 (n of them; 0 = not completed), and the tick rate in kHz.
int smcrt_diag_done_times(smcrt_scene* s, unsigned long long* out, uint64_t n, int32_t* khz) {
  if (!s || !out || !s->d_done || n > s->n_done) return fail(SMCRT_ERR_INVALID_ARG, "no completion times");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, s->d_done, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  if (khz) *khz = s->wall_khz;
  return SMCRT_OK;
}
#endif

int smcrt_scene_info(const smcrt_scene* s, smcrt_grid* grid, int32_t* n_top, int32_t* n_dets) {
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (grid) *grid = s->grid;
  if (n_top) *n_top = s->n_top;
  if (n_dets) *n_dets = s->n_dets;
  return SMCRT_OK;
}

int smcrt_scene_classify(smcrt_scene* s, const double* points, int64_t n, int32_t* layer, double* kappa) {
  g_last_error.clear();
  if (!s || (n > 0 && (!points || !layer))) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  if (n <= 0) return SMCRT_OK;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->voxel) {  // the label of the voxel the point is in (+ 1), 0 outside the grid: host only
    for (int64_t i = 0; i < n; ++i) {
      const int32_t ci = host_vox_of(points[3 * i], s->grid.nx, s->grid.xmax),
                    cj = host_vox_of(points[3 * i + 1], s->grid.ny, s->grid.ymax),
                    ck = host_vox_of(points[3 * i + 2], s->grid.nz, s->grid.zmax);
      layer[i] = (ci < 1 || cj < 1 || ck < 1)
                     ? 0
                     : 1 + (int32_t)s->labels[(size_t)(ci - 1) + (size_t)s->grid.nx * ((size_t)(cj - 1) + (size_t)s->grid.ny * (size_t)(ck - 1))];
      if (kappa) kappa[i] = layer[i] > 0 ? s->h_props[layer[i] - 1].kappa : 0.0;
    }
    return SMCRT_OK;
  }
  if (s->mesh) {  // a host cast along (0, 0, 1) and the emission rule; 0 outside the grid: host only
    for (int64_t i = 0; i < n; ++i) {
      const bool in = host_vox_of(points[3 * i], s->grid.nx, s->grid.xmax) >= 1 &&
                      host_vox_of(points[3 * i + 1], s->grid.ny, s->grid.ymax) >= 1 &&
                      host_vox_of(points[3 * i + 2], s->grid.nz, s->grid.zmax) >= 1;
      layer[i] = in ? 1 + mesh_medium_at(*s, points + 3 * i) : 0;
      if (kappa) kappa[i] = layer[i] > 0 ? s->h_props[layer[i] - 1].kappa : 0.0;
    }
    return SMCRT_OK;
  }
  HIPCHK(hipSetDevice(s->device));
  DevBuf<double> d_pts;
  DevBuf<int32_t> d_lay;
  int st = dalloc(d_pts, (size_t)n * 3);
  if (!st) st = dalloc(d_lay, (size_t)n);
  if (!st) {
    hipError_t e = hipMemcpy(d_pts, points, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      const int blocks = (int)std::min<int64_t>((n + 255) / 256, 65535);
      hipLaunchKernelGGL(classify_kernel, dim3(blocks), dim3(256), 0, s->stream, (const smcrt_sdf_node*)s->d_nodes,
                         (const ProgOp*)s->d_prog, (int32_t)s->n_prog, (const double*)d_pts, n, d_lay);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e == hipSuccess) e = hipMemcpy(layer, d_lay, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) st = fail(SMCRT_ERR_HIP, std::string("classify: ") + hipGetErrorString(e));
  }
  if (!st && kappa)
    for (int64_t i = 0; i < n; ++i) kappa[i] = layer[i] > 0 ? s->h_props[layer[i] - 1].kappa : 0.0;
  return st;
}

int smcrt_scene_fence(smcrt_scene* s, void* stream) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  for (int i = 0; i < MAX_SLOTS; ++i)  // overlapped launches (their folds are ordered after them)
    if (s->lpending[i]) HIPCHK(hipStreamWaitEvent((hipStream_t)stream, s->lev[i], 0));
  if (s->last_slot >= 0 && s->f_pending[s->last_slot])  // folds are serial: the last covers all
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, s->ev_f[s->last_slot], 0));
  return SMCRT_OK;
}

int smcrt_scene_check(smcrt_scene* s) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  for (int i = 0; i < MAX_SLOTS; ++i)
    if (s->lstream[i]) {
      const hipError_t e = hipStreamSynchronize(s->lstream[i]);
      if (e != hipSuccess) return fail(SMCRT_ERR_DEVICE_FAULT, std::string("transport kernel: ") + hipGetErrorString(e));
    }
  for (hipStream_t st : {(hipStream_t)s->stream, (hipStream_t)s->fstream})
    if (st) {
      const hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) return fail(SMCRT_ERR_DEVICE_FAULT, std::string("transport kernel: ") + hipGetErrorString(e));
    }
  return take_watchdog(s);
}

int smcrt_scene_set_timing(smcrt_scene* s, int32_t enable) {
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  std::lock_guard<std::mutex> g(s->mu);
  s->timing = enable != 0;
  return SMCRT_OK;
}

int smcrt_scene_kernel_times(smcrt_scene* s, smcrt_kernel_times* out) {
  if (!s || !out) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(harvest_times(s));
  out->transport_ms = s->t_transport;
  out->deposit_ms = s->t_deposit;
  out->launches = s->t_launches;
  out->lean_launches = s->lean_launches;
  s->lean_launches = 0;
  unsigned long long far = 0;  // (a running total: steps of launches still running count later)
  HIPCHK(hipMemcpy(&far, s->d_queue + Q_FAR_STEPS, sizeof(far), hipMemcpyDeviceToHost));
  out->far_steps = (int64_t)(far - s->far_reported);
  s->far_reported = far;
  unsigned long long ticks = 0;  // bk_reduce workgroup run time (running total, wall-clock ticks)
  HIPCHK(hipMemcpy(&ticks, s->d_queue + Q_FOLD_TICKS, sizeof(ticks), hipMemcpyDeviceToHost));
  out->fold_cu_ms = (double)(ticks - s->fold_ticks_reported) / (double)s->wall_khz / (double)s->n_cus;
  s->fold_ticks_reported = ticks;
  unsigned long long hz = 0;  // deferred lean segments that ended in tflag / an error stop (running total)
  HIPCHK(hipMemcpy(&hz, s->d_queue + Q_LEAN_HAZARDS, sizeof(hz), hipMemcpyDeviceToHost));
  out->lean_hazards = (int64_t)(hz - s->hazards_reported);
  s->hazards_reported = hz;
  s->t_transport = s->t_deposit = 0.0;
  s->t_launches = 0;
  return SMCRT_OK;
}

int smcrt_scene_deposit_regime(const smcrt_scene* s, int32_t* regime) {
  if (!s || !regime) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  *regime = !launch_binned(*s, true, SMCRT_FLAG_PATHLENGTH) ? SMCRT_DEPOSIT_ATOMIC
            : s->bucketed                                   ? SMCRT_DEPOSIT_BUCKETS
                                                            : SMCRT_DEPOSIT_SORTED;
  return SMCRT_OK;
}

int smcrt_scene_invoxel_segments(smcrt_scene* s, int64_t* out) {
  if (!s || !out) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  if (const int vst = smcrt::scene_needs_sdf(s, "smcrt_scene_invoxel_segments")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  unsigned long long n = 0;  // (a running total: segments of launches still running count later)
  HIPCHK(hipMemcpy(&n, s->d_queue + Q_INVOXEL, sizeof(n), hipMemcpyDeviceToHost));
  *out = (int64_t)n;
  return SMCRT_OK;
}

int smcrt_scene_out_of_order_handouts(smcrt_scene* s, int64_t* out) {
  if (!s || !out) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  if (const int vst = smcrt::scene_needs_sdf(s, "smcrt_scene_out_of_order_handouts")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  unsigned long long n = 0;  // (a running total: hand-outs of launches still running count later)
  HIPCHK(hipMemcpy(&n, s->d_queue + Q_OOO_HANDOUTS, sizeof(n), hipMemcpyDeviceToHost));
  *out = (int64_t)n;
  return SMCRT_OK;
}

// ---- photon paths (paths.h) ---------------------------------------------------------
static void release_paths(smcrt_scene* s) {
  s->path_on = false;
  s->d_hist_scratch.reset(); s->d_path_vertices.reset(); s->d_path_headers.reset(); s->d_path_ctl.reset();
  s->hist_lanes = 0;
}

int smcrt_scene_set_path_tracking(smcrt_scene* s, const smcrt_path_config* cfg) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = smcrt::scene_needs_sdf(s, "path tracking")) return vst;
  if (cfg) {  // (decided before any device call)
    if (cfg->max_vertices < 2 || cfg->max_vertices > 1024)
      return fail(SMCRT_ERR_INVALID_ARG, "path tracking: max_vertices must lie in 2 .. 1024");
    if (cfg->max_paths < 1) return fail(SMCRT_ERR_INVALID_ARG, "path tracking: max_paths must be >= 1");
    if (cfg->range_count > UINT64_MAX - cfg->range_first)
      return fail(SMCRT_ERR_INVALID_ARG, "path tracking: the photon range overflows");
  }
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));  // (no launch of this scene may still use the buffers)
  release_paths(s);
  if (!cfg) return SMCRT_OK;
  int hist_blocks = 0;  // the larger of the HIST instantiations' persistent grids (plain, XSRC)
  for (int x = 0; x < 2; ++x)
    hist_blocks = std::max(hist_blocks, blocks_for(s, launch_choice(*s, false, x == 1, 0, SMCRT_FLAG_TRACK_PATHS, true, false, 0)));
  const uint64_t lanes = (uint64_t)hist_blocks * 256ull;
  const uint64_t mv = (uint64_t)cfg->max_vertices, mp = (uint64_t)cfg->max_paths;
  if (mp > (1ull << 40) / mv) return fail(SMCRT_ERR_OOM, "path tracking: the arena does not fit");
  int st;
  if ((st = dalloc(s->d_hist_scratch, (size_t)(lanes * mv * 4))) || (st = dalloc(s->d_path_vertices, (size_t)(mp * mv * 4))) ||
      (st = dalloc(s->d_path_headers, (size_t)mp)) || (st = dalloc(s->d_path_ctl, 3))) {
    (void)hipGetLastError();
    release_paths(s);
    return st;
  }
  HIPCHK(hipMemset(s->d_path_ctl, 0, 3 * sizeof(unsigned long long)));
  s->path_cfg = *cfg;
  s->hist_lanes = lanes;
  s->path_on = true;
  return SMCRT_OK;
}

// The arena's counters and headers (the used slots) after the scene's launches. Caller holds s->mu.
static int fetch_paths(smcrt_scene* s, unsigned long long ctl[3], std::vector<smcrt_path>& hdr) {
  if (!s->path_on) return fail(SMCRT_ERR_INVALID_ARG, "path tracking is not configured on this scene");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  HIPCHK(hipMemcpy(ctl, s->d_path_ctl, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const uint64_t n = std::min<uint64_t>(ctl[0], (uint64_t)s->path_cfg.max_paths);
  hdr.resize((size_t)n);
  if (n) HIPCHK(hipMemcpy(hdr.data(), s->d_path_headers, (size_t)n * sizeof(smcrt_path), hipMemcpyDeviceToHost));
  for (smcrt_path& p : hdr)  // (the library's own bound, whatever the device wrote)
    p.n_stored = std::min<uint32_t>(p.n_stored, (uint32_t)s->path_cfg.max_vertices);
  return SMCRT_OK;
}

int smcrt_scene_path_counts(smcrt_scene* s, int64_t* n_paths, int64_t* n_vertices, int64_t* n_dropped,
                            int64_t* n_truncated) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = smcrt::scene_needs_sdf(s, "path tracking")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  unsigned long long ctl[3];
  std::vector<smcrt_path> hdr;
  if (const int st = fetch_paths(s, ctl, hdr)) return st;
  int64_t nv = 0;
  for (const smcrt_path& p : hdr) nv += p.n_stored;
  if (n_paths) *n_paths = (int64_t)hdr.size();
  if (n_vertices) *n_vertices = nv;
  if (n_dropped) *n_dropped = (int64_t)ctl[1];
  if (n_truncated) *n_truncated = (int64_t)ctl[2];
  return SMCRT_OK;
}

int smcrt_scene_read_paths(smcrt_scene* s, smcrt_path* paths, double* vertices) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = smcrt::scene_needs_sdf(s, "path tracking")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  unsigned long long ctl[3];
  std::vector<smcrt_path> hdr;
  if (const int st = fetch_paths(s, ctl, hdr)) return st;
  if (hdr.empty()) return SMCRT_OK;
  if (!paths || !vertices) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  // arena order is whatever the atomics gave: (photon, hit) makes the output deterministic
  std::vector<size_t> order(hdr.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    if (hdr[a].photon != hdr[b].photon) return hdr[a].photon < hdr[b].photon;
    if (hdr[a].hit != hdr[b].hit) return hdr[a].hit < hdr[b].hit;
    return a < b;
  });
  const size_t mv = (size_t)s->path_cfg.max_vertices;
  std::vector<double> arena(hdr.size() * mv * 4);
  HIPCHK(hipMemcpy(arena.data(), s->d_path_vertices, arena.size() * sizeof(double), hipMemcpyDeviceToHost));
  int64_t off = 0;
  for (size_t k = 0; k < order.size(); ++k) {
    const size_t slot = order[k];
    paths[k] = hdr[slot];
    paths[k].offset = off;
    std::memcpy(vertices + 4 * off, arena.data() + slot * mv * 4, (size_t)hdr[slot].n_stored * 4 * sizeof(double));
    off += hdr[slot].n_stored;
  }
  return SMCRT_OK;
}

// ---- partial path lengths (ppath.h) ------------------------------------------------------
static void release_ppaths(smcrt_scene* s) {
  s->ppath_on = false;
  s->d_ppl_lengths.reset(); s->d_ppl_headers.reset(); s->d_ppl_ctl.reset();
}

// The three entry points serve voxel and mesh scenes only.
static int ppaths_scene_ok(const smcrt_scene* s) {
  if (s->voxel || s->mesh) return SMCRT_OK;
  return fail(SMCRT_ERR_UNSUPPORTED, "partial path lengths are not supported on SDF scenes (smcrt_scene_create): "
                                     "they are kept by voxel and mesh scenes only");
}

int smcrt_scene_set_partial_paths(smcrt_scene* s, const smcrt_ppath_config* cfg) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = ppaths_scene_ok(s)) return vst;
  uint64_t mr = 0;
  const uint64_t nm = (uint64_t)s->n_top;
  if (cfg) {  // (decided before any device call)
    if (cfg->max_records < 1) return fail(SMCRT_ERR_INVALID_ARG, "partial path lengths: max_records must be >= 1");
    if (cfg->reserved != 0) return fail(SMCRT_ERR_INVALID_ARG, "partial path lengths: reserved must be 0");
    if (cfg->range_count > UINT64_MAX - cfg->range_first)
      return fail(SMCRT_ERR_INVALID_ARG, "partial path lengths: the photon range overflows");
    if (s->n_top > PPL_MAX_MEDIA)
      return fail(SMCRT_ERR_UNSUPPORTED, "partial path lengths: the scene has " + std::to_string(s->n_top) +
                                             " media, more than the cap of " + std::to_string(PPL_MAX_MEDIA) +
                                             " (SMCRT_PPATH_MAX_MEDIA: the lengths live in the kernels' LDS)");
    // a block's LDS with the lengths: what launch_choice asks for, next to the kernels' counters
    const size_t lds = launch_choice(*s, false, false, 0, SMCRT_FLAG_PATHLENGTH | SMCRT_FLAG_PARTIAL_PATHS, false, false, 0,
                                     ppl_lds_bytes(*s)).lds + SDFLESS_STATIC_LDS;
    if (lds > LDS_BYTES)
      return fail(SMCRT_ERR_UNSUPPORTED, "partial path lengths: a block would need " + std::to_string(lds) +
                                             " bytes of LDS, more than " + std::to_string(LDS_BYTES));
    mr = (uint64_t)cfg->max_records;
    if (mr > (1ull << 40) / (nm * sizeof(double) + sizeof(smcrt_ppath)))
      return fail(SMCRT_ERR_OOM, "partial path lengths: the arena does not fit");
  }
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));  // (no launch of this scene may still use the buffers)
  release_ppaths(s);
  if (!cfg) return SMCRT_OK;
  int st;
  if ((st = dalloc(s->d_ppl_lengths, (size_t)(mr * nm))) || (st = dalloc(s->d_ppl_headers, (size_t)mr)) ||
      (st = dalloc(s->d_ppl_ctl, 2))) {
    (void)hipGetLastError();
    release_ppaths(s);
    return st;
  }
  HIPCHK(hipMemset(s->d_ppl_ctl, 0, 2 * sizeof(unsigned long long)));
  s->ppath_cfg = *cfg;
  s->ppath_on = true;
  // (the tracking launches' persistent grids: asked for once, here)
  for (int x = 0; x < 2; ++x)
    (void)blocks_for(s, launch_choice(*s, false, x == 1, 0, SMCRT_FLAG_PATHLENGTH | SMCRT_FLAG_PARTIAL_PATHS, false, false, 0,
                                      ppl_lds_of(s)));
  return SMCRT_OK;
}

// The arena's counters and headers (the used slots) after the scene's launches. Caller holds s->mu.
static int fetch_ppaths(smcrt_scene* s, unsigned long long ctl[2], std::vector<smcrt_ppath>& hdr) {
  if (!s->ppath_on) return fail(SMCRT_ERR_INVALID_ARG, "partial path lengths are not configured on this scene");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));
  HIPCHK(hipMemcpy(ctl, s->d_ppl_ctl, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const uint64_t n = std::min<uint64_t>(ctl[0], (uint64_t)s->ppath_cfg.max_records);
  hdr.resize((size_t)n);
  if (n) HIPCHK(hipMemcpy(hdr.data(), s->d_ppl_headers, (size_t)n * sizeof(smcrt_ppath), hipMemcpyDeviceToHost));
  return SMCRT_OK;
}

int smcrt_scene_partial_path_counts(smcrt_scene* s, int64_t* n_records, int64_t* n_dropped) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = ppaths_scene_ok(s)) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  unsigned long long ctl[2];
  std::vector<smcrt_ppath> hdr;
  if (const int st = fetch_ppaths(s, ctl, hdr)) return st;
  if (n_records) *n_records = (int64_t)hdr.size();
  if (n_dropped) *n_dropped = (int64_t)ctl[1];
  return SMCRT_OK;
}

int smcrt_scene_read_partial_paths(smcrt_scene* s, smcrt_ppath* headers, double* lengths) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = ppaths_scene_ok(s)) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  unsigned long long ctl[2];
  std::vector<smcrt_ppath> hdr;
  if (const int st = fetch_ppaths(s, ctl, hdr)) return st;
  if (hdr.empty()) return SMCRT_OK;
  if (!headers || !lengths) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  // arena order is whatever the atomics gave: (photon, hit) makes the output deterministic
  std::vector<size_t> order(hdr.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    if (hdr[a].photon != hdr[b].photon) return hdr[a].photon < hdr[b].photon;
    if (hdr[a].hit != hdr[b].hit) return hdr[a].hit < hdr[b].hit;
    return a < b;
  });
  const size_t nm = (size_t)s->n_top;
  std::vector<double> arena(hdr.size() * nm);
  HIPCHK(hipMemcpy(arena.data(), s->d_ppl_lengths, arena.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < order.size(); ++k) {
    headers[k] = hdr[order[k]];
    std::memcpy(lengths + k * nm, arena.data() + order[k] * nm, nm * sizeof(double));
  }
  return SMCRT_OK;
}

// ---- the phasor tally (phasor.h) ----------------------------------------------------
int smcrt_scene_set_phasor(smcrt_scene* s, const smcrt_phasor_config* cfg) {
  g_last_error.clear();
  if (cfg && cfg->fixed_k && !(cfg->wavenumber >= 0.0 && cfg->wavenumber <= 0x1.fffffffffffffp+1023))
    return fail(SMCRT_ERR_INVALID_ARG, "phasor: a fixed wavenumber must be finite and >= 0");  // (before any device call)
  if (cfg && (cfg->reserved & ~SMCRT_PHASOR_OPTICAL_PATH))
    return fail(SMCRT_ERR_INVALID_ARG, "phasor: reserved has bits set other than SMCRT_PHASOR_OPTICAL_PATH");
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = smcrt::scene_needs_sdf(s, "the phasor tally")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));  // (no launch of this scene may still use the grid)
  s->phasor_on = false;
  s->d_phasor.reset();
  if (!cfg) return SMCRT_OK;
  for (int scr = 0; scr < 2; ++scr)  // the PHAS instantiations' grids (plain, XSRC), without and with the screens' LDS row
    for (int x = 0; x < 2; ++x) (void)blocks_for(s, launch_choice(*s, false, x == 1, 0, SMCRT_FLAG_PHASOR, false, true, scr));
  const size_t n2 = 2 * (size_t)s->grid.nx * (size_t)s->grid.ny * (size_t)s->grid.nz;
  if (const int st = dalloc(s->d_phasor, n2)) {
    (void)hipGetLastError();
    s->d_phasor.reset();
    return st;
  }
  HIPCHK(hipMemset(s->d_phasor, 0, n2 * sizeof(double)));
  s->phasor_cfg = *cfg;
  s->phasor_on = true;
  return SMCRT_OK;
}

int smcrt_scene_read_phasor(smcrt_scene* s, double* out) {
  g_last_error.clear();
  if (!s || !out) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  if (const int vst = smcrt::scene_needs_sdf(s, "the phasor tally")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  if (!s->phasor_on) return fail(SMCRT_ERR_INVALID_ARG, "the phasor tally is not configured on this scene");
  HIPCHK(read_add(s, (const double*)s->d_phasor, 2 * (size_t)s->grid.nx * (size_t)s->grid.ny * (size_t)s->grid.nz, out));
  return SMCRT_OK;
}

int smcrt_scene_reset_phasor(smcrt_scene* s) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = smcrt::scene_needs_sdf(s, "the phasor tally")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  if (!s->phasor_on) return fail(SMCRT_ERR_INVALID_ARG, "the phasor tally is not configured on this scene");
  return zero_tally(s, s->d_phasor, 2 * (size_t)s->grid.nx * (size_t)s->grid.ny * (size_t)s->grid.nz);
}

// ---- field screens (screen.h, phasor.h screen_hits) -------------------------------------
int smcrt_scene_set_screens(smcrt_scene* s, const smcrt_screen* screens, int32_t n) {
  g_last_error.clear();
  const bool off = !screens || n == 0;
  std::vector<ScreenDev> plan;
  int64_t nd = 0;
  if (!off)  // (before any device call)
    if (const int st = plan_screens(screens, n, &plan, &nd)) return st;
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = smcrt::scene_needs_sdf(s, "field screens")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));  // (no launch of this scene may still use the buffer)
  s->screens.clear();
  s->screen_doubles = 0;
  s->d_screens.reset();
  s->d_screen_field.reset();
  if (off) return SMCRT_OK;
  int st = upload(s->d_screens, plan.data(), plan.size(), "screens: table");
  if (!st) st = dalloc(s->d_screen_field, (size_t)nd);
  if (st) {
    (void)hipGetLastError();
    s->d_screens.reset();
    s->d_screen_field.reset();
    return st;
  }
  HIPCHK(hipMemset(s->d_screen_field, 0, (size_t)nd * sizeof(double)));
  s->screens = std::move(plan);
  s->screen_doubles = nd;
  return SMCRT_OK;
}

int smcrt_scene_screen_info(const smcrt_scene* s, int32_t* n, int64_t* n_doubles) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (n) *n = (int32_t)s->screens.size();
  if (n_doubles) *n_doubles = s->screen_doubles;
  return SMCRT_OK;
}

int smcrt_scene_read_screens(smcrt_scene* s, double* out) {
  g_last_error.clear();
  if (!s || !out) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  if (const int vst = smcrt::scene_needs_sdf(s, "field screens")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->screens.empty()) return fail(SMCRT_ERR_INVALID_ARG, "no screens are configured on this scene");
  HIPCHK(read_add(s, (const double*)s->d_screen_field, (size_t)s->screen_doubles, out));
  return SMCRT_OK;
}

int smcrt_scene_reset_screens(smcrt_scene* s) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (const int vst = smcrt::scene_needs_sdf(s, "field screens")) return vst;
  std::lock_guard<std::mutex> g(s->mu);
  if (s->screens.empty()) return fail(SMCRT_ERR_INVALID_ARG, "no screens are configured on this scene");
  return zero_tally(s, s->d_screen_field, (size_t)s->screen_doubles);
}

int smcrt_screen_hit(const smcrt_screen* screen, const double start[3], const double dir[3], double sep, double* t,
                     int32_t* pixel) {
  g_last_error.clear();
  if (!screen || !start || !dir || !t || !pixel) return fail(SMCRT_ERR_INVALID_ARG, "NULL argument");
  std::vector<ScreenDev> plan;
  int64_t nd = 0;
  if (const int st = plan_screens(screen, 1, &plan, &nd)) return st;  // (the statuses are negative)
  double tt = 0.0;
  int32_t px = 0;
  if (!screen_hit(plan[0], v3(start[0], start[1], start[2]), v3(dir[0], dir[1], dir[2]), sep, tt, px)) return 0;
  *t = tt;
  *pixel = px;
  return 1;
}

// ---- the volume source (volsrc.h, emit_ext case SMCRT_SRC_VOLUME) -------------------------
int smcrt_scene_set_volume_source(smcrt_scene* s, const double* weights) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  std::vector<double> cdf;
  int64_t last = 0, np = 0, nr = 0;
  if (weights)  // (before any device call)
    if (const int st = plan_volume_source(weights, (int64_t)s->grid.nx * s->grid.ny * s->grid.nz, &cdf, &last, &np, &nr))
      return st;
  std::lock_guard<std::mutex> g(s->mu);
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipStreamSynchronize(s->stream));  // (no launch of this scene may still read the table)
  for (int i = 0; i < MAX_SLOTS; ++i)
    if (s->lpending[i]) HIPCHK(hipEventSynchronize(s->lev[i]));
  s->d_vs_cdf.reset();
  s->vs_last = s->vs_positive = s->vs_reachable = 0;
  s->vs_total = 0.0;
  if (!weights) return SMCRT_OK;
  if (const int st = upload(s->d_vs_cdf, cdf.data(), cdf.size(), "volume source: table")) {
    (void)hipGetLastError();
    s->d_vs_cdf.reset();
    return st;
  }
  s->vs_last = last; s->vs_positive = np; s->vs_reachable = nr;
  s->vs_total = cdf.back();
  return SMCRT_OK;
}

int smcrt_scene_volume_source_info(const smcrt_scene* s, int64_t* n_positive, int64_t* n_reachable, double* total) {
  g_last_error.clear();
  if (!s) return fail(SMCRT_ERR_INVALID_ARG, "scene is NULL");
  if (n_positive) *n_positive = s->vs_positive;
  if (n_reachable) *n_reachable = s->vs_reachable;
  if (total) *total = s->vs_total;
  return SMCRT_OK;
}

int smcrt_volume_pick(const double* weights, int64_t nvox, const double* u, int64_t m, int64_t* voxel) {
  g_last_error.clear();
  if (!weights || m < 0 || (m > 0 && (!u || !voxel))) return fail(SMCRT_ERR_INVALID_ARG, "volume pick: bad arguments");
  std::vector<double> cdf;
  int64_t last = 0, np = 0, nr = 0;
  if (const int st = plan_volume_source(weights, nvox, &cdf, &last, &np, &nr)) return st;
  for (int64_t i = 0; i < m; ++i) {
    if (!(u[i] >= 0.0 && u[i] < 1.0))
      return fail(SMCRT_ERR_INVALID_ARG, "volume pick: uniform " + std::to_string(i) + " is not in [0, 1)");
    voxel[i] = (int64_t)volsrc_pick(cdf.data(), (uint32_t)nvox, (uint32_t)last, cdf.back(), u[i]);
  }
  return SMCRT_OK;
}

int smcrt_volume_sample(const double* weights, const smcrt_grid* g, uint64_t seed, uint64_t first, int64_t n, double* pos,
                        double* dir, int64_t* voxel) {
  g_last_error.clear();
  if (!weights || !g || n < 0) return fail(SMCRT_ERR_INVALID_ARG, "volume sample: bad arguments");
  if (g->nx < 1 || g->ny < 1 || g->nz < 1 || !(g->xmax > 0.0) || !(g->ymax > 0.0) || !(g->zmax > 0.0) ||
      !std::isfinite(g->xmax) || !std::isfinite(g->ymax) || !std::isfinite(g->zmax))
    return fail(SMCRT_ERR_INVALID_ARG, "volume sample: bad grid");
  const int64_t nvox = (int64_t)g->nx * g->ny * g->nz;
  std::vector<double> cdf;
  int64_t last = 0, np = 0, nr = 0;
  if (const int st = plan_volume_source(weights, nvox, &cdf, &last, &np, &nr)) return st;
  const std::vector<double> faces = grid_faces(g);  // (as every scene has them)
  const double* xf = faces.data();
  const double* yf = xf + (g->nx + 1);
  const double* zf = yf + (g->ny + 1);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int64_t i = 0; i < n; ++i) {
    // the photon's stream (detmath.h Rng): draw d is the (d & 1) half of block (d >> 1, 0, pid_lo, pid_hi)
    const uint64_t pid = first + (uint64_t)i;
    double u[6];
    for (uint32_t b = 0; b < 3; ++b) {
      uint32_t c[4] = {b, 0u, (uint32_t)pid, (uint32_t)(pid >> 32)};
      host_philox(c, k0, k1);
      u[2 * b] = (double)((((uint64_t)c[1] << 32) | c[0]) >> 11) * 0x1.0p-53;
      u[2 * b + 1] = (double)((((uint64_t)c[3] << 32) | c[2]) >> 11) * 0x1.0p-53;
    }
    const uint32_t v = volsrc_pick(cdf.data(), (uint32_t)nvox, (uint32_t)last, cdf.back(), u[0]);
    const uint32_t ci = v % (uint32_t)g->nx, cj = (v / (uint32_t)g->nx) % (uint32_t)g->ny,
                   ck = v / ((uint32_t)g->nx * (uint32_t)g->ny);
    if (voxel) voxel[i] = (int64_t)v;
    if (pos) {
      pos[3 * i] = volsrc_place(xf[ci], xf[ci + 1], u[1], g->xmax);
      pos[3 * i + 1] = volsrc_place(yf[cj], yf[cj + 1], u[2], g->ymax);
      pos[3 * i + 2] = volsrc_place(zf[ck], zf[ck + 1], u[3], g->zmax);
    }
    if (dir) {
      const V3 d = volsrc_dir(u[4], u[5]);
      dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z;
    }
  }
  return SMCRT_OK;
}

int smcrt_normalise_fluence(float* g, const smcrt_grid* grid, uint64_t nphotons) {
  if (!g || !grid || nphotons == 0) return fail(SMCRT_ERR_INVALID_ARG, "bad arguments");
  // writer.f90:25-52, evaluated in double as the Fortran expression is
  const double xmax = grid->xmax, ymax = grid->ymax, zmax = grid->zmax;
  const double f = (2.0 * xmax * 2.0 * ymax * 2.0 * zmax) /
                   ((double)nphotons * (2.0 * xmax / grid->nx) * (2.0 * ymax / grid->ny) * (2.0 * zmax / grid->nz));
  const int64_t nv = (int64_t)grid->nx * grid->ny * grid->nz;
  for (int64_t i = 0; i < nv; ++i) g[i] = (float)((double)g[i] * f);
  return SMCRT_OK;
}

}  // extern "C"
