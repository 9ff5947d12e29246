// sceneplan.h — the engine's host policy without a device: the SMCRT_* knobs, the plan of a
// scene (validation, the flattened SDF program, the kernel instantiation and deposition path
// it gets) and the pure sizing rules of the record pool and of a launch.
//
// Nothing here makes a HIP runtime call or needs a kernel object: smcrt.hip reads the knobs,
// calls plan_scene and then only uploads the plan and owns the device state (devmem.h);
// tests/sceneplan_probe.cpp prints a plan on a machine without a GPU. Every value that
// reaches a kernel (fm_err, fm_step, inv2, fe, the faces, the lean margins, the cull grid)
// keeps the operations and their order that the kernels' bit-exact parity was measured with.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/smcrt.h"
#include "transport.h"  // (before deposit.h, which uses KParams)
#include "cull.h"
#include "deposit.h"
#include "launchchoice.h"

namespace smcrt {

// Record-log slots (and internal launch streams) per scene: launches whose pools are small
// enough run up to MAX_SLOTS deep, so long-tailed launches overlap more than pairwise.
constexpr int MAX_SLOTS = 4;
#ifndef SMCRT_DEEP_SLOT_GIB
#define SMCRT_DEEP_SLOT_GIB 24
#endif
constexpr uint64_t DEEP_SLOT_BYTES = (uint64_t)SMCRT_DEEP_SLOT_GIB << 30;  // a slot pool at most this large: MAX_SLOTS slots

// The words of smcrt_scene::d_queue: a work-queue head per launch stream, then the scene's
// running totals and the watchdog word (transport.h watchdog_expired).
enum QueueWord : int {
  Q_STREAM0 = 0,         // heads of the internal streams 0 .. MAX_SLOTS-1
  Q_CALLER = MAX_SLOTS,  // head of launches on the caller's stream
  Q_FAR_STEPS,           // far-field march steps (far.h)
  Q_FOLD_TICKS,          // bk_reduce workgroup run time, s_memrealtime ticks
  Q_LEAN_HAZARDS,        // deferred lean segments that ended in tflag or an error stop (lean.h)
  Q_WATCHDOG,            // the first expired wait: site | (block + 1) << 8
  Q_INVOXEL,             // segments deposited by ws_kernel's photon waves (invoxel.h)
  Q_OOO_HANDOUTS,        // ws_kernel hand-outs into a slot other than the next in rotation (ws.h)
  Q_COUNT
};
constexpr int N_QUEUES = Q_CALLER + 1;  // launch streams: each has a queue head, a KCold ring, a lane scratch

constexpr size_t LDS_BYTES = 163840;        // a workgroup's LDS ceiling (160 KiB)
constexpr size_t MAX_FACE_BYTES = 40960;    // props + voxel faces are staged in LDS up to this size
constexpr uint32_t MAX_FUSED_HIST_TILES = 512;  // 8 KiB of LDS per block for the wave histograms
// Record pool: record indices in the bin kernels are 32-bit, so at most 2^32 - 2^28 records
// (30 GiB, plus the same again for the sorted copy) per launch; a launch that would need more
// is split into sub-batches. POOL_SLACK covers the spread of records per photon between
// batches; a launch that still overflows folds the excess with atomics (exact, slower).
constexpr uint64_t MAX_POOL_RECORDS = (1ull << 32) - (1ull << 28);
constexpr double POOL_SLACK = 1.15;
constexpr double DEFAULT_WATCHDOG_MS = 2000.0;  // a wait past 2 s of wall clock is a lost wake-up

// ---- knobs: every SMCRT_* setting of smcrt.hip and cull.cpp, each read at one moment ----
struct Knobs {  // read_knobs(): at scene creation
  int32_t coop_min_tops = 8;  // SMCRT_COOP_MIN_TOPS: the fewest tops that get the COOP instantiation
  int32_t coop_lanes = 0;     // SMCRT_COOP_LANES (experiments: the sparse-wave threshold); 0 = the rule
  bool coop_tab = true;       // SMCRT_COOP_TAB=0 keeps the global-memory cooperative EVAL
  bool cull = true;           // SMCRT_CULL=0
  CullKnobs cull_grid;        // SMCRT_CULL_CPT / _MAX_CELLS / _MAX_LIST / _K / _UFRAC
  bool cull_log = false;      // SMCRT_CULL_LOG
  bool far_march = true;      // SMCRT_FAR_MARCH=0
  bool deposit_atomic = false, deposit_sorted = false;  // SMCRT_DEPOSIT=atomic / =sorted
  uint64_t pool_cap_chunks = 0;  // SMCRT_POOL_CAP (records; tests of pool exhaustion): 0 = none
  bool fold_prio = true;      // SMCRT_FOLD_PRIO=0: the fold stream at normal priority
  bool fused_hist = true;     // SMCRT_FUSED_HIST=0
  bool ws_two_slots = false;  // SMCRT_WS_SLOTS=2
  int ws_invoxel = -1;        // SMCRT_WS_INVOXEL: -1 automatic (on, but off for Fresnel/detector scenes), 0 off, 1 on
  int lean_mode = -1;         // SMCRT_LEAN: -1 automatic, 0 off, 1 forced
  uint32_t lean_debug = 0;    // SMCRT_DEBUG_LEAN_MARGIN (tests only): 1 = "0", 2 = "all"
  bool verbose = false;       // SMCRT_VERBOSE
};
struct LaunchKnobs {  // read_launch_knobs(): at every launch
  int32_t path_vertices = 64;  // SMCRT_PATH_VERTICES: smcrt_job_run's vertices per path (2 .. 1024)
  int64_t path_max = 65536;    // SMCRT_PATH_MAX: smcrt_job_run's arena slots (>= 1)
  double watchdog_ms = DEFAULT_WATCHDOG_MS;  // SMCRT_WATCHDOG_MS; 0: unbounded waits
  uint32_t claim_delay = 0;  // SMCRT_DEBUG_CLAIM_DELAY (tests only)
  bool drop_event = false;   // SMCRT_DEBUG_DROP_EVENT=1 (tests only: the watchdog's proof)
  bool eval_loop = false;    // SMCRT_DEBUG_EVAL_LOOP=1 (tests only: ws_kernel's EVAL takes no pairs)
  bool diag_done = false;    // SMCRT_DIAG_DONE=1 (diagnostic builds: completion times)
};
struct PoolKnobs {  // read_pool_knobs(): when the record pool is (re)allocated
  int slots = 0;            // SMCRT_SLOTS clamped to 2 .. MAX_SLOTS; 0 = the rule
  bool deep_set = false;    // SMCRT_DEEP_SLOT_GIB given
  uint64_t deep_bytes = 0;
};
Knobs read_knobs();
LaunchKnobs read_launch_knobs();
PoolKnobs read_pool_knobs();
bool pool_log_knob();  // SMCRT_POOL_LOG, read once

// ---- the plan ----
struct PlanLimits {
  size_t ws_shared2 = 0, ws_shared3 = 0;  // sizeof(WsSharedT<2>), sizeof(WsSharedT<3>): ws_kernel's static LDS
};

struct ScenePlan {
  int n_nodes = 0, n_top = 0, n_dets = 0;
  smcrt_grid grid{};
  int64_t det_total = 0;
  std::vector<smcrt_sdf_node> h_nodes;
  std::vector<int32_t> h_top;
  std::vector<TopProps> h_props;
  std::vector<smcrt_detector> h_dets;
  std::vector<int64_t> h_det_off;
  std::vector<double> faces;  // x (nx+1) | y (ny+1) | z (nz+2)
  // the SDF array flattened into one evaluation program (eval_model fold order), followed by
  // eval_sdfs_coop's table of each top's first op (n_top + 1 entries after the n_prog ops)
  std::vector<ProgOp> prog;
  std::vector<int32_t> top_first;
  int n_prog = 0;
  // a top model has a model or modifier among its children, or a top is a modifier: only the
  // general instantiation evaluates composites below the top level (geometry.h node_value), so
  // such scenes always run it: with many tops its COOP variant (cooperative and culled EVALs,
  // round 4), else the serial EVAL; never the lean kernel
  bool nested = false;
  int coop_lanes = 0;
  std::vector<double> ctab;  // the cooperative EVAL's primitive table (transport.h), or empty
  CullHost cull;             // exact SDF culling (cull.h): grid + lists + the always-evaluated tops
  // far-field march (far.h): KParams::fm_err / fm_step, 0 when the scene does not qualify
  double fm_err = 0.0, fm_step = 0.0;
  double inv2[3] = {0.0, 0.0, 0.0};
  int grid_mode = 0;  // transport_kernel<*, GM>: 1 = every 2*max a power of two, 2 = and every n too
  int32_t fe[3] = {0, 0, 0};
  uint32_t n_tiles = 0;          // binned jmean deposition (deposit.h); 0: the grid has too many tiles
  bool force_atomic = false;     // SMCRT_DEPOSIT=atomic
  uint64_t pool_cap_chunks = 0;  // SMCRT_POOL_CAP
  bool bucketed = false;    // records go straight into per-tile buckets (deposit.h); else sorted path
  uint32_t hist_tiles = 0;  // fused tile histogram in the transport kernel (0: bin_hist kernel)
  size_t face_bytes = 0;
  bool lds_faces = false;   // stage props + voxel faces in LDS when they fit
  bool fresnel = false;     // two tops with different refractive indices
  int ws_slots = 3;         // ws_kernel's segment slots per photon: 3, or 2 when 3 do not fit the LDS (ws.h)
  // SMCRT_LEAN. (Rounds 3-4 chose lean_kernel only up to 5.5 voxel crossings per segment: long
  // walks were cheaper in one lane. ws_kernel's walker waves take them at any length: M0, 8.2
  // crossings per segment, 54.9 vs 43.4-44.2 M photons/s on transport_kernel,
  // profiles/r05_ws/ab_m0.txt.)
  int lean_mode = -1;
  uint32_t lean_debug = 0;
  int ws_invoxel = -1;     // SMCRT_WS_INVOXEL (-1 automatic, 0 off, 1 on; see ws_invoxel_on)
  // the lean path (ws_kernel) serves this scene: a few tops, bucketed deposition, axes below
  // 2^20 cells, its LDS fits (SMCRT_LEAN=0 keeps transport_kernel); the lane-scratch
  // allocation may still veto it (smcrt_scene::lean_ok)
  bool lean_candidate = false;
  bool fold_prio = true, cull_log = false, verbose = false;  // (knobs the device side acts on)
  // voxel media (plan_voxel_scene): the labels, x fastest; h_props are the media and h_nodes /
  // h_top hold one placeholder node per medium, so that the optical-property accessors serve both
  // kinds of scene
  bool voxel = false;
  std::vector<uint8_t> labels;
  // mesh media (plan_mesh_scene): the threaded hierarchy, the triangles in its order and the faces
  // by the caller's triangle index (meshcast.h); h_props, h_nodes and h_top hold the media as in a
  // voxel scene
  bool mesh = false;
  int32_t mesh_ambient = 0;
  std::vector<MeshNode> mesh_nodes;
  std::vector<MeshTri> mesh_tris;
  std::vector<MeshFace> mesh_faces;
};

// Validate the scene and decide everything about it that needs no device. Returns SMCRT_OK,
// or the status with its message in smcrt_last_error (hosterr.h).
int plan_scene(const smcrt_sdf_node* nodes, int32_t n_nodes, const int32_t* top, int32_t n_top, const smcrt_grid* grid,
               const smcrt_detector* dets, int32_t n_dets, const Knobs& knobs, const PlanLimits& lim, ScenePlan* out);

TopProps make_props(const smcrt_sdf_node& nd);  // init_mono, opticalProperties.f90:107-125

// A voxel scene (smcrt_voxel_scene_create): validates, and fills what a launch of voxel_kernel
// needs: grid mode, inv2 / fe, faces, the deposit regime, the media as props. No SDF logic, no
// lean path. Same return convention as plan_scene.
int plan_voxel_scene(const uint8_t* labels, const smcrt_medium* media, int32_t n_media, const smcrt_grid* grid,
                     const smcrt_detector* dets, int32_t n_dets, const Knobs& knobs, ScenePlan* out);
// The host's restatement of vox_of (transport.h) for smcrt_scene_classify on a voxel scene: the
// 1-based cell of centred coordinate p on an axis of n cells, -1 outside
int32_t host_vox_of(double p, int32_t n, double max);

// A mesh scene (smcrt_mesh_scene_create): validates (finite vertices, indices in range, no
// degenerate triangle, media, every surface closed and consistently oriented with one pair of
// media along each edge), builds the hierarchy (median split of the centroids on the longest axis,
// leaves of at most MESH_LEAF_TRIS triangles, depth-first order, padded boxes) and fills what a
// launch of mesh_kernel needs, as plan_voxel_scene does. Surfaces that intersect each other are
// not detected. Same return convention as plan_scene.
int plan_mesh_scene(const double* verts, int32_t nv, const int32_t* tris, const uint8_t* tri_media, int32_t nt,
                    const smcrt_medium* media, int32_t n_media, int32_t ambient, const smcrt_grid* grid,
                    const smcrt_detector* dets, int32_t n_dets, const Knobs& knobs, ScenePlan* out);
// The medium (0-based) of centred point p of a mesh plan: a host cast along (0, 0, 1) and the
// emission rule (inside(tri) if dir . N > 0 at the hit, outside(tri) if not, ambient without a hit)
int32_t mesh_medium_at(const ScenePlan& p, const double pt[3]);

// Field screens (smcrt_scene_set_screens, smcrt_screen_hit): validates smcrt.h's list (1 <= n <= 16,
// finite numbers, non-zero orthogonal edges, 1 <= nu, nv <= 4096, sides, reserved), naming the
// first offending screen, and fills what the hit rule reads (screen.h): N, dot(eu, eu), dot(ev, ev)
// and each screen's offset in the field buffer; *n_doubles is the buffer's size. Same return
// convention as plan_scene.
int plan_screens(const smcrt_screen* screens, int32_t n, std::vector<ScreenDev>* out, int64_t* n_doubles);

// The volume source's table (smcrt_scene_set_volume_source, smcrt_volume_sample, smcrt_volume_pick;
// the rule reads it in volsrc.h): validates w[nvox] (1 <= nvox < 2^32; every weight finite and
// >= 0; not all zero; no running sum overflows), naming the first offending voxel index, and fills
// cdf[i] = cdf[i-1] + w[i], summed left to right. *last is the largest i with cdf[i] > cdf[i-1],
// *n_positive counts w[i] > 0 and *n_reachable cdf[i] > cdf[i-1]. Same return convention as
// plan_scene.
int plan_volume_source(const double* w, int64_t nvox, std::vector<double>* cdf, int64_t* last, int64_t* n_positive,
                       int64_t* n_reachable);

// The faces every scene of this grid has (ScenePlan::faces: x (nx+1) | y (ny+1) | z (nz+2)), for
// the scene-free smcrt_volume_sample.
std::vector<double> grid_faces(const smcrt_grid* grid);

// ---- pure rules of the launch path ----
// the lean path's dynamic LDS (ws_kernel): staged props + faces, then the block's bucket words
inline size_t lean_lds(const ScenePlan& p) {
  return (p.lds_faces ? p.face_bytes : 0) + (size_t)2 * p.n_tiles * sizeof(uint32_t);
}
// 32-bit LDS words of a block's deposit state (deposit.h): a tile histogram per wave, or one
// 64-bit bucket word per tile shared by the block.
inline uint32_t dep_words(const ScenePlan& p) { return p.bucketed ? 2 * p.n_tiles : 4 * p.hist_tiles; }
// Dynamic LDS of the transport kernel: staged props + faces, detector start points, then the
// deposit words, then the coop table.
// (`hist`: also the phasor tally's instantiations, which keep their faces there too)
// (`screens`: a phasor launch that tallies field screens keeps the start points whether or not the
// scene has detectors, and a fourth row: the phase there)
inline size_t transport_lds(const ScenePlan& p, uint32_t dep_words, bool xsrc, bool hist = false, bool screens = false) {
  const bool ctab = !p.ctab.empty() && p.coop_lanes > 0;  // the COOP instantiations stage it
  // (the general emitter with the COOP machinery and the path recorder keep their faces in
  // device memory, kernel_ptrs.h)
  const bool faces = p.lds_faces && !(xsrc && p.coop_lanes > 0) && !hist;
  const size_t start_rows = screens ? 4 : p.n_dets ? 3 : 0;
  return (faces ? p.face_bytes : 0) + start_rows * 256 * sizeof(double) +
         (size_t)dep_words * sizeof(uint32_t) + (ctab ? CTAB_DOUBLES * sizeof(double) : 0);
}
// Pool records that a launch of `blocks` transport blocks does not fill: per wave, the last
// chunk (sorted path); bucketed: per block and tile an open bucket and its pre-taken
// successor, per wave a batch of unused ids.
inline double pool_slack_records(const ScenePlan& p, int blocks) {
  const double waves = (double)blocks * 4.0;
  return p.bucketed ? (waves / 4.0 * 2.0 * p.n_tiles + waves * BUCKET_BATCH) * BUCKET_RECORDS
                    : waves * CHUNK_RECORDS;
}
// Records the record pool must hold for one launch of n photons at rpp records per photon.
inline uint64_t pool_records_for(const ScenePlan& p, int blocks, uint64_t n, double rpp) {
  const double want = (double)n * rpp * POOL_SLACK + pool_slack_records(p, blocks);
  return (uint64_t)std::min(want, (double)MAX_POOL_RECORDS);
}
// Record-log slots for pools of cap_bytes per slot: MAX_SLOTS while a slot is at most
// DEEP_SLOT_BYTES (or 60 % of the device's total_mem over MAX_SLOTS, if more;
// SMCRT_DEEP_SLOT_GIB overrides), larger pools two. Scenes of the lean kernel and of the
// far-field march keep two at any size; SMCRT_SLOTS overrides that choice.
inline int slot_depth(const PoolKnobs& k, bool lean_or_far, uint64_t cap_bytes, uint64_t total_mem) {
  const int want = k.slots ? k.slots : (lean_or_far ? 2 : MAX_SLOTS);
  uint64_t deep = std::max<uint64_t>(DEEP_SLOT_BYTES, (uint64_t)(0.6 * (double)total_mem) / MAX_SLOTS);
  if (k.deep_set) deep = k.deep_bytes;
  return cap_bytes <= deep ? want : 2;
}
// binned deposition needs path-length tallies into jmean with unit weights (fp32 record
// values are exact only then) and a grid of at most MAX_TILES tiles
inline bool launch_binned(const ScenePlan& p, bool has_jmean, uint32_t flags) {
  return has_jmean && (flags & SMCRT_FLAG_PATHLENGTH) && !(flags & SMCRT_FLAG_SURVIVAL_BIAS) && p.n_tiles > 0 &&
         !p.force_atomic;
}
// the lean path (ws_kernel, ws.h) when the scene and the run qualify: bucketed path-length
// deposition, unit weights (no survival bias), a plain source, no path tracking and no phasor
// tally (ws_kernel has neither)
inline bool launch_lean(bool lean_ok, bool xsrc, uint32_t bucket_tiles, uint32_t flags) {
  return !xsrc && lean_ok && bucket_tiles && (flags & SMCRT_FLAG_PATHLENGTH) &&
         !(flags & (SMCRT_FLAG_SURVIVAL_BIAS | SMCRT_FLAG_TRACK_PATHS | SMCRT_FLAG_PHASOR));
}
// ws_kernel's in-voxel segments (ws.h): on by default in the plain instantiation; the XF one
// (xf: Fresnel interfaces or detectors), which measured slower with them, only when asked for
inline bool ws_invoxel_on(int knob, bool xf) { return knob < 0 ? !xf : knob != 0; }
// XF: the scene has Fresnel interfaces or detectors (ws_kernel's instantiation with their program
// points, and the lane scratch that goes with it)
inline bool plan_xf(const ScenePlan& p) { return p.fresnel || p.n_dets > 0; }

// Partial path lengths (ppath.h): a scene of at most this many media can be tracked, and the LDS
// of a tracking launch after its deposit words: one double per medium and lane of the 256-thread block.
constexpr int32_t PPL_MAX_MEDIA = SMCRT_PPATH_MAX_MEDIA;
inline size_t ppl_lds_bytes(const ScenePlan& p) { return (size_t)p.n_top * 256 * sizeof(double); }
// the static LDS of voxel_kernel and mesh_kernel: their LaneCounters (transport.h)
constexpr size_t SDFLESS_STATIC_LDS = sizeof(LaneCounters);

// ---- the launch choice (launchchoice.h): which compiled kernel a launch runs, and with what LDS ----
// The choice for one launch of plan p: `xsrc` the general emitter, `bucket_tiles` the launch's
// KParams::bucket_tiles, `flags` the run's, and the scene state that matters: path tracking and
// the phasor tally configured, the number of field screens. (`lean_ok` false, or no bucket
// tiles, never gives ws_kernel: what a scene's transport_kernel grids are sized with.)
// `ppl_lds`: the bytes of LDS that partial path lengths are configured with on a voxel or a mesh
// scene (ppl_lds_bytes), 0 when they are not; a run with SMCRT_FLAG_PARTIAL_PATHS then takes the
// PPL instantiation and that much LDS after the deposit words.
inline LaunchChoice launch_choice(const ScenePlan& p, bool lean_ok, bool xsrc, uint32_t bucket_tiles, uint32_t flags,
                                  bool path_on, bool phasor_on, size_t n_screens, size_t ppl_lds = 0) {
  LaunchChoice c;
  c.gm = p.grid_mode;
  if (p.voxel || p.mesh) {  // (neither has a lean path, a path recorder or a phasor tally)
    c.family = p.mesh ? KF_MESH : KF_VOXEL;
    c.xsrc = xsrc;
    c.lds = p.face_bytes + (size_t)dep_words(p) * sizeof(uint32_t);  // (voxel.h, mesh.h: media + faces, then the deposit words)
    c.ppl = (flags & SMCRT_FLAG_PARTIAL_PATHS) && ppl_lds > 0;
    if (c.ppl) c.lds += ppl_lds;  // (ppath.h: then len[medium][lane])
  } else if (launch_lean(lean_ok, xsrc, bucket_tiles, flags)) {
    c.family = KF_WS;
    c.lds_faces = p.lds_faces;
    c.xf = plan_xf(p);
    c.slots = p.ws_slots;
    c.iv = ws_invoxel_on(p.ws_invoxel, c.xf);
    c.tk = (flags & SMCRT_FLAG_TEST_KERNEL) != 0;
    c.lds = lean_lds(p);
  } else {
    c.xsrc = xsrc;
    c.coop = p.coop_lanes > 0;  // (many tops: the cooperative tail EVAL and culling; it costs registers)
    c.hist = (flags & SMCRT_FLAG_TRACK_PATHS) && path_on;
    c.phas = (flags & SMCRT_FLAG_PHASOR) && phasor_on && !c.hist;  // (smcrt_run refuses the two together)
    c.scr = c.phas && n_screens > 0;
    // (the general emitter with the COOP machinery, the path recorder and the phasor tally are
    // instantiated with faces in device memory only: the library's build time; transport_lds follows)
    c.lds_faces = p.lds_faces && !((xsrc && c.coop) || c.hist || c.phas);
    c.lds = transport_lds(p, dep_words(p), xsrc, c.hist || c.phas, c.scr);
  }
  return c;
}
// lean_margin per axis (lean.h, ws.h), with the operations the kernel used to do
inline void lean_margins(uint32_t lean_debug, const smcrt_grid& g, double lo[3], double hi[3]) {
  const double eps = 1e-8, mf = (lean_debug & 3u) ? 0.0 : 2.0 * eps;
  const double mx = mf * (double)(g.nx + 2), my = mf * (double)(g.ny + 2), mz = mf * (double)(g.nz + 2);
  lo[0] = mx; lo[1] = my; lo[2] = mz;
  hi[0] = 2.0 * g.xmax - mx; hi[1] = 2.0 * g.ymax - my; hi[2] = 2.0 * g.zmax - mz;
}

}  // namespace smcrt
