// sceneplan.cpp — the knob readers, plan_scene and the pure launch rules (sceneplan.h).
// Host code only: no HIP runtime call, no kernel object.
#include "sceneplan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>

#include "dispexpr.h"
#include "hosterr.h"

namespace smcrt {
namespace {

int fail(int code, const std::string& msg) { return set_error(code, msg); }
bool is(const char* v, const char* s) { return v && std::strcmp(v, s) == 0; }

}  // namespace

Knobs read_knobs() {
  Knobs k;
  auto num = [](const char* v, double d) { return v ? std::atof(v) : d; };
  if (const char* cm = std::getenv("SMCRT_COOP_MIN_TOPS")) k.coop_min_tops = std::max(1, std::atoi(cm));
  if (const char* cl = std::getenv("SMCRT_COOP_LANES")) k.coop_lanes = std::max(1, std::min(64, std::atoi(cl)));
  k.coop_tab = !is(std::getenv("SMCRT_COOP_TAB"), "0");
  k.cull = !is(std::getenv("SMCRT_CULL"), "0");
  k.cull_grid.cells_per_top = num(std::getenv("SMCRT_CULL_CPT"), 512.0);
  k.cull_grid.max_cells = num(std::getenv("SMCRT_CULL_MAX_CELLS"), 1 << 18);
  k.cull_grid.max_list = (int32_t)num(std::getenv("SMCRT_CULL_MAX_LIST"), 64);
  k.cull_grid.k_nearest = (int32_t)num(std::getenv("SMCRT_CULL_K"), 8);
  k.cull_grid.u_frac = num(std::getenv("SMCRT_CULL_UFRAC"), 1.0);
  k.cull_log = std::getenv("SMCRT_CULL_LOG") != nullptr;
  k.far_march = !is(std::getenv("SMCRT_FAR_MARCH"), "0");
  const char* dm = std::getenv("SMCRT_DEPOSIT");
  k.deposit_atomic = is(dm, "atomic");
  k.deposit_sorted = is(dm, "sorted");
  if (const char* pc = std::getenv("SMCRT_POOL_CAP"))
    k.pool_cap_chunks = std::max<uint64_t>(1, std::strtoull(pc, nullptr, 10) / CHUNK_RECORDS);
  const char* fp = std::getenv("SMCRT_FOLD_PRIO");
  k.fold_prio = !(fp && fp[0] == '0');
  k.fused_hist = !is(std::getenv("SMCRT_FUSED_HIST"), "0");
  const char* wsl = std::getenv("SMCRT_WS_SLOTS");
  k.ws_two_slots = wsl && wsl[0] == '2';
  const char* wi = std::getenv("SMCRT_WS_INVOXEL");
  k.ws_invoxel = wi ? (is(wi, "0") ? 0 : 1) : -1;
  const char* le = std::getenv("SMCRT_LEAN");
  k.lean_mode = le ? (is(le, "0") ? 0 : 1) : -1;
  const char* lm = std::getenv("SMCRT_DEBUG_LEAN_MARGIN");
  k.lean_debug = is(lm, "all") ? 2u : (is(lm, "0") ? 1u : 0u);
  k.verbose = std::getenv("SMCRT_VERBOSE") != nullptr;
  return k;
}

LaunchKnobs read_launch_knobs() {
  LaunchKnobs k;
#ifdef SMCRT_DIAG
  const char* dd = std::getenv("SMCRT_DIAG_DONE");
  k.diag_done = dd && dd[0] == '1';
#endif
  if (const char* wm = std::getenv("SMCRT_WATCHDOG_MS")) k.watchdog_ms = std::strtod(wm, nullptr);
  if (const char* cd = std::getenv("SMCRT_DEBUG_CLAIM_DELAY")) k.claim_delay = (uint32_t)std::strtoul(cd, nullptr, 10);
  const char* de = std::getenv("SMCRT_DEBUG_DROP_EVENT");
  k.drop_event = de && de[0] == '1';
  const char* el = std::getenv("SMCRT_DEBUG_EVAL_LOOP");
  k.eval_loop = el && el[0] == '1';
  if (const char* pv = std::getenv("SMCRT_PATH_VERTICES")) k.path_vertices = (int32_t)std::strtol(pv, nullptr, 10);
  if (const char* pm = std::getenv("SMCRT_PATH_MAX")) k.path_max = (int64_t)std::strtoll(pm, nullptr, 10);
  return k;
}

void job_path_knobs(int32_t* max_vertices, int64_t* max_paths) {
  const LaunchKnobs k = read_launch_knobs();
  *max_vertices = k.path_vertices;
  *max_paths = k.path_max;
}

PoolKnobs read_pool_knobs() {
  PoolKnobs k;
  if (const char* ns = std::getenv("SMCRT_SLOTS")) k.slots = std::max(2, std::min(MAX_SLOTS, std::atoi(ns)));
  if (const char* dg = std::getenv("SMCRT_DEEP_SLOT_GIB")) {
    k.deep_set = true;
    k.deep_bytes = (uint64_t)std::strtoull(dg, nullptr, 10) << 30;
  }
  return k;
}

bool pool_log_knob() {
  static const bool on = std::getenv("SMCRT_POOL_LOG") != nullptr;  // diagnostics
  return on;
}

TopProps make_props(const smcrt_sdf_node& nd) {
  TopProps p;
  p.kappa = nd.mus + nd.mua;
  if (nd.flags & SMCRT_NODE_ALBEDO_UNGUARDED) p.albedo = nd.mus / p.kappa;  // updateSpectral :198-199
  else p.albedo = (nd.mua < 1e-9) ? 1.0 : nd.mus / p.kappa;
  p.hgg = nd.hgg;
  p.n = nd.n;
  return p;
}

namespace {

int validate(const smcrt_sdf_node* nodes, int32_t n_nodes, const int32_t* top, int32_t n_top, const smcrt_grid* grid,
             const smcrt_detector* dets, int32_t n_dets) {
  if (!nodes || n_nodes < 1 || !top || n_top < 1 || !grid || n_dets < 0 || (n_dets > 0 && !dets))
    return fail(SMCRT_ERR_INVALID_ARG, "bad scene arguments");
  if (grid->nx < 1 || grid->ny < 1 || grid->nz < 1 || !(grid->xmax > 0) || !(grid->ymax > 0) ||
      !(grid->zmax > 0))
    return fail(SMCRT_ERR_INVALID_ARG, "grid dimensions must be positive");
  if ((uint64_t)grid->nx * (uint64_t)grid->ny * (uint64_t)grid->nz >= (1ull << 32))
    return fail(SMCRT_ERR_UNSUPPORTED, "grids of 2^32 or more voxels are not supported");
  for (int32_t i = 0; i < n_nodes; ++i) {
    const smcrt_sdf_node& nd = nodes[i];
    if (nd.kind < SMCRT_SDF_SPHERE || nd.kind > SMCRT_SDF_DISPLACEMENT)
      return fail(SMCRT_ERR_INVALID_ARG, "node " + std::to_string(i) + ": unknown SDF kind");
    if (nd.kind == SMCRT_SDF_MODEL) {
      if (nd.n_children < 1 || nd.first_child < 0 || nd.first_child + nd.n_children > n_nodes)
        return fail(SMCRT_ERR_INVALID_ARG, "model node " + std::to_string(i) + ": bad child range");
      if (nd.op < SMCRT_OP_UNION || nd.op > SMCRT_OP_INTERSECTION)
        return fail(SMCRT_ERR_INVALID_ARG, "model node " + std::to_string(i) + ": bad CSG op");
    } else if (composite_kind(nd.kind)) {  // a modifier wraps exactly one node
      if (nd.n_children != 1 || nd.first_child < 0 || nd.first_child >= n_nodes)
        return fail(SMCRT_ERR_INVALID_ARG, "modifier node " + std::to_string(i) + ": needs exactly one child");
      if (nd.kind == SMCRT_SDF_DISPLACEMENT && nd.param[0] == (double)SMCRT_DISP_EXPR) {
        std::string why;  // the stored program, before the device interprets it (dispexpr.h)
        if (!disp_expr_verify(nd, &why))
          return fail(SMCRT_ERR_INVALID_ARG, "displacement node " + std::to_string(i) + ": bad expression program: " + why);
      } else if (nd.kind == SMCRT_SDF_DISPLACEMENT && nd.param[0] != (double)SMCRT_DISP_SINE) {
        return fail(SMCRT_ERR_INVALID_ARG, "displacement node " + std::to_string(i) + ": unknown function");
      }
    }
  }
  // models and modifiers nested at most PROG_MAX_DEPTH levels (geometry.h node_value); this
  // also rejects a composite that contains itself
  std::function<int(int32_t, int)> depth_ok = [&](int32_t idx, int lvl) -> int {
    const smcrt_sdf_node& nd = nodes[idx];
    if (!composite_kind(nd.kind)) return 1;
    if (lvl >= PROG_MAX_DEPTH) return 0;
    for (int32_t c = 0; c < nd.n_children; ++c)
      if (!depth_ok(nd.first_child + c, lvl + 1)) return 0;
    return 1;
  };
  for (int32_t i = 0; i < n_top; ++i)
    if (top[i] >= 0 && top[i] < n_nodes && !depth_ok(top[i], 0))
      return fail(SMCRT_ERR_UNSUPPORTED, "top " + std::to_string(i) + ": models/modifiers nested more than " +
                                             std::to_string(PROG_MAX_DEPTH) + " levels deep are not supported");
  for (int32_t i = 0; i < n_top; ++i)
    if (top[i] < 0 || top[i] >= n_nodes) return fail(SMCRT_ERR_INVALID_ARG, "top index out of range");
  for (int32_t i = 0; i < n_dets; ++i) {
    if (dets[i].kind < SMCRT_DET_CIRCLE || dets[i].kind > SMCRT_DET_FIBRE || dets[i].nbins < 1)
      return fail(SMCRT_ERR_INVALID_ARG, "bad detector " + std::to_string(i));
  }
  return SMCRT_OK;
}

bool translate_only(const smcrt_sdf_node& nd) {  // 3x3 part of the column-major transform is I
  const double* t = nd.transform;
  return t[0] == 1.0 && t[1] == 0.0 && t[2] == 0.0 && t[4] == 0.0 && t[5] == 1.0 && t[6] == 0.0 &&
         t[8] == 0.0 && t[9] == 0.0 && t[10] == 1.0;
}

// flatten the SDF array into one evaluation program (eval_model fold order)
void flatten(const smcrt_sdf_node* nodes, const int32_t* top, int32_t n_top, ScenePlan& p) {
  std::vector<ProgOp>& prog = p.prog;
  p.top_first.assign((size_t)n_top + 1, 0);
  for (int32_t i = 0; i < n_top; ++i) {
    const smcrt_sdf_node& nd = nodes[top[i]];
    p.top_first[i] = (int32_t)prog.size();
    if (!composite_kind(nd.kind)) {
      prog.push_back(ProgOp{top[i], PROG_TOP, i + 1, 0, 0.0, translate_only(nd), 0});
    } else if (nd.kind != SMCRT_SDF_MODEL) {  // a top-level modifier: one PROG_SUB op (geometry.h node_value)
      prog.push_back(ProgOp{top[i], PROG_TOP | PROG_SUB, i + 1, 0, 0.0, 0, 0});
    } else {
      // eval_model's left fold, children in order; a child model or modifier is one PROG_SUB
      // op (geometry.h node_value)
      for (int32_t c = 0; c < nd.n_children; ++c) {
        const int32_t ci = nd.first_child + c;
        const bool sub = composite_kind(nodes[ci].kind);
        prog.push_back(ProgOp{ci, (c == 0 ? PROG_CHILD_FIRST : PROG_CHILD) | (sub ? PROG_SUB : 0),
                              c == nd.n_children - 1 ? i + 1 : 0, nd.op, nd.k, sub ? 0 : translate_only(nodes[ci]), 0});
      }
    }
  }
  p.n_prog = (int)prog.size();
  p.top_first[n_top] = p.n_prog;
  for (int32_t i = 0; i <= n_top; ++i)  // eval_sdfs_coop's table of each top's first op
    prog.push_back(ProgOp{p.top_first[i], PROG_TOP, 0, 0, 0.0, 0, 0});
  for (const ProgOp& op : prog) p.nested = p.nested || (op.action & PROG_SUB) != 0;
}

// The far-field march and glance (far.h) need every top 1-Lipschitz (exact-distance
// primitives under translation-only transforms), a full EVAL that yields a certificate (the
// cooperative LDS table or the culled EVAL) and a bound on the computed values' error: a few
// ulps of the largest operand, taken here as 2^-44 of the scene's extent.
void plan_far_march(const smcrt_sdf_node* nodes, const int32_t* top, int32_t n_top, const smcrt_grid* grid, bool fm,
                    ScenePlan& p) {
  double ext = grid->xmax + grid->ymax + grid->zmax + 1.0;
  double scale = 0.0;
  // A top qualifies if it is such a primitive, or (round 4) a model of qualifying children
  // folded with union, intersection, subtraction or smooth union (min/max of 1-Lipschitz
  // values is 1-Lipschitz, and so is the polynomial smooth minimum: its partials are 1 - h^2/2
  // and h^2/2), at most 4 model levels deep so the fold's few roundings per level stay far
  // below the bound. The near top of a certificate is still a lone sphere or box (far.h).
  // m accumulates the operand magnitudes the error bound scales with.
  std::function<bool(int32_t, int, double&)> far_ok = [&](int32_t idx, int lvl, double& m) -> bool {
    const smcrt_sdf_node& nd = nodes[idx];
    if (nd.kind == SMCRT_SDF_MODEL) {
      const bool op_ok = nd.op == SMCRT_OP_UNION || nd.op == SMCRT_OP_INTERSECTION || nd.op == SMCRT_OP_SUBTRACTION ||
                         (nd.op == SMCRT_OP_SMOOTH_UNION && nd.k > 0.0 && std::isfinite(nd.k));
      if (lvl >= 4 || !op_ok || nd.n_children < 1) return false;
      if (nd.op == SMCRT_OP_SMOOTH_UNION) m = std::max(m, nd.k);
      for (int32_t c = 0; c < nd.n_children; ++c)
        if (!far_ok(nd.first_child + c, lvl + 1, m)) return false;
      return true;
    }
    const int32_t kd = nd.kind;
    if (!translate_only(nd) || !(kd == SMCRT_SDF_SPHERE || kd == SMCRT_SDF_BOX || kd == SMCRT_SDF_TORUS ||
                                 kd == SMCRT_SDF_SEGMENT || kd == SMCRT_SDF_CAPSULE))
      return false;
    double mm = std::fabs(nd.transform[3]) + std::fabs(nd.transform[7]) + std::fabs(nd.transform[11]);
    for (int r = 0; r < 8; ++r) mm += std::fabs(nd.param[r]);
    if (!std::isfinite(mm)) return false;
    m = std::max(m, mm);
    return true;
  };
  for (int32_t i = 0; fm && i < n_top; ++i) {
    double m = 0.0;
    fm = far_ok(top[i], 0, m);
    scale = std::max(scale, m);
  }
  fm = fm && std::isfinite(ext);
  if (fm) {
    p.fm_err = std::ldexp(scale + ext, -44);
    p.fm_step = std::ldexp(scale + ext, -48);
  }
}

// detector data offsets (a camera owns nbins^2 doubles)
void plan_detectors(const smcrt_detector* dets, int32_t n_dets, ScenePlan& p) {
  p.h_dets.assign(dets, dets + n_dets);
  p.h_det_off.assign((size_t)n_dets + 1, 0);
  for (int32_t i = 0; i < n_dets; ++i) {
    const int64_t nb = dets[i].nbins;
    p.h_det_off[i + 1] = p.h_det_off[i] + (dets[i].kind == SMCRT_DET_CAMERA ? nb * nb : nb);
  }
  p.det_total = p.h_det_off[n_dets];
}

// voxel faces, grid.f90:147-157: (i-1)*2*max/n; zface has nz+2 entries
void plan_faces(const smcrt_grid* grid, ScenePlan& p) {
  for (int32_t i = 0; i < grid->nx + 1; ++i) p.faces.push_back((double)i * 2.0 * grid->xmax / (double)grid->nx);
  for (int32_t i = 0; i < grid->ny + 1; ++i) p.faces.push_back((double)i * 2.0 * grid->ymax / (double)grid->ny);
  for (int32_t i = 0; i < grid->nz + 2; ++i) p.faces.push_back((double)i * 2.0 * grid->zmax / (double)grid->nz);
}

// inv2, fe and the kernels' grid mode
void plan_grid_mode(const smcrt_grid* grid, ScenePlan& p) {
  const double maxes[3] = {grid->xmax, grid->ymax, grid->zmax};
  // n*p/(2*max) may be computed as n*p*inv exactly when 2*max is a power of two
  for (int a = 0; a < 3; ++a) {
    int ex = 0;
    const double m = std::frexp(2.0 * maxes[a], &ex);
    p.inv2[a] = (m == 0.5 && std::isfinite(1.0 / (2.0 * maxes[a]))) ? 1.0 / (2.0 * maxes[a]) : 0.0;
  }
  const bool p2 = p.inv2[0] != 0.0 && p.inv2[1] != 0.0 && p.inv2[2] != 0.0;
  const int32_t ns[3] = {grid->nx, grid->ny, grid->nz};
  bool f2 = p2;
  for (int a = 0; a < 3; ++a) {
    if ((ns[a] & (ns[a] - 1)) != 0) { f2 = false; continue; }
    int e2m = 0, en = 0;  // 2*max = 2^(e2m-1), n = 2^(en-1)
    (void)std::frexp(2.0 * maxes[a], &e2m);
    (void)std::frexp((double)ns[a], &en);
    p.fe[a] = e2m - en;  // face k = k * 2*max/n = k * 2^fe
  }
  p.grid_mode = f2 ? 2 : (p2 ? 1 : 0);
}

// binned deposition (deposit.h); SMCRT_DEPOSIT=sorted (or a disabled fused histogram) keeps the sorted record path
void plan_deposit(const smcrt_grid* grid, const Knobs& knobs, ScenePlan& p) {
  const uint64_t nv = (uint64_t)grid->nx * grid->ny * grid->nz;
  const uint64_t tiles = (nv + TILE_VOXELS - 1) / TILE_VOXELS;
  p.n_tiles = (tiles <= MAX_TILES && nv < 0xFFFFFFFFull) ? (uint32_t)tiles : 0;
  p.force_atomic = knobs.deposit_atomic;
  p.pool_cap_chunks = knobs.pool_cap_chunks;
  const bool sorted = knobs.deposit_sorted || !knobs.fused_hist;
  p.bucketed = !sorted && p.n_tiles > 0 && p.n_tiles <= MAX_DIRECT_TILES;
  p.hist_tiles = (!p.bucketed && knobs.fused_hist && p.n_tiles > 0 && p.n_tiles <= MAX_FUSED_HIST_TILES) ? p.n_tiles : 0;
}

// the media checks of both label volumes and meshes; `kind` opens the message
int check_media(const char* kind, const smcrt_medium* media, int32_t n_media) {
  const std::string k = std::string(kind) + ": medium ";
  for (int32_t i = 0; i < n_media; ++i) {
    const smcrt_medium& m = media[i];
    if (!(m.mus >= 0.0) || !(m.mua >= 0.0) || !std::isfinite(m.mus) || !std::isfinite(m.mua))
      return fail(SMCRT_ERR_INVALID_ARG, k + std::to_string(i) + ": mus and mua must be finite and >= 0");
    if (!(std::fabs(m.hgg) <= 1.0)) return fail(SMCRT_ERR_INVALID_ARG, k + std::to_string(i) + ": |hgg| must be <= 1");
    if (!(m.n > 0.0) || !std::isfinite(m.n))
      return fail(SMCRT_ERR_INVALID_ARG, k + std::to_string(i) + ": n must be finite and > 0");
  }
  return SMCRT_OK;
}

// a placeholder node per medium carries its mus, mua, hgg, n (voxel and mesh scenes)
void plan_media(const smcrt_medium* media, int32_t n_media, ScenePlan& p) {
  p.n_nodes = p.n_top = n_media;
  for (int32_t i = 0; i < n_media; ++i) {
    smcrt_sdf_node nd;
    std::memset(&nd, 0, sizeof nd);
    nd.layer = i + 1;
    nd.mus = media[i].mus; nd.mua = media[i].mua; nd.hgg = media[i].hgg; nd.n = media[i].n;
    p.h_nodes.push_back(nd);
    p.h_top.push_back(i);
    p.h_props.push_back(make_props(nd));
  }
}

}  // namespace

int plan_scene(const smcrt_sdf_node* nodes, int32_t n_nodes, const int32_t* top, int32_t n_top, const smcrt_grid* grid,
               const smcrt_detector* dets, int32_t n_dets, const Knobs& knobs, const PlanLimits& lim, ScenePlan* out) {
  if (const int st = validate(nodes, n_nodes, top, n_top, grid, dets, n_dets)) return st;
  ScenePlan& p = *out;
  p.n_nodes = n_nodes;
  p.n_top = n_top;
  p.n_dets = n_dets;
  p.grid = *grid;
  p.h_nodes.assign(nodes, nodes + n_nodes);
  p.h_top.assign(top, top + n_top);
  for (int32_t i = 0; i < n_top; ++i) p.h_props.push_back(make_props(nodes[top[i]]));
  plan_detectors(dets, n_dets, p);
  plan_faces(grid, p);
  flatten(nodes, top, n_top, p);
  // A sparse wave evaluates its lanes' SDF arrays one lane at a time across the wave when
  // that is cheaper than the serial per-lane chain over all n_top tops (transport.h).
  p.coop_lanes = n_top >= knobs.coop_min_tops ? std::max(1, std::min(16, n_top / ((n_top + 63) / 64 + 3))) : 0;
  if (knobs.coop_lanes && p.coop_lanes > 0) p.coop_lanes = knobs.coop_lanes;
  {  // The cooperative EVAL's LDS table: at most 64 tops, none of them a model (transport.h).
    bool ok = p.coop_lanes > 0 && n_top <= 64 && knobs.coop_tab;
    for (int32_t i = 0; ok && i < n_top; ++i) ok = !composite_kind(nodes[top[i]].kind);
    if (ok) {
      p.ctab.assign(CTAB_DOUBLES, 0.0);
      for (int32_t i = 0; i < n_top; ++i) {
        const smcrt_sdf_node& nd = nodes[top[i]];
        for (int r = 0; r < 12; ++r) p.ctab[r * 64 + i] = nd.transform[r];
        for (int r = 0; r < 8; ++r) p.ctab[(12 + r) * 64 + i] = nd.param[r];
        p.ctab[20 * 64 + i] = (double)nd.kind + (translate_only(nd) ? 16.0 : 0.0);
      }
    }
  }
  const double maxes[3] = {grid->xmax, grid->ymax, grid->zmax};
  // exact culling of the SDF array for many-top scenes (cull.h)
  if (p.coop_lanes > 0 && knobs.cull) p.cull = build_cull(nodes, n_nodes, top, n_top, maxes, knobs.cull_grid);
  if (!p.ctab.empty() || p.cull.enabled) plan_far_march(nodes, top, n_top, grid, knobs.far_march, p);
  plan_grid_mode(grid, p);
  plan_deposit(grid, knobs, p);
  p.face_bytes = p.faces.size() * sizeof(double) + sizeof(TopProps) * (size_t)n_top;
  p.lds_faces = p.face_bytes <= MAX_FACE_BYTES;
  for (int32_t i = 1; i < n_top; ++i) p.fresnel = p.fresnel || p.h_props[i].n != p.h_props[0].n;
  {  // the lean path (ws.h): scenes with a few tops
    bool ok = p.bucketed && p.coop_lanes == 0 && grid->nx < (1 << 20) - 2 && grid->ny < (1 << 20) - 2 &&
              grid->nz < (1 << 20) - 2;
    // three segment slots per photon when their LDS fits beside the tile words and faces, else
    // two (SMCRT_WS_SLOTS=2 forces two)
    p.ws_slots = (!knobs.ws_two_slots && lean_lds(p) + lim.ws_shared3 <= LDS_BYTES) ? 3 : 2;
    ok = ok && lean_lds(p) + (p.ws_slots == 3 ? lim.ws_shared3 : lim.ws_shared2) <= LDS_BYTES;
    p.lean_mode = knobs.lean_mode;
    // Scenes with detectors take the lean path only when forced (SMCRT_LEAN=1): record_hits at
    // every segment end keeps their photon waves the bottleneck, and transport_kernel measured
    // faster on M5 (43.0 vs 30.3-31.1 M photons/s). Fresnel scenes take it (reflect_refract runs
    // in the event waves): M3 169.2-169.8 vs 144.0-144.3 (profiles/r05_ws/ab_m3_m5_fresnel_events.txt)
    p.lean_candidate = ok && !p.nested && (p.lean_mode == 1 || (p.lean_mode != 0 && n_dets == 0));
    p.lean_debug = knobs.lean_debug;
    p.ws_invoxel = knobs.ws_invoxel;
  }
  p.fold_prio = knobs.fold_prio;
  p.cull_log = knobs.cull_log;
  p.verbose = knobs.verbose;
  return SMCRT_OK;
}

int plan_voxel_scene(const uint8_t* labels, const smcrt_medium* media, int32_t n_media, const smcrt_grid* grid,
                     const smcrt_detector* dets, int32_t n_dets, const Knobs& knobs, ScenePlan* out) {
  if (!labels || !media || !grid || n_dets < 0 || (n_dets > 0 && !dets))
    return fail(SMCRT_ERR_INVALID_ARG, "voxel scene: NULL argument");
  if (n_media < 1 || n_media > 256)
    return fail(SMCRT_ERR_INVALID_ARG, "voxel scene: n_media = " + std::to_string(n_media) + " is outside 1 .. 256");
  if (grid->nx < 1 || grid->ny < 1 || grid->nz < 1 || !(grid->xmax > 0) || !(grid->ymax > 0) || !(grid->zmax > 0) ||
      !std::isfinite(grid->xmax) || !std::isfinite(grid->ymax) || !std::isfinite(grid->zmax))
    return fail(SMCRT_ERR_INVALID_ARG, "voxel scene: grid dimensions must be positive and finite");
  const uint64_t nv = (uint64_t)grid->nx * (uint64_t)grid->ny * (uint64_t)grid->nz;
  if (nv >= (1ull << 32)) return fail(SMCRT_ERR_UNSUPPORTED, "grids of 2^32 or more voxels are not supported");
  if (const int mst = check_media("voxel scene", media, n_media)) return mst;
  for (uint64_t v = 0; v < nv; ++v)
    if (labels[v] >= n_media) {
      const uint64_t i = v % (uint64_t)grid->nx, j = (v / (uint64_t)grid->nx) % (uint64_t)grid->ny,
                     k = v / ((uint64_t)grid->nx * (uint64_t)grid->ny);
      return fail(SMCRT_ERR_INVALID_ARG, "voxel scene: label " + std::to_string((int)labels[v]) + " of voxel (" +
                                             std::to_string(i) + ", " + std::to_string(j) + ", " + std::to_string(k) +
                                             ") (0-based, linear index " + std::to_string(v) + ") is not below n_media = " +
                                             std::to_string(n_media));
    }
  for (int32_t i = 0; i < n_dets; ++i)
    if (dets[i].kind < SMCRT_DET_CIRCLE || dets[i].kind > SMCRT_DET_FIBRE || dets[i].nbins < 1)
      return fail(SMCRT_ERR_INVALID_ARG, "bad detector " + std::to_string(i));
  ScenePlan& p = *out;
  p.voxel = true;
  p.n_dets = n_dets;
  p.grid = *grid;
  p.labels.assign(labels, labels + nv);
  plan_media(media, n_media, p);
  plan_detectors(dets, n_dets, p);
  plan_faces(grid, p);
  plan_grid_mode(grid, p);
  plan_deposit(grid, knobs, p);
  // voxel_kernel stages the media and the faces in LDS whatever their size
  p.face_bytes = p.faces.size() * sizeof(double) + sizeof(TopProps) * (size_t)n_media;
  p.lds_faces = true;
  if (p.face_bytes > MAX_FACE_BYTES)
    return fail(SMCRT_ERR_UNSUPPORTED, "voxel scene: nx + ny + nz is too large for the faces to be staged in LDS");
  for (int32_t i = 1; i < n_media; ++i) p.fresnel = p.fresnel || p.h_props[i].n != p.h_props[0].n;
  p.lean_mode = 0;
  p.lean_candidate = false;  // ws_kernel has no label walk
  p.fold_prio = knobs.fold_prio;
  p.verbose = knobs.verbose;
  return SMCRT_OK;
}

int32_t host_vox_of(double p, int32_t n, double max) {  // get_voxel_cart, grid.f90:51-78
  const double f = std::floor(((double)n * (p + max)) / (2.0 * max));
  if (!(f >= 0.0 && f < (double)n)) return -1;
  return (int32_t)f + 1;
}

// ---- mesh media ----------------------------------------------------------------------------
namespace {

struct MeshEdge {
  int32_t a, b;  // a < b
  int32_t tri;
  bool fwd;      // the triangle runs it a -> b
};

// Every undirected edge in exactly two triangles, once in each direction, both with the same pair
// of media. Names the offending edge with the smallest triangle index.
int check_closed(const int32_t* tris, const uint8_t* tri_media, int32_t nt) {
  std::vector<MeshEdge> edges;
  edges.reserve((size_t)3 * nt);
  for (int32_t t = 0; t < nt; ++t)
    for (int k = 0; k < 3; ++k) {
      const int32_t a = tris[3 * t + k], b = tris[3 * t + (k + 1) % 3];
      edges.push_back(a < b ? MeshEdge{a, b, t, true} : MeshEdge{b, a, t, false});
    }
  std::sort(edges.begin(), edges.end(), [](const MeshEdge& x, const MeshEdge& y) {
    return x.a != y.a ? x.a < y.a : (x.b != y.b ? x.b < y.b : x.tri < y.tri);
  });
  int32_t worst = -1;
  std::string msg;
  for (size_t i = 0; i < edges.size();) {
    size_t j = i;
    while (j < edges.size() && edges[j].a == edges[i].a && edges[j].b == edges[i].b) ++j;
    const MeshEdge& e = edges[i];  // (the group's smallest triangle index)
    std::string why;
    if (j - i != 2) {
      why = "occurs in " + std::to_string(j - i) + " triangle(s), not in exactly two: the surface is not closed";
    } else {
      const MeshEdge& f = edges[i + 1];
      if (e.fwd == f.fwd)
        why = "runs the same way in triangles " + std::to_string(e.tri) + " and " + std::to_string(f.tri) +
              ": the surface is not consistently oriented";
      else if (tri_media[2 * e.tri] != tri_media[2 * f.tri] || tri_media[2 * e.tri + 1] != tri_media[2 * f.tri + 1])
        why = "joins triangles " + std::to_string(e.tri) + " and " + std::to_string(f.tri) +
              ", which carry different (outside, inside) media";
    }
    if (!why.empty() && (worst < 0 || e.tri < worst)) {
      worst = e.tri;
      msg = "mesh scene: triangle " + std::to_string(e.tri) + ": edge (" + std::to_string(e.a) + ", " + std::to_string(e.b) +
            ") " + why;
    }
    i = j;
  }
  return worst < 0 ? SMCRT_OK : fail(SMCRT_ERR_INVALID_ARG, msg);
}

// The hierarchy over tris[b, e) (already in p.mesh_tris), depth-first; returns nothing, appends nodes.
void build_bvh(ScenePlan& p, std::vector<double>& cen, int32_t b, int32_t e, double pad) {
  const size_t self = p.mesh_nodes.size();
  p.mesh_nodes.push_back(MeshNode{});
  double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  double clo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, chi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  for (int32_t k = b; k < e; ++k) {
    const MeshTri& T = p.mesh_tris[k];
    for (int a = 0; a < 3; ++a) {
      // (the corners as v0 + e rounds them; the pad covers the rounding many times over)
      const double c[3] = {T.v0[a], T.v0[a] + T.e1[a], T.v0[a] + T.e2[a]};
      for (double x : c) { lo[a] = std::min(lo[a], x); hi[a] = std::max(hi[a], x); }
      clo[a] = std::min(clo[a], cen[3 * (size_t)T.id + a]);
      chi[a] = std::max(chi[a], cen[3 * (size_t)T.id + a]);
    }
  }
  {
    MeshNode& nd = p.mesh_nodes[self];
    for (int a = 0; a < 3; ++a) { nd.lo[a] = lo[a] - pad; nd.hi[a] = hi[a] + pad; }
    nd.first = b;
    nd.count = e - b <= MESH_LEAF_TRIS ? e - b : 0;
    nd.reserved = 0;
  }
  if (e - b > MESH_LEAF_TRIS) {
    int ax = 0;
    if (chi[1] - clo[1] > chi[ax] - clo[ax]) ax = 1;
    if (chi[2] - clo[2] > chi[ax] - clo[ax]) ax = 2;
    std::sort(p.mesh_tris.begin() + b, p.mesh_tris.begin() + e, [&](const MeshTri& x, const MeshTri& y) {
      const double cx = cen[3 * (size_t)x.id + ax], cy = cen[3 * (size_t)y.id + ax];
      return cx != cy ? cx < cy : x.id < y.id;
    });
    const int32_t mid = b + (e - b) / 2;
    build_bvh(p, cen, b, mid, pad);
    build_bvh(p, cen, mid, e, pad);
  }
  p.mesh_nodes[self].skip = (int32_t)p.mesh_nodes.size();  // the node after this subtree
}

}  // namespace

int plan_mesh_scene(const double* verts, int32_t nv, const int32_t* tris, const uint8_t* tri_media, int32_t nt,
                    const smcrt_medium* media, int32_t n_media, int32_t ambient, const smcrt_grid* grid,
                    const smcrt_detector* dets, int32_t n_dets, const Knobs& knobs, ScenePlan* out) {
  if (!verts || !tris || !tri_media || !media || !grid || n_dets < 0 || (n_dets > 0 && !dets))
    return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: NULL argument");
  if (n_media < 1 || n_media > 256)
    return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: n_media = " + std::to_string(n_media) + " is outside 1 .. 256");
  if (ambient < 0 || ambient >= n_media)
    return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: ambient = " + std::to_string(ambient) + " is not below n_media = " +
                                           std::to_string(n_media));
  if (nv < 4 || nt < 4)
    return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: nv = " + std::to_string(nv) + ", nt = " + std::to_string(nt) +
                                           ": a closed surface has at least 4 vertices and 4 triangles");
  if (nt > MESH_MAX_TRIS)
    return fail(SMCRT_ERR_UNSUPPORTED, "mesh scene: nt = " + std::to_string(nt) + " is above the " +
                                           std::to_string(MESH_MAX_TRIS) + " triangles that 32-bit node links allow");
  if (grid->nx < 1 || grid->ny < 1 || grid->nz < 1 || !(grid->xmax > 0) || !(grid->ymax > 0) || !(grid->zmax > 0) ||
      !std::isfinite(grid->xmax) || !std::isfinite(grid->ymax) || !std::isfinite(grid->zmax))
    return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: grid dimensions must be positive and finite");
  if ((uint64_t)grid->nx * (uint64_t)grid->ny * (uint64_t)grid->nz >= (1ull << 32))
    return fail(SMCRT_ERR_UNSUPPORTED, "grids of 2^32 or more voxels are not supported");
  if (const int mst = check_media("mesh scene", media, n_media)) return mst;
  double scale = std::max(grid->xmax, std::max(grid->ymax, grid->zmax));
  for (int64_t i = 0; i < (int64_t)3 * nv; ++i) {
    if (!std::isfinite(verts[i]))
      return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: vertex " + std::to_string(i / 3) + " is not finite");
    scale = std::max(scale, std::fabs(verts[i]));
  }
  for (int32_t t = 0; t < nt; ++t)
    for (int k = 0; k < 3; ++k)
      if (tris[3 * t + k] < 0 || tris[3 * t + k] >= nv)
        return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: triangle " + std::to_string(t) + ": vertex index " +
                                               std::to_string(tris[3 * t + k]) + " is outside 0 .. nv - 1 = " +
                                               std::to_string(nv - 1));
  for (int32_t t = 0; t < nt; ++t)
    for (int k = 0; k < 2; ++k)
      if (tri_media[2 * t + k] >= n_media)
        return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: triangle " + std::to_string(t) + ": medium index " +
                                               std::to_string((int)tri_media[2 * t + k]) + " is not below n_media = " +
                                               std::to_string(n_media));
  for (int32_t i = 0; i < n_dets; ++i)
    if (dets[i].kind < SMCRT_DET_CIRCLE || dets[i].kind > SMCRT_DET_FIBRE || dets[i].nbins < 1)
      return fail(SMCRT_ERR_INVALID_ARG, "bad detector " + std::to_string(i));
  ScenePlan& p = *out;
  p.mesh_tris.resize(nt);
  p.mesh_faces.resize(nt);
  std::vector<double> cen((size_t)3 * nt);
  for (int32_t t = 0; t < nt; ++t) {
    const double *v0 = verts + 3 * (size_t)tris[3 * t], *v1 = verts + 3 * (size_t)tris[3 * t + 1],
                 *v2 = verts + 3 * (size_t)tris[3 * t + 2];
    MeshTri& T = p.mesh_tris[t];
    for (int a = 0; a < 3; ++a) {
      T.v0[a] = v0[a];
      T.e1[a] = v1[a] - v0[a];
      T.e2[a] = v2[a] - v0[a];
      cen[3 * (size_t)t + a] = (v0[a] + v1[a] + v2[a]) / 3.0;
    }
    T.id = t;
    T.reserved = 0;
    // N = normalise(e1 x e2), with sqrt and / (exact under IEEE)
    const double cx = T.e1[1] * T.e2[2] - T.e1[2] * T.e2[1], cy = T.e1[2] * T.e2[0] - T.e1[0] * T.e2[2],
                 cz = T.e1[0] * T.e2[1] - T.e1[1] * T.e2[0];
    const double len = std::sqrt(cx * cx + cy * cy + cz * cz);
    if (len == 0.0 || !std::isfinite(len))
      return fail(SMCRT_ERR_INVALID_ARG, "mesh scene: triangle " + std::to_string(t) + " is degenerate (|e1 x e2| == 0)");
    MeshFace& F = p.mesh_faces[t];
    F.N[0] = cx / len; F.N[1] = cy / len; F.N[2] = cz / len;
    F.outside = tri_media[2 * t];
    F.inside = tri_media[2 * t + 1];
  }
  if (const int cst = check_closed(tris, tri_media, nt)) return cst;
  p.mesh = true;
  p.mesh_ambient = ambient;
  p.n_dets = n_dets;
  p.grid = *grid;
  p.mesh_nodes.reserve((size_t)nt);
  // boxes are padded by 2^-20 of the scene's size: the exact test's hit point lies in the unpadded
  // box up to the rounding of t, u, v, which the pad exceeds unless |det| is below ~1e-9 of its scale
  build_bvh(p, cen, 0, nt, scale * 0x1.0p-20);
  plan_media(media, n_media, p);
  plan_detectors(dets, n_dets, p);
  plan_faces(grid, p);
  plan_grid_mode(grid, p);
  plan_deposit(grid, knobs, p);
  // mesh_kernel stages the media and the faces in LDS whatever their size
  p.face_bytes = p.faces.size() * sizeof(double) + sizeof(TopProps) * (size_t)n_media;
  p.lds_faces = true;
  if (p.face_bytes > MAX_FACE_BYTES)
    return fail(SMCRT_ERR_UNSUPPORTED, "mesh scene: nx + ny + nz is too large for the faces to be staged in LDS");
  for (int32_t i = 1; i < n_media; ++i) p.fresnel = p.fresnel || p.h_props[i].n != p.h_props[0].n;
  p.lean_mode = 0;
  p.lean_candidate = false;  // ws_kernel has no cast
  p.fold_prio = knobs.fold_prio;
  p.verbose = knobs.verbose;
  return SMCRT_OK;
}

int32_t mesh_medium_at(const ScenePlan& p, const double pt[3]) {
  const double d[3] = {0.0, 0.0, 1.0};
  const MeshHit h = mesh_cast(p.mesh_nodes.data(), (uint32_t)p.mesh_nodes.size(), p.mesh_tris.data(), pt, d, MESH_NONE);
  if (h.tri == MESH_NONE) return p.mesh_ambient;
  const MeshFace& F = p.mesh_faces[h.tri];
  return (int32_t)((d[0] * F.N[0] + d[1] * F.N[1] + d[2] * F.N[2]) > 0.0 ? F.inside : F.outside);
}

int plan_screens(const smcrt_screen* screens, int32_t n, std::vector<ScreenDev>* out, int64_t* n_doubles) {
  if (!screens || !out || !n_doubles) return fail(SMCRT_ERR_INVALID_ARG, "screens: NULL argument");
  if (n < 1 || n > SCREEN_MAX)
    return fail(SMCRT_ERR_INVALID_ARG, "screens: " + std::to_string(n) + " screens (1 to " + std::to_string(SCREEN_MAX) + ")");
  out->clear();
  int64_t off = 0;
  for (int32_t i = 0; i < n; ++i) {
    const smcrt_screen& s = screens[i];
    const std::string who = "screen " + std::to_string(i) + ": ";
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(s.origin[a]) || !std::isfinite(s.eu[a]) || !std::isfinite(s.ev[a]))
        return fail(SMCRT_ERR_INVALID_ARG, who + "origin, eu and ev must be finite");
    const V3 eu = v3(s.eu[0], s.eu[1], s.eu[2]), ev = v3(s.ev[0], s.ev[1], s.ev[2]);
    const double uu = dot(eu, eu), vv = dot(ev, ev);
    if (!(uu > 0.0) || !(vv > 0.0) || !std::isfinite(uu) || !std::isfinite(vv))
      return fail(SMCRT_ERR_INVALID_ARG, who + "eu and ev must have a length above 0 (and a finite square)");
    if (!(std::fabs(dot(eu, ev)) <= 1e-12 * (std::sqrt(uu) * std::sqrt(vv))))
      return fail(SMCRT_ERR_INVALID_ARG, who + "eu and ev must be orthogonal (|eu . ev| <= 1e-12 |eu| |ev|)");
    if (s.nu < 1 || s.nu > SCREEN_MAX_PIXELS || s.nv < 1 || s.nv > SCREEN_MAX_PIXELS)
      return fail(SMCRT_ERR_INVALID_ARG, who + "nu and nv must be 1 to " + std::to_string(SCREEN_MAX_PIXELS));
    if (s.sides < -1 || s.sides > 1) return fail(SMCRT_ERR_INVALID_ARG, who + "sides must be -1, 0 or 1");
    if (s.reserved != 0) return fail(SMCRT_ERR_INVALID_ARG, who + "reserved must be 0");
    const V3 c = v3(eu.y * ev.z - eu.z * ev.y, eu.z * ev.x - eu.x * ev.z, eu.x * ev.y - eu.y * ev.x);
    const double lc = len(c);
    if (!(lc > 0.0) || !std::isfinite(lc))
      return fail(SMCRT_ERR_INVALID_ARG, who + "eu x ev must have a finite length above 0");
    ScreenDev d{};
    for (int a = 0; a < 3; ++a) { d.origin[a] = s.origin[a]; d.eu[a] = s.eu[a]; d.ev[a] = s.ev[a]; }
    d.N[0] = c.x / lc; d.N[1] = c.y / lc; d.N[2] = c.z / lc;
    d.uu = uu; d.vv = vv;
    d.nu = s.nu; d.nv = s.nv; d.sides = s.sides; d.reserved = 0;
    d.offset = (uint64_t)off;
    off += 2 * (int64_t)s.nu * (int64_t)s.nv;
    out->push_back(d);
  }
  *n_doubles = off;
  return SMCRT_OK;
}

int plan_volume_source(const double* w, int64_t nvox, std::vector<double>* cdf, int64_t* last, int64_t* n_positive,
                       int64_t* n_reachable) {
  if (!w || !cdf || !last || !n_positive || !n_reachable) return fail(SMCRT_ERR_INVALID_ARG, "volume source: NULL argument");
  if (nvox < 1 || nvox > 0xFFFFFFFFll)
    return fail(SMCRT_ERR_INVALID_ARG, "volume source: " + std::to_string(nvox) + " voxels (1 to 2^32 - 1)");
  for (int64_t i = 0; i < nvox; ++i) {
    if (!std::isfinite(w[i]))
      return fail(SMCRT_ERR_INVALID_ARG, "volume source: the weight of voxel " + std::to_string(i) + " is not finite");
    if (w[i] < 0.0)
      return fail(SMCRT_ERR_INVALID_ARG, "volume source: the weight of voxel " + std::to_string(i) + " is negative");
  }
  cdf->assign((size_t)nvox, 0.0);
  double run = 0.0;
  int64_t la = -1, np = 0, nr = 0;
  for (int64_t i = 0; i < nvox; ++i) {
    const double next = run + w[i];
    if (!std::isfinite(next))
      return fail(SMCRT_ERR_INVALID_ARG, "volume source: the sum of the weights overflows at voxel " + std::to_string(i));
    if (w[i] > 0.0) ++np;
    if (next > run) { ++nr; la = i; }
    run = next;
    (*cdf)[(size_t)i] = run;
  }
  if (la < 0)
    return fail(SMCRT_ERR_INVALID_ARG, "volume source: every weight is zero (voxel 0 .. " + std::to_string(nvox - 1) + ")");
  *last = la; *n_positive = np; *n_reachable = nr;
  return SMCRT_OK;
}

std::vector<double> grid_faces(const smcrt_grid* grid) {
  ScenePlan p;
  plan_faces(grid, p);
  return p.faces;
}

}  // namespace smcrt
