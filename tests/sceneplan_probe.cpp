// sceneplan_probe.cpp — prints the engine's device-free decisions (rsmcrt_amd/csrc/sceneplan.h)
// as key=value lines, for tests/planprobe.py. Host code only: built from this file,
// sceneplan.cpp and cull.cpp; no kernel object, no libsmcrt.so, no GPU.
//
//   sceneplan_probe plan FILE   FILE: int32 n_nodes, n_top, n_dets | smcrt_sdf_node[n_nodes] |
//                               int32 top[n_top] | smcrt_grid | smcrt_detector[n_dets]
//   sceneplan_probe cull FILE OUT   the plan's culling grid (cull.h CullHost) into OUT: int32 enabled,
//                               n[3], n_always, pad | double lo[3], cell | uint64 sizes of off, list,
//                               elb, lb | uint32 off[] | uint32 list[] | float elb[] | double lb[] |
//                               int32 always[]
//   sceneplan_probe slots LEAN_OR_FAR CAP_BYTES TOTAL_MEM
//   sceneplan_probe choice FILE KIND (XSRC FLAGS LEAN_OK PATHS_ON PHASOR_ON N_SCREENS)...
//                               the launch choice (sceneplan.h launch_choice) of the plan of FILE for each
//                               run state, one block of lines from family= to grid_key= each; a launch that may deposit into buckets has the plan's tiles as its
//                               bucket_tiles (launch_binned, as smcrt.hip's launch() sets them). KIND sdf
//                               probes the plan as it is; voxel and mesh mark it as a voxel or a mesh plan
//                               after planning (the choice for those reads only p.voxel, p.mesh, grid_mode,
//                               face_bytes and the deposit words, so they need no file format of their own).
// The SMCRT_* knobs come from the environment, through the readers the library uses.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../rsmcrt_amd/csrc/hosterr.h"
#include "../rsmcrt_amd/csrc/kernels.h"  // WsSharedT (ws.h, in the order it needs)
#include "../rsmcrt_amd/csrc/sceneplan.h"

thread_local std::string smcrt::g_last_error;
using namespace smcrt;

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <class T>
static bool write_n(std::FILE* f, const T* v, size_t n) {
  return n == 0 || std::fwrite(v, sizeof(T), n, f) == n;
}

// the culling grid the kernels read (smcrt.hip upload_cull copies these arrays as they are)
static int dump_cull(const CullHost& H, const char* path) {
  std::FILE* f = std::fopen(path, "wb");
  if (!f) return 2;
  const int32_t head[6] = {(int32_t)H.enabled, H.n[0], H.n[1], H.n[2], (int32_t)H.always.size(), 0};
  const double geo[4] = {H.lo[0], H.lo[1], H.lo[2], H.cell};
  const uint64_t sizes[4] = {H.off.size(), H.list.size(), H.elb.size(), H.lb.size()};
  const bool ok = write_n(f, head, 6) && write_n(f, geo, 4) && write_n(f, sizes, 4) &&
                  write_n(f, H.off.data(), H.off.size()) && write_n(f, H.list.data(), H.list.size()) &&
                  write_n(f, H.elb.data(), H.elb.size()) && write_n(f, H.lb.data(), H.lb.size()) &&
                  write_n(f, H.always.data(), H.always.size());
  return std::fclose(f) == 0 && ok ? 0 : 2;
}

static void choice(const ScenePlan& p, char** a) {
  const bool xsrc = std::atoi(a[0]) != 0;
  const uint32_t flags = (uint32_t)std::strtoul(a[1], nullptr, 0);
  const uint32_t bucket_tiles = launch_binned(p, true, flags) && p.bucketed ? p.n_tiles : 0;
  const LaunchChoice c = launch_choice(p, std::atoi(a[2]) != 0, xsrc, bucket_tiles, flags, std::atoi(a[3]) != 0,
                                       std::atoi(a[4]) != 0, (size_t)std::atoi(a[5]));
  static const char* const family[] = {"transport_kernel", "ws_kernel", "voxel_kernel", "mesh_kernel"};
  std::printf("family=%s\ngm=%d\nxsrc=%d\nlds_faces=%d\ncoop=%d\nhist=%d\nphas=%d\nxf=%d\nslots=%d\niv=%d\ntk=%d\nscr=%d\n",
              family[c.family], c.gm, (int)c.xsrc, (int)c.lds_faces, (int)c.coop, (int)c.hist, (int)c.phas, (int)c.xf,
              c.slots, (int)c.iv, (int)c.tk, (int)c.scr);
  // (the block-size class: kernel_ptrs.h kernel_threads gives ws_kernel its own block, every other family 256)
  std::printf("block=%s\nlds=%zu\ngrid_key=%d\n", c.family == KF_WS ? "ws" : "256", c.lds, c.grid_key());
}

static int plan(const char* path, const char* cull_out = nullptr, char** choice_args = nullptr, int n_choices = 0) {
  std::FILE* f = std::fopen(path, "rb");
  int32_t hdr[3];
  if (!f || std::fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 0) return 2;
  std::vector<smcrt_sdf_node> nodes;
  std::vector<int32_t> top;
  std::vector<smcrt_grid> grid;
  std::vector<smcrt_detector> dets;
  if (!read_n(f, nodes, hdr[0]) || !read_n(f, top, hdr[1]) || !read_n(f, grid, 1) || !read_n(f, dets, hdr[2])) return 2;
  std::fclose(f);
  const PlanLimits lim{sizeof(WsSharedT<2>), sizeof(WsSharedT<3>)};
  ScenePlan p;
  const int st = plan_scene(nodes.data(), hdr[0], top.data(), hdr[1], grid.data(), hdr[2] ? dets.data() : nullptr, hdr[2],
                            read_knobs(), lim, &p);
  std::printf("status=%d\nerror=%s\n", st, g_last_error.c_str());
  if (st) return 0;
  if (cull_out) return dump_cull(p.cull, cull_out);
  if (choice_args) {
    const std::string kind = choice_args[0];
    p.voxel = kind == "voxel";
    p.mesh = kind == "mesh";
    for (int i = 0; i < n_choices; ++i) choice(p, choice_args + 1 + 6 * i);
    return 0;
  }
  std::printf("det_total=%lld\nh_det_off=", (long long)p.det_total);
  for (int64_t o : p.h_det_off) std::printf("%lld,", (long long)o);
  std::printf("\nn_prog=%d\nprog_size=%zu\nnested=%d\ncoop_lanes=%d\nctab=%d\ncull=%d\n", p.n_prog, p.prog.size(),
              (int)p.nested, p.coop_lanes, (int)!p.ctab.empty(), (int)p.cull.enabled);
  std::printf("fm_err=%a\nfm_step=%a\ninv2=%a,%a,%a\nfe=%d,%d,%d\ngrid_mode=%d\n", p.fm_err, p.fm_step, p.inv2[0],
              p.inv2[1], p.inv2[2], p.fe[0], p.fe[1], p.fe[2], p.grid_mode);
  std::printf("n_tiles=%u\nforce_atomic=%d\npool_cap_chunks=%llu\nbucketed=%d\nhist_tiles=%u\n", p.n_tiles,
              (int)p.force_atomic, (unsigned long long)p.pool_cap_chunks, (int)p.bucketed, p.hist_tiles);
  std::printf("face_bytes=%zu\nlds_faces=%d\nfresnel=%d\nws_slots=%d\nlean_mode=%d\nlean_debug=%u\nlean_candidate=%d\n",
              p.face_bytes, (int)p.lds_faces, (int)p.fresnel, p.ws_slots, p.lean_mode, p.lean_debug, (int)p.lean_candidate);
  std::printf("lean_lds=%zu\ntransport_lds=%zu\n", lean_lds(p), transport_lds(p, dep_words(p), false));
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "plan" && argc == 3) return plan(argv[2]);
  if (mode == "cull" && argc == 4) return plan(argv[2], argv[3]);
  if (mode == "choice" && argc >= 10 && (argc - 4) % 6 == 0) return plan(argv[2], nullptr, argv + 3, (argc - 4) / 6);
  if (mode == "slots" && argc == 5) {
    std::printf("slots=%d\n", slot_depth(read_pool_knobs(), std::atoi(argv[2]) != 0, std::strtoull(argv[3], nullptr, 10),
                                         std::strtoull(argv[4], nullptr, 10)));
    return 0;
  }
  std::fprintf(stderr, "usage: sceneplan_probe plan FILE | cull FILE OUT | slots LEAN_OR_FAR CAP_BYTES TOTAL_MEM | "
                       "choice FILE KIND (XSRC FLAGS LEAN_OK PATHS_ON PHASOR_ON N_SCREENS)...\n");
  return 2;
}
