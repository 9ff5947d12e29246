// mesh_probe.cpp — runs the mesh cast of the engine (rsmcrt_amd/csrc/meshcast.h, the text mesh_kernel
// compiles) on the host, through the hierarchy plan_mesh_scene builds, for tests/mesh_cases.py.
// Host code only: built from this file, sceneplan.cpp and cull.cpp; no kernel object, no
// libsmcrt.so, no GPU.
//
//   mesh_probe cast FILE OUT   FILE: int32 nv, nt, n_rays, 0 | smcrt_grid | double verts[nv][3] |
//                              int32 tris[nt][3] | double origins[n_rays][3] | double dirs[n_rays][3] |
//                              int32 skips[n_rays]
//                              OUT: int32 n_nodes, n_leaves, max_leaf, 0 | double t[n_rays] |
//                              int32 tri[n_rays] | uint32 visits[n_rays]
// Prints status=, error= and n_nodes= lines. Every triangle gets the media (0, 0).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../rsmcrt_amd/csrc/hosterr.h"
#include "../rsmcrt_amd/csrc/sceneplan.h"

thread_local std::string smcrt::g_last_error;
using namespace smcrt;

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 4 || std::string(argv[1]) != "cast") return 2;
  std::FILE* f = std::fopen(argv[2], "rb");
  int32_t hdr[4];
  if (!f || std::fread(hdr, sizeof(int32_t), 4, f) != 4 || hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 0) return 2;
  const int32_t nv = hdr[0], nt = hdr[1], nr = hdr[2];
  std::vector<smcrt_grid> grid;
  std::vector<double> verts, org, dir;
  std::vector<int32_t> tris, skips;
  if (!read_n(f, grid, 1) || !read_n(f, verts, (size_t)3 * nv) || !read_n(f, tris, (size_t)3 * nt) ||
      !read_n(f, org, (size_t)3 * nr) || !read_n(f, dir, (size_t)3 * nr) || !read_n(f, skips, (size_t)nr))
    return 2;
  std::fclose(f);
  const std::vector<uint8_t> tri_media((size_t)2 * nt, 0);
  const smcrt_medium medium = {1.0, 0.0, 0.0, 1.0};
  ScenePlan p;
  const int st = plan_mesh_scene(verts.data(), nv, tris.data(), tri_media.data(), nt, &medium, 1, 0, grid.data(), nullptr, 0,
                                 read_knobs(), &p);
  std::printf("status=%d\nerror=%s\n", st, g_last_error.c_str());
  if (st) return 0;
  const int32_t n_nodes = (int32_t)p.mesh_nodes.size();
  int32_t n_leaves = 0, max_leaf = 0;
  bool links_ok = true;  // skip > own index, first child next, leaves tile the triangles
  for (int32_t i = 0; i < n_nodes; ++i) {
    const MeshNode& nd = p.mesh_nodes[i];
    links_ok = links_ok && nd.skip > i && nd.skip <= n_nodes;
    if (nd.count > 0) {
      ++n_leaves;
      max_leaf = nd.count > max_leaf ? nd.count : max_leaf;
      links_ok = links_ok && nd.first >= 0 && nd.first + nd.count <= nt;
    }
  }
  std::printf("n_nodes=%d\nlinks_ok=%d\n", n_nodes, (int)links_ok);
  std::vector<double> t(nr);
  std::vector<int32_t> tri(nr);
  std::vector<uint32_t> visits(nr);
  for (int32_t r = 0; r < nr; ++r) {
    const MeshHit h = mesh_cast(p.mesh_nodes.data(), (uint32_t)n_nodes, p.mesh_tris.data(), &org[3 * (size_t)r],
                                &dir[3 * (size_t)r], skips[r]);
    t[r] = h.tri == MESH_NONE ? HUGE_VAL : h.t;
    tri[r] = h.tri;
    visits[r] = h.visits;
  }
  std::FILE* o = std::fopen(argv[3], "wb");
  const int32_t oh[4] = {n_nodes, n_leaves, max_leaf, 0};
  const bool ok = o && std::fwrite(oh, sizeof(int32_t), 4, o) == 4 && std::fwrite(t.data(), sizeof(double), nr, o) == (size_t)nr &&
                  std::fwrite(tri.data(), sizeof(int32_t), nr, o) == (size_t)nr &&
                  std::fwrite(visits.data(), sizeof(uint32_t), nr, o) == (size_t)nr;
  return o && std::fclose(o) == 0 && ok ? 0 : 2;
}
