// meshcast.h — the ray cast of mesh scenes ("Mesh media"): the triangle test and the
// traversal of the threaded bounding-volume hierarchy, written once for host and device.
//
// Nothing here is device-only: sceneplan.cpp (the builder, smcrt_scene_classify's host cast),
// tests/mesh_probe.cpp and mesh_kernel (mesh.h) compile this very text, with -ffp-contract=off,
// so the same ray gives the same bits everywhere.
//
// Definition: cast(o, dir, skip) is the hit (t, tri) with the smallest t > 0 over all triangles
// != skip, ties to the smallest triangle index, or "none". The hierarchy only prunes: its box test
// is conservative (padded boxes, a slab test that takes zero direction components by themselves;
// mesh_slab names the one subnormal case it leaves open), so the result is that of the brute-force
// loop over all triangles bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SMCRT_HD __host__ __device__
#else
#define SMCRT_HD
#endif

namespace smcrt {

constexpr int32_t MESH_NONE = -1;            // "no triangle": the one reserved index value
constexpr int32_t MESH_MAX_TRIS = 1 << 30;   // so that 2 nt - 1 nodes and the end link fit an int32
constexpr int32_t MESH_LEAF_TRIS = 4;

// A triangle as the cast reads it, in the hierarchy's order; `id` is its index in the caller's array.
struct MeshTri {
  double v0[3], e1[3], e2[3];  // e1 = v1 - v0, e2 = v2 - v0
  int32_t id, reserved;
};
// What a surface event reads, indexed by the caller's triangle index.
struct MeshFace {
  double N[3];               // normalise(e1 x e2)
  uint32_t outside, inside;  // the media on the side N points to, and on the other side
};
// A node of the threaded hierarchy. Nodes are stored in depth-first order: the first child of an
// inner node is the next node, and `skip` is the node to visit when the box is missed or the leaf
// is done (n_nodes: the traversal ends). skip > own index, so a cast visits each node at most once.
struct MeshNode {
  double lo[3], hi[3];    // padded box
  int32_t skip;
  int32_t first, count;   // a leaf's triangles (count > 0), tris[first .. first + count)
  int32_t reserved;
};

struct MeshHit {
  double t;         // (undefined when tri == MESH_NONE)
  int32_t tri;
  uint32_t visits;  // nodes visited
};

// Moeller-Trumbore in fp64, in the one order of operations DESIGN.md writes out.
SMCRT_HD inline bool mesh_tri_test(const MeshTri& T, const double o[3], const double d[3], double& t) {
  const double px = d[1] * T.e2[2] - d[2] * T.e2[1];
  const double py = d[2] * T.e2[0] - d[0] * T.e2[2];
  const double pz = d[0] * T.e2[1] - d[1] * T.e2[0];
  const double det = T.e1[0] * px + T.e1[1] * py + T.e1[2] * pz;
  if (det == 0.0) return false;
  const double inv = 1.0 / det;
  const double sx = o[0] - T.v0[0], sy = o[1] - T.v0[1], sz = o[2] - T.v0[2];
  const double u = (sx * px + sy * py + sz * pz) * inv;
  if (u < 0.0 || u > 1.0) return false;
  const double qx = sy * T.e1[2] - sz * T.e1[1];
  const double qy = sz * T.e1[0] - sx * T.e1[2];
  const double qz = sx * T.e1[1] - sy * T.e1[0];
  const double v = (d[0] * qx + d[1] * qy + d[2] * qz) * inv;
  if (v < 0.0 || u + v > 1.0) return false;
  t = (T.e2[0] * qx + T.e2[1] * qy + T.e2[2] * qz) * inv;
  return t > 0.0;
}

// One axis of the slab test. A zero direction component tests the origin against the slab; else
// the entry and exit parameters narrow [tn, tf]. With a finite reciprocal no NaN arises here at
// all (lo, hi and o are finite, and finite * finite is never NaN); the 0 * inf of a zero component
// is what the first line keeps out. One case is left open: a component so small (|d| < 2^-1024,
// subnormal) that 1/d overflows to inf, with the origin exactly on a slab plane. Then t1 or t2 is
// NaN, `t1 < t2` is false, and a can become +inf and reject the node. Directions here are unit
// vectors from fp64 sines and cosines, which do not produce such components; the cast test's
// rays have none either.
SMCRT_HD inline bool mesh_slab(double lo, double hi, double o, double d, double inv, double& tn, double& tf) {
  if (d == 0.0) return !(o < lo) && !(o > hi);
  const double t1 = (lo - o) * inv, t2 = (hi - o) * inv;
  const double a = t1 < t2 ? t1 : t2, b = t1 < t2 ? t2 : t1;
  if (a > tn) tn = a;
  if (b < tf) tf = b;
  return true;
}

SMCRT_HD inline MeshHit mesh_cast(const MeshNode* __restrict__ nodes, uint32_t n_nodes,
                                  const MeshTri* __restrict__ tris, const double o[3], const double d[3],
                                  int32_t skip) {
  MeshHit h;
  h.t = __builtin_inf();
  h.tri = MESH_NONE;
  h.visits = 0;
  const double ix = 1.0 / d[0], iy = 1.0 / d[1], iz = 1.0 / d[2];
  uint32_t node = 0;
  while (node < n_nodes) {
    const MeshNode* const nd = nodes + node;
    ++h.visits;
    // the box is missed if the ray leaves it before it enters, behind the origin, or beyond the
    // best hit so far (a tie at t == h.t is not beyond)
    double tn = 0.0, tf = h.t;
    bool in = mesh_slab(nd->lo[0], nd->hi[0], o[0], d[0], ix, tn, tf);
    in = mesh_slab(nd->lo[1], nd->hi[1], o[1], d[1], iy, tn, tf) && in;
    in = mesh_slab(nd->lo[2], nd->hi[2], o[2], d[2], iz, tn, tf) && in;
    in = in && !(tn > tf);
    const int32_t count = nd->count;
    if (in && count > 0) {
      const int32_t first = nd->first;
      for (int32_t k = first; k < first + count; ++k) {
        const MeshTri* const T = tris + k;
        double t;
        if (T->id != skip && mesh_tri_test(*T, o, d, t) && (t < h.t || (t == h.t && T->id < h.tri))) {
          h.t = t;
          h.tri = T->id;
        }
      }
    }
    node = (in && count == 0) ? node + 1 : (uint32_t)nd->skip;
  }
  return h;
}

}  // namespace smcrt
