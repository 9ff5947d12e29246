// launchchoice.h — which compiled kernel a launch runs, and with what dynamic LDS: plain data.
// sceneplan.h launch_choice fills it without a device, kernel_ptrs.h maps it to the host stub and
// the block size (a header of its own, so that kinst.hip does not depend on sceneplan.h), and
// smcrt.hip's occupancy query (blocks_for) and its launch both read it: the two cannot differ.
#pragma once
#include <stddef.h>

namespace smcrt {

enum KernelFamily : int { KF_TRANSPORT, KF_WS, KF_VOXEL, KF_MESH };
constexpr int GRID_KEY_WS = 8, GRID_KEY_PPL = 9, N_GRID_KEYS = 11;
struct LaunchChoice {
  KernelFamily family = KF_TRANSPORT;
  // the family's template coordinates as kernel_ptrs.h takes them (the others stay 0)
  int gm = 0;              // every family
  bool xsrc = false;       // transport_kernel, voxel_kernel, mesh_kernel
  bool lds_faces = false;  // transport_kernel (already dropped for (xsrc && coop) || hist || phas), ws_kernel
  bool coop = false, hist = false, phas = false;  // transport_kernel
  bool xf = false, iv = false, tk = false;        // ws_kernel
  int slots = 0;
  bool ppl = false;  // voxel_kernel, mesh_kernel: the partial path lengths (ppath.h), with their rows of LDS
  bool scr = false;  // a PHAS launch that tallies field screens: no coordinate, a fourth start-point row of LDS
  size_t lds = 0;    // dynamic LDS bytes
  // Launches of a scene with equal keys run the same kernel with the same block and LDS, up to
  // ws_kernel's TK (same block, same LDS, same register cap): they share a persistent grid.
  int grid_key() const {
    if (ppl) return GRID_KEY_PPL + (xsrc ? 1 : 0);
    return family == KF_WS ? GRID_KEY_WS : 2 * (hist ? 1 : scr ? 3 : phas ? 2 : 0) + (xsrc ? 1 : 0);
  }
};

}  // namespace smcrt
