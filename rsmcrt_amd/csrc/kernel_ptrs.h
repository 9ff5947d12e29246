// kernel_ptrs.h — the transport kernel instantiations, reached through pointers.
//
// build.py compiles kinst.hip once per (LDS faces F, grid mode G, part P) with -DKI_F=F -DKI_G=G
// -DKI_P=P (part 1: the plain ws_kernel, with its own scheduler flags; parts 5 and 6: the plain
// and the XF ws_kernel of test_kernel runs, TK = true in ws.h; part 2, F = 0 only:
// transport_kernel's HIST instantiations, the photon path recorder of paths.h; part 3, F = 0
// only: its PHAS instantiations, the phasor tally of phasor.h; part 4, F = 0 only: voxel_kernel,
// the label-volume transport of voxel.h; part 7, F = 0 only: mesh_kernel, the triangle-surface
// transport of mesh.h; parts 8 and 9, F = 0 only: the PPL instantiations of voxel_kernel and of
// mesh_kernel, the partial path lengths of ppath.h), so
// the instantiations of transport_kernel and ws_kernel (kernels.h, ws.h) build in parallel
// instead of in one translation unit. Each object exports these getters; hipLaunchKernel and
// the occupancy query take the host stub that kernel_ptr returns for a launch choice.
#pragma once
#include <stddef.h>

#include "launchchoice.h"

namespace smcrt {

size_t kinst_ws_shared_bytes(int slots);  // sizeof(WsSharedT<slots>), ws_kernel's static LDS (slots 2 or 3)
int kinst_ws_threads();            // ws_kernel's block size
int kinst_ws_photon_lanes();       // photon lanes per ws_kernel block
size_t kinst_ws_scratch_bytes(size_t lanes);  // ws_kernel lane scratch (ws.h WX_*) of that many photon lanes

#define SMCRT_KINST_DECL(F, G)                                                               \
  const void* kinst_transport_##F##_##G(int xsrc, int coop);                                 \
  const void* kinst_ws_##F##_##G(int xf, int slots, int tk);                                 \
  const void* kinst_wsp_##F##_##G(int slots);                                                \
  const void* kinst_wspt_##F##_##G(int slots);                                               \
  const void* kinst_wsxt_##F##_##G(int xf, int slots);                                       \
  void kinst_diagpt_##F##_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6); \
  void kinst_diagxt_##F##_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6); \
  void kinst_diag_##F##_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6); \
  void kinst_diagp_##F##_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6);
SMCRT_KINST_DECL(0, 0)
SMCRT_KINST_DECL(0, 1)
SMCRT_KINST_DECL(0, 2)
SMCRT_KINST_DECL(1, 0)
SMCRT_KINST_DECL(1, 1)
SMCRT_KINST_DECL(1, 2)
#undef SMCRT_KINST_DECL
#define SMCRT_KINST_HIST_DECL(G)                                  \
  const void* kinst_transport_hist_0_##G(int xsrc, int coop);     \
  void kinst_diagh_0_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6);
SMCRT_KINST_HIST_DECL(0)
SMCRT_KINST_HIST_DECL(1)
SMCRT_KINST_HIST_DECL(2)
#undef SMCRT_KINST_HIST_DECL
#define SMCRT_KINST_PHAS_DECL(G)                                  \
  const void* kinst_transport_phas_0_##G(int xsrc, int coop);     \
  void kinst_diagf_0_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6);
SMCRT_KINST_PHAS_DECL(0)
SMCRT_KINST_PHAS_DECL(1)
SMCRT_KINST_PHAS_DECL(2)
#undef SMCRT_KINST_PHAS_DECL
#define SMCRT_KINST_VOXEL_DECL(G)              \
  const void* kinst_voxel_0_##G(int xsrc);     \
  void kinst_diagv_0_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6);
SMCRT_KINST_VOXEL_DECL(0)
SMCRT_KINST_VOXEL_DECL(1)
SMCRT_KINST_VOXEL_DECL(2)
#undef SMCRT_KINST_VOXEL_DECL
#define SMCRT_KINST_MESH_DECL(G)               \
  const void* kinst_mesh_0_##G(int xsrc);      \
  void kinst_diagm_0_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6);
SMCRT_KINST_MESH_DECL(0)
SMCRT_KINST_MESH_DECL(1)
SMCRT_KINST_MESH_DECL(2)
#undef SMCRT_KINST_MESH_DECL
#define SMCRT_KINST_PPL_DECL(G)                    \
  const void* kinst_voxel_ppl_0_##G(int xsrc);     \
  const void* kinst_mesh_ppl_0_##G(int xsrc);      \
  void kinst_diagvp_0_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6); \
  void kinst_diagmp_0_##G(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6);
SMCRT_KINST_PPL_DECL(0)
SMCRT_KINST_PPL_DECL(1)
SMCRT_KINST_PPL_DECL(2)
#undef SMCRT_KINST_PPL_DECL

// transport_kernel<lds_faces, gm, xsrc, coop, hist, phas>; the general emitter with the COOP
// machinery (xsrc && coop), the path recorder (hist, paths.h) and the phasor tally (phas,
// phasor.h) exist with faces in device memory only; hist && phas does not exist (nullptr)
inline const void* transport_kernel_ptr(bool lds_faces, int gm, bool xsrc, bool coop, bool hist = false,
                                        bool phas = false) {
  if ((xsrc && coop) || hist || phas) lds_faces = false;
  const int x = xsrc ? 1 : 0, c = coop ? 1 : 0;
  if (hist && phas) return nullptr;
  if (phas) return gm == 0 ? kinst_transport_phas_0_0(x, c) : gm == 1 ? kinst_transport_phas_0_1(x, c)
                                                                      : kinst_transport_phas_0_2(x, c);
  if (hist) return gm == 0 ? kinst_transport_hist_0_0(x, c) : gm == 1 ? kinst_transport_hist_0_1(x, c)
                                                                      : kinst_transport_hist_0_2(x, c);
  switch ((lds_faces ? 3 : 0) + gm) {
    case 0: return kinst_transport_0_0(x, c);
    case 1: return kinst_transport_0_1(x, c);
    case 2: return kinst_transport_0_2(x, c);
    case 3: return kinst_transport_1_0(x, c);
    case 4: return kinst_transport_1_1(x, c);
    default: return kinst_transport_1_2(x, c);
  }
}
// voxel_kernel<gm, xsrc, ppl> (voxel.h)
inline const void* voxel_kernel_ptr(int gm, bool xsrc, bool ppl = false) {
  const int x = xsrc ? 1 : 0;
  if (ppl) return gm == 0 ? kinst_voxel_ppl_0_0(x) : gm == 1 ? kinst_voxel_ppl_0_1(x) : kinst_voxel_ppl_0_2(x);
  return gm == 0 ? kinst_voxel_0_0(x) : gm == 1 ? kinst_voxel_0_1(x) : kinst_voxel_0_2(x);
}
// mesh_kernel<gm, xsrc, ppl> (mesh.h)
inline const void* mesh_kernel_ptr(int gm, bool xsrc, bool ppl = false) {
  const int x = xsrc ? 1 : 0;
  if (ppl) return gm == 0 ? kinst_mesh_ppl_0_0(x) : gm == 1 ? kinst_mesh_ppl_0_1(x) : kinst_mesh_ppl_0_2(x);
  return gm == 0 ? kinst_mesh_0_0(x) : gm == 1 ? kinst_mesh_0_1(x) : kinst_mesh_0_2(x);
}
// ws_kernel<lds_faces, gm, xf, slots, iv, tk> (xf: the Fresnel/detector program points; slots 2 or
// 3; iv: the in-voxel segments' code, always in the plain instantiation; tk: a run with
// SMCRT_FLAG_TEST_KERNEL, every other run takes the instantiation without its event code, ws.h)
inline const void* ws_kernel_ptr(bool lds_faces, int gm, bool xf, int slots, bool iv, bool tk) {
  const int x = xf ? (iv ? 2 : 1) : 0, t = tk ? 1 : 0;
  switch ((lds_faces ? 3 : 0) + gm) {
    case 0: return kinst_ws_0_0(x, slots, t);
    case 1: return kinst_ws_0_1(x, slots, t);
    case 2: return kinst_ws_0_2(x, slots, t);
    case 3: return kinst_ws_1_0(x, slots, t);
    case 4: return kinst_ws_1_1(x, slots, t);
    default: return kinst_ws_1_2(x, slots, t);
  }
}
// the host stub and the block size of a launch choice (sceneplan.h launch_choice)
inline const void* kernel_ptr(const LaunchChoice& c) {
  switch (c.family) {
    case KF_WS: return ws_kernel_ptr(c.lds_faces, c.gm, c.xf, c.slots, c.iv, c.tk);
    case KF_VOXEL: return voxel_kernel_ptr(c.gm, c.xsrc, c.ppl);
    case KF_MESH: return mesh_kernel_ptr(c.gm, c.xsrc, c.ppl);
    default: return transport_kernel_ptr(c.lds_faces, c.gm, c.xsrc, c.coop, c.hist, c.phas);
  }
}
inline int kernel_threads(const LaunchChoice& c) { return c.family == KF_WS ? kinst_ws_threads() : 256; }
// diagnostic builds: the kernels' tallies summed over the objects (each is cleared)
inline void kinst_diag_gather(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6) {
  for (int i = 0; i < 72; ++i) d72[i] = 0;
  for (int i = 0; i < 9; ++i) t9[i] = 0;
  for (int i = 0; i < 6; ++i) c6[i] = 0;
  kinst_diag_0_0(d72, t9, c6); kinst_diag_0_1(d72, t9, c6); kinst_diag_0_2(d72, t9, c6);
  kinst_diag_1_0(d72, t9, c6); kinst_diag_1_1(d72, t9, c6); kinst_diag_1_2(d72, t9, c6);
  kinst_diagp_0_0(d72, t9, c6); kinst_diagp_0_1(d72, t9, c6); kinst_diagp_0_2(d72, t9, c6);
  kinst_diagp_1_0(d72, t9, c6); kinst_diagp_1_1(d72, t9, c6); kinst_diagp_1_2(d72, t9, c6);
  kinst_diagpt_0_0(d72, t9, c6); kinst_diagpt_0_1(d72, t9, c6); kinst_diagpt_0_2(d72, t9, c6);
  kinst_diagpt_1_0(d72, t9, c6); kinst_diagpt_1_1(d72, t9, c6); kinst_diagpt_1_2(d72, t9, c6);
  kinst_diagxt_0_0(d72, t9, c6); kinst_diagxt_0_1(d72, t9, c6); kinst_diagxt_0_2(d72, t9, c6);
  kinst_diagxt_1_0(d72, t9, c6); kinst_diagxt_1_1(d72, t9, c6); kinst_diagxt_1_2(d72, t9, c6);
  kinst_diagh_0_0(d72, t9, c6); kinst_diagh_0_1(d72, t9, c6); kinst_diagh_0_2(d72, t9, c6);
  kinst_diagf_0_0(d72, t9, c6); kinst_diagf_0_1(d72, t9, c6); kinst_diagf_0_2(d72, t9, c6);
  kinst_diagv_0_0(d72, t9, c6); kinst_diagv_0_1(d72, t9, c6); kinst_diagv_0_2(d72, t9, c6);
  kinst_diagm_0_0(d72, t9, c6); kinst_diagm_0_1(d72, t9, c6); kinst_diagm_0_2(d72, t9, c6);
  kinst_diagvp_0_0(d72, t9, c6); kinst_diagvp_0_1(d72, t9, c6); kinst_diagvp_0_2(d72, t9, c6);
  kinst_diagmp_0_0(d72, t9, c6); kinst_diagmp_0_1(d72, t9, c6); kinst_diagmp_0_2(d72, t9, c6);
}

}  // namespace smcrt
