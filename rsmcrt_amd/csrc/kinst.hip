// kinst.hip — one (LDS faces, grid mode) slice of the transport kernel instantiations.
// Compiled forty-two times by build.py (-DKI_F=0/1 -DKI_G=0/1/2 -DKI_P=0/1/5/6, and -DKI_P=2, 3,
// 4, 7, 8 and 9 with -DKI_F=0); see kernel_ptrs.h.
// Part 0 holds transport_kernel and the XF ws_kernel, part 1 the plain ws_kernel (the lean path
// of M1), which build.py compiles with its own scheduler flags (see UNITS there), part 2 the
// HIST instantiations of transport_kernel (the photon path recorder, paths.h; faces in device
// memory only), in units of their own so that they build beside the others, part 3 likewise the
// PHAS instantiations (the phasor tally, phasor.h). Nothing is instantiated for PHAS && HIST.
// Part 4 holds voxel_kernel (voxel.h: label volumes, no SDF), plain and general emitter.
// Parts 5 and 6 hold ws_kernel's TK = true instantiations (SMCRT_FLAG_TEST_KERNEL runs, ws.h), the
// plain ones (5, with part 1's scheduler flags) and the XF ones (6, with part 0's), in units of
// their own so that they build beside the others.
// Part 7 holds mesh_kernel (mesh.h: closed triangle surfaces, no SDF), plain and general emitter.
// Parts 8 and 9 hold the PPL instantiations of voxel_kernel and of mesh_kernel (the partial path
// lengths, ppath.h), in units of their own so that parts 4 and 7 stay the objects they were.
#include "kernels.h"
#include "kernel_ptrs.h"
#if defined(KI_P) && (KI_P == 4 || KI_P == 8)
#include "voxel.h"
#endif
#if defined(KI_P) && (KI_P == 7 || KI_P == 9)
#include "mesh.h"
#endif

#if !defined(KI_F) || !defined(KI_G) || !defined(KI_P)
#error "kinst.hip is compiled with -DKI_F=<0|1> -DKI_G=<0|1|2> -DKI_P=<0|1|2|3|4|5|6|7|8|9> (rsmcrt_amd/build.py)"
#endif
#define KI_NAME3(a, f, g) a##_##f##_##g
#define KI_NAME2(a, f, g) KI_NAME3(a, f, g)
#define KI_NAME(a) KI_NAME2(a, KI_F, KI_G)

namespace smcrt {

#if KI_P == 9
#if KI_F != 0
#error "mesh_kernel's PPL instantiations (KI_P=9) are compiled with KI_F=0 only (its faces are always staged in LDS)"
#endif
const void* KI_NAME(kinst_mesh_ppl)(int xsrc) {
  return xsrc ? (const void*)mesh_kernel<KI_G, true, true> : (const void*)mesh_kernel<KI_G, false, true>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagmp)
#elif KI_P == 8
#if KI_F != 0
#error "voxel_kernel's PPL instantiations (KI_P=8) are compiled with KI_F=0 only (its faces are always staged in LDS)"
#endif
const void* KI_NAME(kinst_voxel_ppl)(int xsrc) {
  return xsrc ? (const void*)voxel_kernel<KI_G, true, true> : (const void*)voxel_kernel<KI_G, false, true>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagvp)
#elif KI_P == 7
#if KI_F != 0
#error "mesh_kernel (KI_P=7) is compiled with KI_F=0 only (its faces are always staged in LDS)"
#endif
const void* KI_NAME(kinst_mesh)(int xsrc) {
  return xsrc ? (const void*)mesh_kernel<KI_G, true> : (const void*)mesh_kernel<KI_G, false>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagm)
#elif KI_P == 4
#if KI_F != 0
#error "voxel_kernel (KI_P=4) is compiled with KI_F=0 only (its faces are always staged in LDS)"
#endif
const void* KI_NAME(kinst_voxel)(int xsrc) {
  return xsrc ? (const void*)voxel_kernel<KI_G, true> : (const void*)voxel_kernel<KI_G, false>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagv)
#elif KI_P == 3
#if KI_F != 0
#error "the PHAS instantiations (KI_P=3) exist with KI_F=0 only"
#endif
const void* KI_NAME(kinst_transport_phas)(int xsrc, int coop) {
  if (xsrc && coop) return (const void*)transport_kernel<false, KI_G, true, true, false, true>;
  if (xsrc) return (const void*)transport_kernel<false, KI_G, true, false, false, true>;
  if (coop) return (const void*)transport_kernel<false, KI_G, false, true, false, true>;
  return (const void*)transport_kernel<false, KI_G, false, false, false, true>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagf)
#elif KI_P == 2
#if KI_F != 0
#error "the HIST instantiations (KI_P=2) exist with KI_F=0 only"
#endif
const void* KI_NAME(kinst_transport_hist)(int xsrc, int coop) {
  if (xsrc && coop) return (const void*)transport_kernel<false, KI_G, true, true, true>;
  if (xsrc) return (const void*)transport_kernel<false, KI_G, true, false, true>;
  if (coop) return (const void*)transport_kernel<false, KI_G, false, true, true>;
  return (const void*)transport_kernel<false, KI_G, false, false, true>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagh)
#elif KI_P == 6
// the XF ws_kernel of test_kernel runs (xf 2: with the in-voxel segments' code)
const void* KI_NAME(kinst_wsxt)(int xf, int slots) {
  if (xf == 2)
    return slots == 3 ? (const void*)ws_kernel<KI_F != 0, KI_G, true, 3, true, true>
                      : (const void*)ws_kernel<KI_F != 0, KI_G, true, 2, true, true>;
  return slots == 3 ? (const void*)ws_kernel<KI_F != 0, KI_G, true, 3, false, true>
                    : (const void*)ws_kernel<KI_F != 0, KI_G, true, 2, false, true>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagxt)
#elif KI_P == 5
// the plain ws_kernel of test_kernel runs
const void* KI_NAME(kinst_wspt)(int slots) {
  return slots == 3 ? (const void*)ws_kernel<KI_F != 0, KI_G, false, 3, true, true>
                    : (const void*)ws_kernel<KI_F != 0, KI_G, false, 2, true, true>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagpt)
#elif KI_P == 1
// the plain ws_kernel (no Fresnel program points, no detectors)
const void* KI_NAME(kinst_wsp)(int slots) {
  return slots == 3 ? (const void*)ws_kernel<KI_F != 0, KI_G, false, 3, true, false>
                    : (const void*)ws_kernel<KI_F != 0, KI_G, false, 2, true, false>;
}
#define KI_DIAG_NAME KI_NAME(kinst_diagp)
#else
const void* KI_NAME(kinst_transport)(int xsrc, int coop) {
  constexpr bool F = KI_F != 0;
  if (xsrc && coop) {
    if constexpr (!F) return (const void*)transport_kernel<false, KI_G, true, true>;
    return nullptr;
  }
  if (xsrc) return (const void*)transport_kernel<F, KI_G, true, false>;
  if (coop) return (const void*)transport_kernel<F, KI_G, false, true>;
  return (const void*)transport_kernel<F, KI_G, false, false>;
}

#if KI_F == 0 && KI_G == 0
size_t kinst_ws_shared_bytes(int slots) { return slots == 3 ? sizeof(WsSharedT<3>) : sizeof(WsSharedT<2>); }
int kinst_ws_threads() { return WS_THREADS; }
int kinst_ws_photon_lanes() { return (int)WS_NPL; }
size_t kinst_ws_scratch_bytes(size_t lanes) { return ws_scratch_bytes(lanes); }
#endif

// xf 2: the XF instantiation with the in-voxel segments' code; tk: a test_kernel run (parts 5 and 6)
const void* KI_NAME(kinst_ws)(int xf, int slots, int tk) {
  if (tk) return xf ? KI_NAME(kinst_wsxt)(xf, slots) : KI_NAME(kinst_wspt)(slots);
  if (xf == 2)
    return slots == 3 ? (const void*)ws_kernel<KI_F != 0, KI_G, true, 3, true, false>
                      : (const void*)ws_kernel<KI_F != 0, KI_G, true, 2, true, false>;
  if (xf)
    return slots == 3 ? (const void*)ws_kernel<KI_F != 0, KI_G, true, 3, false, false>
                      : (const void*)ws_kernel<KI_F != 0, KI_G, true, 2, false, false>;
  return KI_NAME(kinst_wsp)(slots);
}
#define KI_DIAG_NAME KI_NAME(kinst_diag)
#endif


// (each part has its own copy of the static tallies)
void KI_DIAG_NAME(unsigned long long* d72, unsigned long long* t9, unsigned long long* c6) {
#ifdef SMCRT_DIAG
  unsigned long long h[72] = {0}, z[72] = {0};
  if (hipDeviceSynchronize() != hipSuccess) return;
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_diag), sizeof(h)) == hipSuccess)
    for (int i = 0; i < 72; ++i) d72[i] += (i >= 68 && i <= 69) ? 0 : h[i];
  for (int i = 68; i <= 69; ++i) d72[i] = h[i] > d72[i] ? h[i] : d72[i];  // the longest wave: a max
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_diag), z, sizeof(z));
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_diag_t), sizeof(unsigned long long) * 9) == hipSuccess)
    for (int i = 0; i < 9; ++i) t9[i] += h[i];
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_diag_t), z, sizeof(unsigned long long) * 9);
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_cull_diag), sizeof(unsigned long long) * 6) == hipSuccess)
    for (int i = 0; i < 6; ++i) c6[i] += h[i];
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_cull_diag), z, sizeof(unsigned long long) * 6);
#else
  (void)d72; (void)t9; (void)c6;
#endif
}

}  // namespace smcrt
