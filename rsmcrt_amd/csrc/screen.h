// screen.h — the hit rule of the field screens (include/smcrt.h "field screens"),
// written once for host and device, as meshcast.h is.
//
// smcrt_screen_hit (smcrt.hip, host) and screen_hits (phasor.h, the PHAS instantiations of
// transport_kernel) compile this very text with -ffp-contract=off, so the same leg gives the same
// t and the same pixel everywhere.
#pragma once
#include <stdint.h>

#include "geometry.h"

namespace smcrt {

constexpr int32_t SCREEN_MAX = 16;        // screens per scene
constexpr int32_t SCREEN_MAX_PIXELS = 4096;  // per edge

// A screen as the rule reads it: smcrt_screen plus what plan_screens (sceneplan.cpp) computes once.
struct ScreenDev {
  double origin[3], eu[3], ev[3];
  double N[3];      // normalise(eu x ev)
  double uu, vv;    // dot(eu, eu), dot(ev, ev)
  int32_t nu, nv, sides, reserved;
  uint64_t offset;  // doubles before this screen's pixels in the field buffer
};

// One leg (start, dir, sep) against one screen: true, t and pixel = iu + nu * iv for a hit.
__host__ __device__ inline bool screen_hit(const ScreenDev& S, const V3 start, const V3 dir, double sep, double& t,
                                           int32_t& pixel) {
  const V3 N = v3(S.N[0], S.N[1], S.N[2]);
  const V3 o = v3(S.origin[0], S.origin[1], S.origin[2]);
  const double den = dot(dir, N);
  if (den == 0.0) return false;
  if ((S.sides > 0 && !(den > 0.0)) || (S.sides < 0 && !(den < 0.0))) return false;
  const double tt = dot(o - start, N) / den;
  if (!(tt > 0.0 && tt <= sep)) return false;
  const V3 w = (start + smul(tt, dir)) - o;
  const double u = dot(w, v3(S.eu[0], S.eu[1], S.eu[2])) / S.uu;
  const double v = dot(w, v3(S.ev[0], S.ev[1], S.ev[2])) / S.vv;
  if (!(u >= 0.0 && u < 1.0 && v >= 0.0 && v < 1.0)) return false;
  int32_t iu = (int32_t)(u * (double)S.nu), iv = (int32_t)(v * (double)S.nv);
  if (iu > S.nu - 1) iu = S.nu - 1;
  if (iv > S.nv - 1) iv = S.nv - 1;
  t = tt;
  pixel = iu + S.nu * iv;
  return true;
}

}  // namespace smcrt
