// k_adaround.cuh — AdaRound (Nagel et al. 2020) element arithmetic, shared by the device
// kernels (k_adaround.hip) and the host loops (k_host.hip): one __host__ __device__
// definition, so both sides compute the same bits wherever their libm / OCML pow agree
// (the regulariser's f64 pow is the only call that is not op-for-op the same).
//
// Per element, fp32 unless stated (include/vsiq.h has the full statement):
//   t   = RN(RN(w / s) + z)            the forward kernels' quotient and add (caller)
//   b   = floor(t)
//   sig = 1 / (1 + sleef_expf_u10(-V))
//   hr  = fmaf(sig, 1.2, -0.1)         zeta = 1.1, gamma = -0.1
//   h   = min(max(hr, 0), 1)           a NaN gives 0 (as the hard rounding does)
//   hp  = 0 < hr < 1 ? 1.2 sig (1 - sig) : 0
//   r   = b + h;  c = clamp(r, lo, hi);  y = (c - z) s;  m = lo <= r <= hi
//   hard: h = V >= 0 ? 1 : 0
//   f64: u = |2h - 1|;  R term = 1 - pow(u, beta);  dR/dh = -2 beta sign(2h - 1) pow(u, beta - 1)
//   grad_V = fp32(((double)g (double)s m + lambda dR/dh) (double)hp)
#pragma once
#include <cmath>

#include "vsiq_common.cuh"

namespace vsiq {

struct AdaH {
  float h, hp;
};

__host__ __device__ __forceinline__ AdaH ada_soft(float v) {
  const float sig = 1.0f / (1.0f + sleef_expf_u10(-v));   // IEEE division (build flags)
  const float hr = __builtin_fmaf(sig, 1.2f, -0.1f);
  AdaH o;
  o.h = hr > 0.0f ? (hr < 1.0f ? hr : 1.0f) : 0.0f;   // NaN -> 0
  o.hp = (0.0f < hr && hr < 1.0f) ? (1.2f * sig) * (1.0f - sig) : 0.0f;
  return o;
}

__host__ __device__ __forceinline__ float ada_hard(float v) { return v >= 0.0f ? 1.0f : 0.0f; }   // tie up, NaN -> 0

struct AdaOut {
  float y;
  bool m;
};

// t = RN(RN(w / s) + z); torch.clamp semantics (a NaN t gives a NaN y)
__host__ __device__ __forceinline__ AdaOut ada_out(float t, float h, float s, float z, float lo, float hi) {
  const float r = __builtin_floorf(t) + h;
  const float c = r < lo ? lo : (r > hi ? hi : r);
  AdaOut o;
  o.y = (c - z) * s;
  o.m = r >= lo && r <= hi;
  return o;
}

// pow(1, e) is 1 exactly: spelled out because h sits at 0 or 1 (u == 1) for most elements
// of a converged layer, and the f64 pow is by far the dearest operation here
__host__ __device__ __forceinline__ double ada_pow(double u, double e) { return u == 1.0 ? 1.0 : pow(u, e); }

__host__ __device__ __forceinline__ double ada_reg(float h, double beta) {
  const double u = __builtin_fabs(2.0 * (double)h - 1.0);
  return 1.0 - ada_pow(u, beta);
}

__host__ __device__ __forceinline__ double ada_dreg(float h, double beta) {
  const double d = 2.0 * (double)h - 1.0;
  const double u = __builtin_fabs(d);
  if (u == 0.0) return 0.0;
  return ((-2.0 * beta) * (d > 0.0 ? 1.0 : -1.0)) * ada_pow(u, beta - 1.0);
}

__host__ __device__ __forceinline__ float ada_grad(float g, float t, float v, float s, float z, float lo, float hi,
                                                   double lam, double beta) {
  const AdaH a = ada_soft(v);
  const AdaOut o = ada_out(t, a.h, s, z, lo, hi);
  const double dy = ((double)g * (double)s) * (o.m ? 1.0 : 0.0);
  return (float)((dy + lam * ada_dreg(a.h, beta)) * (double)a.hp);   // rounded once
}

enum { kAdaSoft = 0, kAdaSoftReg = 1, kAdaHard = 2, kAdaRegOnly = 3 };

}  // namespace vsiq
