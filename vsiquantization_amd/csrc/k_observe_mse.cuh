// k_observe_mse.cuh — the MSE observer's arithmetic, shared by the device pass
// (k_observe_mse.hip) and the host loop (k_host.hip): the ratio table's checks, which calls
// search at all, a candidate's range and qparams, the error term of one element, the pick
// and the end of the call.  Everything is f64 and never contracted (-ffp-contract=off);
// include/vsiq.h states the definition.
#pragma once
#include "k_observe_hist.cuh"

namespace vsiq {

constexpr int kMseMaxCand = 128;   // candidates of one call: two per lane of a wave

// the ratio table as the kernel receives it: by value, 1 KB of kernarg (no device table,
// nothing to copy: the call captures into a HIP graph)
struct MseRatios {
  double r[kMseMaxCand];
};

// count in [1, 128], r[0] == 1, every r[k] in (0, 1] (NaN: no)
inline bool mse_ratios_ok(const double *ratios, int count) {
  if (!ratios || count < 1 || count > kMseMaxCand || ratios[0] != 1.0) return false;
  for (int k = 0; k < count; ++k)
    if (!(ratios[k] > 0.0 && ratios[k] <= 1.0)) return false;
  return true;
}

// the call is MinMaxObserver's (no pass over the tensor): a NaN call changes nothing anyway
// (minmax.py:42-47), a constant or non-finite range has nothing to shrink, one candidate
// is the min / max itself
__host__ __device__ __forceinline__ bool mse_fallback(float mn, float mx, bool has_nan, int count) {
  return has_nan || mn == mx || !__builtin_isfinite(mn) || !__builtin_isfinite(mx) || count == 1;
}

__host__ __device__ __forceinline__ void mse_range(float mn, float mx, double r, float *lo, float *hi) {
  *lo = (float)((double)mn * r);
  *hi = (float)((double)mx * r);
}

// candidate k: the fp32 (scale, zero point) a fresh observer returns for its range, and
// whether the search may use it (scale finite and > 0, zero point finite)
struct MseCand {
  float s, z;
  bool valid;
};

__host__ __device__ __forceinline__ MseCand mse_candidate(float mn, float mx, double r, int sym, double qden,
                                                          double eps) {
  float lo, hi;
  mse_range(mn, mx, r, &lo, &hi);
  double s, z;
  minmax_qparams((double)(lo < 0.0f ? lo : 0.0f), (double)(hi > 0.0f ? hi : 0.0f), sym, qden, eps, &s, &z);
  MseCand c;
  c.s = (float)s;
  c.z = (float)z;
  c.valid = __builtin_isfinite(c.s) && c.s > 0.0f && __builtin_isfinite(z);
  return c;
}

// one element's term of E_k: y the fake-quantized value of v
__host__ __device__ __forceinline__ double mse_term(float y, float v) {
  const double d = (double)y - (double)v;
  return d * d;
}

// the smallest k with E[k] minimal: a strict < scan from 0 (all inf, or a NaN: k = 0 stays)
__host__ __device__ __forceinline__ int mse_pick(const double *E, int count) {
  int best = 0;
  for (int k = 1; k < count; ++k)
    if (E[k] < E[best]) best = k;
  return best;
}

// The end of a call, one thread: candidate `pick`'s range through the running update and
// the f64 qparams (hist_finish: observer_update and the clip record), and the pick.
__host__ __device__ __forceinline__ void mse_finish(float mn, float mx, double r, int pick, float *run_minmax,
                                                    double *qp_out, double *clip_out, int32_t *pick_out, int sym,
                                                    double qden, double eps) {
  float lo, hi;
  mse_range(mn, mx, r, &lo, &hi);
  hist_finish(lo, hi, false, run_minmax, qp_out, clip_out, sym, qden, eps);
  *pick_out = pick;
}

}  // namespace vsiq
