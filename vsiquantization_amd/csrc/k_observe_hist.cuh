// k_observe_hist.cuh — the percentile observer's arithmetic, shared by the device pass
// (k_observe_hist.hip) and the host loop (k_host.hip): which calls clip at all, the bin of
// a value, the rank K and the clipped range from the two bins found.  Everything is f64
// and never contracted (-ffp-contract=off), counts are integers, so the device, the host
// and a numpy restatement agree bit for bit.
#pragma once
#include "vsiq_common.cuh"

namespace vsiq {

constexpr int kHistMinBins = 256;    // one bin per lane of the last workgroup's scan
constexpr int kHistMaxBins = 4096;   // uint32 counts of one workgroup: 16 KB of LDS

inline bool hist_bins_ok(int bins) {
  return bins >= kHistMinBins && bins <= kHistMaxBins && (bins & (bins - 1)) == 0;
}
inline bool hist_tail_ok(double tail) { return tail >= 0.0 && tail < 0.5; }   // NaN: no

// the call is MinMaxObserver's (no histogram): a NaN call changes nothing anyway
// (minmax.py:42-47), a constant or non-finite range has no bins, tail 0 keeps every element
__host__ __device__ __forceinline__ bool hist_noclip(float mn, float mx, bool has_nan, double tail) {
  return has_nan || mn == mx || !__builtin_isfinite(mn) || !__builtin_isfinite(mx) || tail == 0.0;
}

struct HistMap {
  double mn, invw;
  int top;   // bins - 1
};

__host__ __device__ __forceinline__ HistMap hist_map(float mn, float mx, int bins) {
  const double w = (double)mx - (double)mn;
  return HistMap{(double)mn, (double)bins / w, bins - 1};
}

// bin(v) = min(B - 1, (int64)((v - mn) * invw)); v in [mn, mx], so the product is in
// [0, B].  Clamped below as well: a record that is not this tensor's cannot index outside
// the histogram.
__host__ __device__ __forceinline__ int hist_bin(float v, const HistMap &m) {
  const double d = ((double)v - m.mn) * m.invw;
  const int b = d >= (double)m.top ? m.top : (int)d;
  return b > 0 ? b : 0;
}

// K = floor(N * t): the elements each tail may drop
__host__ __device__ __forceinline__ uint64_t hist_rank(int64_t n, double tail) {
  return (uint64_t)__builtin_floor((double)n * tail);
}

// bl: the smallest bin whose inclusive prefix count exceeds K; bh: the largest whose
// inclusive suffix count does.  The clipped range never leaves [mn, mx].
__host__ __device__ __forceinline__ void hist_clip(float mn, float mx, int bins, int bl, int bh, float *lo,
                                                   float *hi) {
  const double step = ((double)mx - (double)mn) / (double)bins;
  const float cl = (float)((double)mn + (double)bl * step);
  const float ch = (float)((double)mn + (double)(bh + 1) * step);
  *lo = (bl != 0 && cl > mn) ? cl : mn;
  *hi = (bh != bins - 1 && ch < mx) ? ch : mx;
}

// The end of a percentile call, one thread: the running update and the f64 qparams of
// the clipped range (observer_update, K2's own epilogue) and the f64[2] clip record.
__host__ __device__ __forceinline__ void hist_finish(float lo, float hi, bool has_nan, float *run_minmax,
                                                     double *qp_out, double *clip_out, int sym, double qden,
                                                     double eps) {
  observer_update(lo, hi, has_nan, run_minmax, qp_out, sym, qden, eps);
  clip_out[0] = (double)lo;
  clip_out[1] = (double)hi;
}

}  // namespace vsiq
