// k_gptq.cuh — GPTQ for group-wise weights: what the kernels of k_gptq.hip and the host loop of
// k_host.hip share.  include/vsiq.h states the arithmetic (vsiq_pg_gptq_f32).
#pragma once
#include <stdint.h>

#include "vsiq_common.cuh"

namespace vsiq {

constexpr int kGptqBlock = 128;   // columns quantized between two trailing updates; the error strip's width

inline bool gptq_group_ok(int64_t group) { return group == 32 || group == 64 || group == 128; }

// sizes the entry points accept: whole groups, and row / column counts the launch grids hold
inline bool gptq_sizes_ok(int64_t rows, int64_t rowlen, int64_t group) {
  return gptq_group_ok(group) && rows > 0 && rowlen > 0 && rowlen % group == 0 && rows <= 0x7fffffffLL &&
         rowlen <= (1LL << 24);
}

// A fresh group's running (min, max): what vsiq_pg_observe_fq_f32's update leaves of the 0 / 0
// state -- strict compares from 0, and a group holding a NaN changes nothing.  Compare-selects,
// so the result does not depend on the order the elements are fed in (a -0.0 never replaces 0).
struct GptqRange {
  float lo = 0.0f, hi = 0.0f;
  bool nan = false;
};

__host__ __device__ __forceinline__ void gptq_range_add(GptqRange &r, float x) {
  r.nan |= x != x;
  r.lo = x < r.lo ? x : r.lo;
  r.hi = x > r.hi ? x : r.hi;
}

__host__ __device__ __forceinline__ void gptq_group_qparams(const GptqRange &r, int sym, double qden, double eps,
                                                            double *scale, double *zp) {
  minmax_qparams(r.nan ? 0.0 : (double)r.lo, r.nan ? 0.0 : (double)r.hi, sym, qden, eps, scale, zp);
}

}  // namespace vsiq
