// k_observe_hist.hip — the percentile observer's second pass (PercentileObserver,
// observers/percentile.py): a histogram of act(x) between the min and max K2 just wrote,
// the two bins where the tails of `tail * N` elements end, and K2's running update and f64
// qparams on that clipped range.  Counts are integers, so the result does not depend on
// the order of the atomics: device, host loop (k_host.hip) and a numpy restatement agree
// bit for bit (the arithmetic they share: k_observe_hist.cuh).
#include "k_observe_hist.cuh"
#include "k_observe_k2.cuh"

namespace vsiq {

// One element per lane into the workgroup's LDS histogram.  Lanes of a wave that hit one
// address serialise in the LDS, and real activations do: about half of a post-ReLU tensor
// is bin 0, and a range stretched by outliers puts nearly every element into a few bins.
// So the wave aggregates first: the lanes whose bin equals the first pending lane's are
// counted with one ballot and added by that lane.  It goes on while a round finds a hot
// bin (>= kHistHot lanes), at least kHistRounds rounds (the first lane may be the one cold
// lane next to a hot bin); the lanes left over add for themselves.  Spread bins cost
// kHistRounds rounds, a tensor in three bins three.
constexpr int kHistHot = 8;
#ifndef VSIQ_HIST_ROUNDS
#define VSIQ_HIST_ROUNDS 2
#endif
constexpr int kHistRounds = VSIQ_HIST_ROUNDS;

__device__ __forceinline__ void lds_count(uint32_t *h, uint32_t c) {
  __hip_atomic_fetch_add(h, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// wave-uniform control flow: call from converged code, `valid` masks the lanes
__device__ __forceinline__ void hist_add(uint32_t *s_h, int bin, bool valid) {
  bool pending = valid;
  for (int r = 0;; ++r) {
    const uint64_t pm = __ballot(pending);
    if (pm == 0) return;
    const int src = __ffsll((unsigned long long)pm) - 1;
    const int cand = __builtin_amdgcn_readlane(bin, src);
    const bool hit = pending && bin == cand;
    const int cnt = __popcll(__ballot(hit));
    if (hit && (int)__lane_id() == src) lds_count(s_h + cand, (uint32_t)cnt);
    pending = pending && !hit;
    if (cnt < kHistHot && r + 1 >= kHistRounds) break;
  }
  if (pending) lds_count(s_h + bin, 1u);
}

__device__ __forceinline__ void hist_add4(uint32_t *s_h, f4 v, int nv, const HistMap &m) {
  hist_add(s_h, hist_bin(v.x, m), nv > 0);
  hist_add(s_h, hist_bin(v.y, m), nv > 1);
  hist_add(s_h, hist_bin(v.z, m), nv > 2);
  hist_add(s_h, hist_bin(v.w, m), nv > 3);
}

// The pass: k_observe_loop's grid-stride walk (same loads, activation and tail handling),
// each workgroup counting into LDS; the workgroups then add their non-empty bins to the
// global uint64 histogram (8-byte agent atomics, drained by every wave before the arrival)
// and the last one to arrive scans it, finishes the call and leaves histogram and counter
// zero for the next stream-ordered call.  One workgroup (small tensors): no global
// histogram, no arrival.
template <bool VEC, bool NT, int ACT, int U>
__global__ __launch_bounds__(kBlock) void k_observe_hist(const float *__restrict__ x, int64_t n,
                                                          const double *__restrict__ stats, int bins, double tail,
                                                          unsigned long long *__restrict__ hist,
                                                          uint32_t *__restrict__ counter,
                                                          float *__restrict__ run_minmax,
                                                          double *__restrict__ qp_out,
                                                          double *__restrict__ clip_out, int sym, double qden,
                                                          double eps, SiluLay L) {
  __shared__ uint32_t s_h[kHistMaxBins];
  __shared__ unsigned long long s_scan[kBlock];
  __shared__ int s_b[2];
  const float mn = (float)stats[VSIQ_ST_MIN], mx = (float)stats[VSIQ_ST_MAX];
  const bool has_nan = stats[VSIQ_ST_NAN] > 0.0;
  if (hist_noclip(mn, mx, has_nan, tail)) {   // the same in every workgroup
    if (blockIdx.x == 0 && threadIdx.x == 0)
      hist_finish(mn, mx, has_nan, run_minmax, qp_out, clip_out, sym, qden, eps);
    return;
  }
  const int top = bins - 1;
  for (int i = threadIdx.x; i < bins; i += kBlock) s_h[i] = 0u;
  if (threadIdx.x == 0) { s_b[0] = 0; s_b[1] = top; }
  __syncthreads();

  const HistMap m = hist_map(mn, mx, bins);
  const int64_t ng = cdiv(n, 4);
  const int64_t nfull = n / 4;
  const int64_t step = (int64_t)gridDim.x * kBlock * U;
  for (int64_t b = (int64_t)blockIdx.x * kBlock * U; b < ng; b += step) {
    f4 v[U];
    if (VEC && b + (int64_t)kBlock * U <= nfull) {   // every group of the step is whole
      const float *xb = x + 4 * b;
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = ld4<NT>(xb + 4 * (threadIdx.x + k * kBlock));
#pragma unroll
      for (int k = 0; k < U; ++k)
        hist_add4(s_h, act_fwd4_at<ACT>(v[k], 4 * (b + threadIdx.x + k * kBlock), L), 4, m);
      continue;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = load_group_c<VEC, NT>(x, b + threadIdx.x + k * kBlock, ng, n);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = b + threadIdx.x + k * kBlock;
      hist_add4(s_h, act_fwd4_at<ACT>(v[k], 4 * (i < ng ? i : ng - 1), L), i < ng ? valid_in_group(i, n) : 0, m);
    }
  }
  __syncthreads();

  const bool single = gridDim.x == 1;
  if (!single) {
    // each workgroup starts at another bin, so the grid's adds spread over the histogram
    const int rot = (int)((blockIdx.x * (uint32_t)kBlock) & (uint32_t)top);
    for (int i = threadIdx.x; i < bins; i += kBlock) {
      const int b = (i + rot) & top;
      const uint32_t c = s_h[b];
      if (c) __hip_atomic_fetch_add(hist + b, (unsigned long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every adding wave, before the arrival
    __syncthreads();
    if (!arrive_last(counter)) return;
  }

  // the last (or only) workgroup: thread t owns bins [t * per, (t + 1) * per)
  auto count = [&](int b) -> unsigned long long {
    return single ? (unsigned long long)s_h[b] : __hip_atomic_load(hist + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  const int per = bins / kBlock, b0 = (int)threadIdx.x * per;
  unsigned long long c = 0;
  for (int j = 0; j < per; ++j) c += count(b0 + j);
  s_scan[threadIdx.x] = c;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {   // inclusive scan of the threads' counts
    const unsigned long long a = (int)threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0ull;
    __syncthreads();
    s_scan[threadIdx.x] += a;
    __syncthreads();
  }
  const unsigned long long incl = s_scan[threadIdx.x], total = s_scan[kBlock - 1];
  const unsigned long long before = incl - c, after = total - incl;
  const unsigned long long K = hist_rank(n, tail);
  if (before <= K && K < incl) {   // one thread holds bl
    unsigned long long p = before;
    for (int j = 0; j < per; ++j) {
      p += count(b0 + j);
      if (p > K) { s_b[0] = b0 + j; break; }
    }
  }
  if (after <= K && K < after + c) {   // one thread holds bh
    unsigned long long p = after;
    for (int j = per - 1; j >= 0; --j) {
      p += count(b0 + j);
      if (p > K) { s_b[1] = b0 + j; break; }
    }
  }
  __syncthreads();
  if (!single)
    for (int j = 0; j < per; ++j) __hip_atomic_store(hist + b0 + j, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x == 0) {
    float lo, hi;
    hist_clip(mn, mx, bins, s_b[0], s_b[1], &lo, &hi);
    hist_finish(lo, hi, false, run_minmax, qp_out, clip_out, sym, qden, eps);
    if (!single) *counter = 0u;   // ready for the next stream-ordered launch
  }
}

// K2's grid-stride grid (fixed per n; one workgroup up to kObsSingle groups)
inline int64_t hist_grid(int64_t ng) {
  if (ng <= kObsSingle) return 1;
  return std::min<int64_t>(kObsGrid, cdiv(ng, (int64_t)kBlock * kObsU));
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_act_observe_hist_f32(const float *c, int64_t n, int act, const double *stats, int bins, double tail,
                              uint64_t *hist, int64_t hist_len, uint32_t *counter, float *run_minmax,
                              double *qp_out, double *clip_out, int symmetric, double qden, double eps,
                              void *stream) {
  if (n <= 0 || !c || !stats || !hist || !counter || !clip_out || !act_ok(act)) return VSIQ_E_ARG;
  if (!hist_bins_ok(bins) || !hist_tail_ok(tail)) return VSIQ_E_ARG;
  if (hist_len < bins) return VSIQ_E_WS;
  const bool vec = aligned16(c) && n % 4 == 0;
  const bool nt = g_tune.nontemporal != 0 && !((n * (int64_t)sizeof(float)) >> 20 < kObsTemporalMB);
  // tail 0 clips nothing: one workgroup finishes the call from the record alone
  const dim3 grid((unsigned)(tail == 0.0 ? 1 : hist_grid(cdiv(n, 4))));
  const SiluLay L = act_lay(act, n);
  with_act(act, [&](auto A) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      hipLaunchKernelGGL((k_observe_hist<decltype(V)::value, decltype(N)::value, decltype(A)::value, kObsU>), grid,
                         dim3(kBlock), 0, (hipStream_t)stream, c, n, stats, bins, tail,
                         reinterpret_cast<unsigned long long *>(hist), counter, run_minmax, qp_out, clip_out,
                         symmetric, qden, eps, L);
    });
  });
  return launch_rc();
}

}  // extern "C"
