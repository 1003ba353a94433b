// k_observe_mse.hip — the MSE observer's second pass (MSEObserver, observers/mse.py): for
// each of K candidate ranges r[k] * (min, max) of the record K2 just wrote, the summed
// squared error of fake-quantizing act(x) with that range's qparams; the range of the
// smallest error then goes through K2's running update and f64 qparams.  One read of the
// tensor serves all K candidates: the kernel is VALU-bound, not HBM-bound.
// Per-element values are fixed by the definition (include/vsiq.h; the arithmetic shared
// with the host loop: k_observe_mse.cuh), the f64 sums have a fixed order per (n, K): no
// floating-point atomics, the same bits run to run.
#include "k_observe_k2.cuh"
#include "k_mse_step.cuh"

namespace vsiq {

template <bool VEC, bool NT, int ACT, int U>
__global__ __launch_bounds__(kBlock) void k_observe_mse(const float *__restrict__ x, int64_t n,
                                                         const double *__restrict__ stats, MseRatios R, int count,
                                                         float qlo, float qhi, double *__restrict__ ws,
                                                         uint32_t *__restrict__ counter,
                                                         float *__restrict__ run_minmax,
                                                         double *__restrict__ qp_out,
                                                         double *__restrict__ clip_out,
                                                         double *__restrict__ err_out,
                                                         int32_t *__restrict__ pick_out, int sym, double qden,
                                                         double eps, SiluLay L) {
  __shared__ double s_w[kWaves][kMseMaxCand];
  __shared__ double s_e[kMseMaxCand];
  const float mn = (float)stats[VSIQ_ST_MIN], mx = (float)stats[VSIQ_ST_MAX];
  const bool has_nan = stats[VSIQ_ST_NAN] > 0.0;
  if (mse_fallback(mn, mx, has_nan, count)) {   // the same in every workgroup
    if (blockIdx.x == 0) {
      for (int k = threadIdx.x; k < count; k += kBlock) err_out[k] = __builtin_inf();
      if (threadIdx.x == 0) {
        hist_finish(mn, mx, has_nan, run_minmax, qp_out, clip_out, sym, qden, eps);
        *pick_out = 0;
      }
    }
    return;
  }

  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  float ps[2], pr[2], pz[2];
  uint32_t pf[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + h * kWave;
    const MseCand c = mse_candidate(mn, mx, R.r[k < count ? k : 0], sym, qden, eps);
    const QP p = make_qp(c.s, c.z, qlo, qhi, 0);
    ps[h] = p.s;
    pr[h] = p.d.r;
    pz[h] = p.z;
    pf[h] = (k < count && c.valid) ? (kMseValid | (p.fast ? kMseFast : 0u)) : 0u;
  }
  double acc[2] = {0.0, 0.0};

  const int64_t ng = cdiv(n, 4);
  const int64_t nfull = n / 4;
  const int64_t step = (int64_t)gridDim.x * kBlock * U;
  for (int64_t b = (int64_t)blockIdx.x * kBlock * U; b < ng; b += step) {
    f4 v[U];
    const bool whole = b + (int64_t)kBlock * U <= nfull;   // every group of the step is whole
    if (VEC && whole) {
      const float *xb = x + 4 * b;
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = ld4<NT>(xb + 4 * (threadIdx.x + k * kBlock));
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = load_group_c<VEC, NT>(x, b + threadIdx.x + k * kBlock, ng, n);
    }
    uint32_t vm = 0u;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = b + threadIdx.x + k * kBlock;
      v[k] = act_fwd4_at<ACT>(v[k], 4 * (i < ng ? i : ng - 1), L);
      if (!whole) vm |= ((1u << (i < ng ? valid_in_group(i, n) : 0)) - 1u) << (4 * k);
    }
    if (whole) mse_step<false, U>(v, vm, count, ps, pr, pz, pf, qlo, qhi, acc);
    else mse_step<true, U>(v, vm, count, ps, pr, pz, pf, qlo, qhi, acc);
  }

  // the workgroup's sums: waves in order, candidate k in thread k
  s_w[wave][lane] = acc[0];
  s_w[wave][lane + kWave] = acc[1];
  __syncthreads();
  const int k = threadIdx.x;
  const bool mine = k < count;
  const bool valid = ((k < kWave ? pf[0] : pf[1]) & kMseValid) != 0u;   // candidate k: this lane's own
  double e = 0.0;
  if (mine) {
    for (int w = 0; w < kWaves; ++w) e += s_w[w][k];
    if (!valid) e = __builtin_inf();
  }
  const bool single = gridDim.x == 1;
  if (!single) {
    // one f64[count] record per workgroup in its own slot; the last workgroup to arrive
    // adds the records in workgroup order
    if (mine) partial_store(ws + (int64_t)blockIdx.x * count + k, e);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave, before the arrival
    __syncthreads();
    if (!arrive_last(counter)) return;
    if (mine) {
      const double *col = ws + k;
      const int nb = (int)gridDim.x;
      e = 0.0;
      for (int b0 = 0; b0 < nb; b0 += 8) {   // 8 loads in flight, added in order
        double r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = partial_load(col + (int64_t)(b0 + u < nb ? b0 + u : nb - 1) * count);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (b0 + u < nb) e += r[u];
      }
    }
  }
  if (mine) {
    s_e[k] = e;
    err_out[k] = e;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int pick = mse_pick(s_e, count);
    mse_finish(mn, mx, R.r[pick], pick, run_minmax, qp_out, clip_out, pick_out, sym, qden, eps);
    if (!single) *counter = 0u;   // ready for the next stream-ordered launch
  }
}

// K2's grid-stride grid (fixed per n; one workgroup up to kObsSingle groups)
inline int64_t mse_grid(int64_t ng) {
  if (ng <= kObsSingle) return 1;
  return std::min<int64_t>(kObsGrid, cdiv(ng, (int64_t)kBlock * kObsU));
}

inline int64_t mse_ws_doubles(int64_t n, int count) {
  const int64_t grid = mse_grid(cdiv(n, 4));
  return grid > 1 ? grid * count : 0;
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int64_t vsiq_observe_mse_ws_doubles(int64_t n, int count) {
  if (n <= 0 || count < 1 || count > kMseMaxCand) return 0;
  return mse_ws_doubles(n, count);
}

int vsiq_act_observe_mse_f32(const float *c, int64_t n, int act, const double *stats, const double *ratios, int count,
                             int qmin, int qmax, double *ws, int64_t ws_len, uint32_t *counter, float *run_minmax,
                             double *qp_out, double *clip_out, double *err_out, int32_t *pick_out, int symmetric,
                             double qden, double eps, void *stream) {
  if (n <= 0 || !c || !stats || !ws || !counter || !clip_out || !err_out || !pick_out || !act_ok(act))
    return VSIQ_E_ARG;
  if (!mse_ratios_ok(ratios, count) || qmin >= qmax) return VSIQ_E_ARG;
  if (ws_len < mse_ws_doubles(n, count)) return VSIQ_E_WS;
  MseRatios R{};
  for (int k = 0; k < count; ++k) R.r[k] = ratios[k];
  const bool vec = aligned16(c) && n % 4 == 0;
  const bool nt = g_tune.nontemporal != 0 && !((n * (int64_t)sizeof(float)) >> 20 < kObsTemporalMB);
  // one candidate searches nothing: one workgroup finishes the call from the record alone
  const dim3 grid((unsigned)(count == 1 ? 1 : mse_grid(cdiv(n, 4))));
  const SiluLay L = act_lay(act, n);
  with_act(act, [&](auto A) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      hipLaunchKernelGGL((k_observe_mse<decltype(V)::value, decltype(N)::value, decltype(A)::value, kObsU>), grid,
                         dim3(kBlock), 0, (hipStream_t)stream, c, n, stats, R, count, (float)qmin, (float)qmax, ws,
                         counter, run_minmax, qp_out, clip_out, err_out, pick_out, symmetric, qden, eps, L);
    });
  });
  return launch_rc();
}

}  // extern "C"
