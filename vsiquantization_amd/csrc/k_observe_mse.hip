// k_observe_mse.hip — the MSE observer's second pass (MSEObserver, observers/mse.py): for
// each of K candidate ranges r[k] * (min, max) of the record K2 just wrote, the summed
// squared error of fake-quantizing act(x) with that range's qparams; the range of the
// smallest error then goes through K2's running update and f64 qparams.  One read of the
// tensor serves all K candidates: the kernel is VALU-bound, not HBM-bound.
// Per-element values are fixed by the definition (include/vsiq.h; the arithmetic shared
// with the host loop: k_observe_mse.cuh), the f64 sums have a fixed order per (n, K): no
// floating-point atomics, the same bits run to run.
#include "k_observe_k2.cuh"
#include "k_observe_mse.cuh"

namespace vsiq {

// candidate flags (wave-uniform, read with the candidate's parameters)
constexpr uint32_t kMseValid = 1u, kMseFast = 2u;

__device__ __forceinline__ float lane_f32(float v, int lane) {
  return u2f((uint32_t)__builtin_amdgcn_readlane((int)f2u(v), lane));
}

// One lane's sum of the error terms of its U groups for one candidate.  IEEE: fq_elem's
// division; else fq_elem_fast (the candidate passed fq_fast_qp and every element of the
// wave's step fq_x_ok: the same y bit for bit).  TAIL: bit 4k + j of `vm` says element j
// of group k exists.
template <bool IEEE, bool TAIL, int U>
__device__ __forceinline__ double mse_part(const f4 (&v)[U], const QP &p, uint32_t vm) {
  double a = 0.0;
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const float x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float y = IEEE ? fq_elem<true>(x[j], p).y : fq_elem_fast(x[j], p).y;
      const double t = mse_term(y, x[j]);
      a += (TAIL && !((vm >> (4 * k + j)) & 1u)) ? 0.0 : t;
    }
  }
  return a;
}

// Lane l of every wave holds the parameters of candidates l and l + 64 (ps / pr / pz /
// pf: scale, its reciprocal, zero point, flags) and the wave's error sums of those two
// (acc).  One step: the wave's U groups per lane against every candidate in turn, the
// candidate's parameters read into SGPRs, the lanes' partial sums reduced on DPP and
// added by the lane that owns the candidate.
template <bool TAIL, int U>
__device__ __forceinline__ void mse_step(const f4 (&v)[U], uint32_t vm, int count, const float (&ps)[2],
                                         const float (&pr)[2], const float (&pz)[2], const uint32_t (&pf)[2],
                                         float qlo, float qhi, double (&acc)[2]) {
  uint32_t ok = 1u;
#pragma unroll
  for (int k = 0; k < U; ++k) ok &= fq_x_ok(v[k].x) & fq_x_ok(v[k].y) & fq_x_ok(v[k].z) & fq_x_ok(v[k].w);
  const bool xfast = __ballot(!ok) == 0;
  const int lane = threadIdx.x % kWave;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {   // (one copy of the loop body: selects, not two unrolled halves)
    const float hs = h ? ps[1] : ps[0], hr = h ? pr[1] : pr[0], hz = h ? pz[1] : pz[0];
    const uint32_t hf = h ? pf[1] : pf[0];
    const int kn = count - h * kWave < kWave ? count - h * kWave : kWave;
    double own = 0.0;   // this step's sum of the candidate this lane owns
    for (int kk = 0; kk < kn; ++kk) {
      const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)hf, kk);
      if (!(f & kMseValid)) continue;   // its error is +inf whatever the tensor holds
      QP p;
      p.s = lane_f32(hs, kk);
      p.z = lane_f32(hz, kk);
      p.lo = qlo;
      p.hi = qhi;
      p.discrete = 0;
      p.d.b = p.s;
      p.d.r = lane_f32(hr, kk);
      p.d.fast = p.fast = (f & kMseFast) ? 1u : 0u;
      double part;
      if (xfast && p.fast) part = mse_part<false, TAIL, U>(v, p, vm);   // wave-uniform branch
      else part = mse_part<true, TAIL, U>(v, p, vm);
      const double red = wave_reduce(part, AddD());
      own = lane == kk ? red : own;
    }
    acc[0] += h ? 0.0 : own;
    acc[1] += h ? own : 0.0;
  }
}

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
