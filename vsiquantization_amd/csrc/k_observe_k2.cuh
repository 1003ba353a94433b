// k_observe_k2.cuh — K2, the per-call per-tensor observer: its kernels, launcher and argument
// checks, over the element type T of the observed tensor.  k_observe.hip instantiates fp32
// (and holds the deferred forms and the C ABI); k_observe_half.hip instantiates bf16 / fp16.
// The grid, the accumulation order and the folds depend on n only, so a 16-bit tensor's
// record holds the bits of the fp32 call on the widened values.
#pragma once
#include "dispatch.cuh"
#include "k_observe.cuh"

namespace vsiq {

// K2: per-tensor observer (min, max, NaN count, sum|x|, sum x, sum x^2).
template <bool VEC, bool NT, int ACT, int U, typename T>
__device__ __forceinline__ void observe_stride(const T *__restrict__ x, int64_t n, ObsAcc &a,
                                               const SiluLay &L) {
  observe_stride_b<VEC, NT, ACT, U>(x, n, a, blockIdx.x, gridDim.x, L);
}

// One-shot: G groups per lane (grid = ng / (256 G)), all G loads issued up front
// (no loop: the loads of a wave stay in flight together and s_waitcnt is exact).
template <bool VEC, bool NT, int ACT, int G, typename T>
__device__ __forceinline__ void observe_oneshot(const T *__restrict__ x, int64_t n, double *__restrict__ stats_out,
                                                float *__restrict__ run_minmax, double *__restrict__ qp_out,
                                                int sym, double qden, double eps, double *__restrict__ ws,
                                                uint32_t *__restrict__ counter, const SiluLay &L) {
  ObsAcc a;
  obs_init(a);
  const int64_t ng = cdiv(n, 4);
  const int64_t base = (int64_t)blockIdx.x * kBlock * G + threadIdx.x;
  f4 v[G];
#pragma unroll
  for (int k = 0; k < G; ++k) v[k] = load_group_c<VEC, NT>(x, base + k * kBlock, ng, n);
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const int64_t i = base + k * kBlock;
    if (i < ng) obs_add4(a, act_fwd4_at<ACT>(v[k], 4 * i, L), valid_in_group(i, n));
  }
  observe_epilogue(a, n, stats_out, run_minmax, qp_out, sym, qden, eps, ws, counter);
}

// (the fp32 kernels keep their names and signatures: kernel traces name them; the _t
// kernels are the same bodies on a 16-bit tensor)
template <bool VEC, bool NT, int ACT, int G>
__global__ __launch_bounds__(kBlock) void k_observe(const float *__restrict__ x, int64_t n,
                                                    double *__restrict__ stats_out,
                                                    float *__restrict__ run_minmax,
                                                    double *__restrict__ qp_out, int sym,
                                                    double qden, double eps,
                                                    double *__restrict__ ws,
                                                    uint32_t *__restrict__ counter, SiluLay L) {
  observe_oneshot<VEC, NT, ACT, G>(x, n, stats_out, run_minmax, qp_out, sym, qden, eps, ws, counter, L);
}

template <typename T, bool VEC, bool NT, int ACT, int G>
__global__ __launch_bounds__(kBlock) void k_observe_t(const T *__restrict__ x, int64_t n,
                                                      double *__restrict__ stats_out,
                                                      float *__restrict__ run_minmax,
                                                      double *__restrict__ qp_out, int sym, double qden,
                                                      double eps, double *__restrict__ ws,
                                                      uint32_t *__restrict__ counter, SiluLay L) {
  observe_oneshot<VEC, NT, ACT, G>(x, n, stats_out, run_minmax, qp_out, sym, qden, eps, ws, counter, L);
}

// Grid-stride: a fixed grid (at most kObsGrid workgroups, independent of the device, so
// the accumulation order is fixed per n) walks the tensor U groups per lane per step.
// A pure read (no stores share vmcnt with the loads), latency hidden by the other
// waves of the CU.  Fewer, longer-lived workgroups than the one-shot form: fewer
// partial records to fold and arrivals to serialize (MI355X, C5 layer sizes:
// 52M elements 53.2 -> 38.6 us, 1.6M 10.1 -> 9.4 us).
template <bool VEC, bool NT, int ACT, int U>
__global__ __launch_bounds__(kBlock) void k_observe_loop(const float *__restrict__ x, int64_t n,
                                                          double *__restrict__ stats_out,
                                                          float *__restrict__ run_minmax,
                                                          double *__restrict__ qp_out, int sym,
                                                          double qden, double eps,
                                                          double *__restrict__ ws,
                                                          uint32_t *__restrict__ counter, SiluLay L) {
  ObsAcc a;
  observe_stride<VEC, NT, ACT, U>(x, n, a, L);
  observe_epilogue(a, n, stats_out, run_minmax, qp_out, sym, qden, eps, ws, counter);
}

template <typename T, bool VEC, bool NT, int ACT, int U>
__global__ __launch_bounds__(kBlock) void k_observe_loop_t(const T *__restrict__ x, int64_t n,
                                                           double *__restrict__ stats_out,
                                                           float *__restrict__ run_minmax,
                                                           double *__restrict__ qp_out, int sym,
                                                           double qden, double eps,
                                                           double *__restrict__ ws,
                                                           uint32_t *__restrict__ counter, SiluLay L) {
  ObsAcc a;
  observe_stride<VEC, NT, ACT, U>(x, n, a, L);
  observe_epilogue(a, n, stats_out, run_minmax, qp_out, sym, qden, eps, ws, counter);
}

template <typename T, bool VEC, bool NT, int ACT, int G>
constexpr auto observe_kernel() {
  if constexpr (std::is_same_v<T, float>) return &k_observe<VEC, NT, ACT, G>;
  else return &k_observe_t<T, VEC, NT, ACT, G>;
}

template <typename T, bool VEC, bool NT, int ACT, int U>
constexpr auto observe_loop_kernel() {
  if constexpr (std::is_same_v<T, float>) return &k_observe_loop<VEC, NT, ACT, U>;
  else return &k_observe_loop_t<T, VEC, NT, ACT, U>;
}

// K2 grid: grid-stride kernel (default) or the one-shot kernel (VSIQ_TUNE_OBS_KERNEL 1)
// Tensors of at most kObsSingle groups (8K elements: one load round per lane) take ONE
// workgroup and skip the record / arrival / fold chain.  (At 64K elements a single
// workgroup's 8 serial load rounds cost more than the chain: 12.5 vs 6.8 us, MI355X.)
constexpr int64_t kObsSingle = (int64_t)kBlock * kObsU;
// K2 (per-call observer) reads tensors under this many MB with cached loads: the fake
// quant re-reading it right after may hit the 256 MB Infinity Cache
constexpr int64_t kObsTemporalMB = 256;

// one-shot K2 has 2 / 4 / 16 groups-per-lane instances: K4's 8 runs as 4
inline int obs_groups_per_lane(int64_t ng) {
  const int p = lsq_groups_per_lane(ng);
  return p == 8 ? 4 : p;
}

inline int64_t observe_grid(int64_t ng) {
  if (g_tune.obs_kernel == 1) return lsq_grid(ng, obs_groups_per_lane(ng));
  if (ng <= kObsSingle) return 1;
  return std::min<int64_t>(kObsGrid, std::max<int64_t>(1, cdiv(ng, (int64_t)kBlock * kObsU)));
}

template <typename T>
void launch_observe(int act, bool vec, bool nt, const T *x, int64_t n, double *stats_out, float *run_minmax,
                    double *qp_out, int sym, double qden, double eps, double *ws, uint32_t *counter, hipStream_t st) {
  const SiluLay L = act_lay(act, n);
  const int64_t ng = cdiv(n, 4);
  const dim3 grid((unsigned)observe_grid(ng));
  with_act(act, [&](auto A) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      if (g_tune.obs_kernel != 1) {
        hipLaunchKernelGGL((observe_loop_kernel<T, decltype(V)::value, decltype(N)::value, decltype(A)::value, kObsU>()),
                           grid, dim3(kBlock), 0, st, x, n, stats_out, run_minmax, qp_out, sym, qden, eps, ws, counter,
                           L);
        return;
      }
      // one-shot: K4's groups-per-lane rule (8 -> 4) and grid
      with_int<kLsqGroups, 4, 2>(obs_groups_per_lane(ng), [&](auto G) {
        hipLaunchKernelGGL((observe_kernel<T, decltype(V)::value, decltype(N)::value, decltype(A)::value,
                                           decltype(G)::value>()),
                           grid, dim3(kBlock), 0, st, x, n, stats_out, run_minmax, qp_out, sym, qden, eps, ws, counter,
                           L);
      });
    });
  });
}

template <typename T>
int observe(const T *x, int64_t n, int act, double *stats_out, float *run_minmax, double *qp_out,
            int symmetric, double qden, double eps, double *ws, int64_t ws_len, uint32_t *counter,
            void *stream) {
  if (n <= 0 || !x || !ws || !counter || !act_ok(act)) return VSIQ_E_ARG;
  const bool vec = aligned_vec<T>(x) && n % 4 == 0;
  const int64_t grid = observe_grid(cdiv(n, 4));
  if (grid > 0x7fffffffLL) return VSIQ_E_ARG;
  if (ws_len < fold_records(grid) * kPartials) return VSIQ_E_WS;
  // kObsTemporalMB: observe + quantize (K2 -> K1) may re-read x from the Infinity Cache
  const bool nt = g_tune.nontemporal != 0 && !((n * (int64_t)sizeof(T)) >> 20 < kObsTemporalMB);
  launch_observe(act, vec, nt, x, n, stats_out, run_minmax, qp_out, symmetric, qden, eps, ws, counter,
                 (hipStream_t)stream);
  return launch_rc();
}

#define VSIQ_OBSERVE_INST(T)                                                                              \
  template int observe<T>(const T *, int64_t, int, double *, float *, double *, int, double, double, double *, \
                          int64_t, uint32_t *, void *)
extern VSIQ_OBSERVE_INST(bf16_t);
extern VSIQ_OBSERVE_INST(f16_t);

}  // namespace vsiq
