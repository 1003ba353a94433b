// k_observe.cuh — the per-tensor observer's device pieces, shared by the observer kernels
// (k_observe.hip: K2, K2p, K2o, K2m, the deferred fold, the finalize kernels) and the
// observe + fake-quant fusions (k_observe_fq.hip: K8, K9, K10, K1r).  Every form promises
// records that are fixed per n and that agree bit for bit across forms: the accumulation,
// the wave reduction and the folds over records are written once, here
// (tests/test_gpu_observer_bits.py pins every form's bits).
#pragma once
#include "vsiq_common.cuh"

namespace vsiq {

// per-lane accumulator: min, max, NaN count, sum|x|, sum x, sum x^2
struct ObsAcc {
  float mn, mx;
  uint32_t nan;
  double sa, s1, s2;
};

__device__ __forceinline__ void obs_init(ObsAcc &a) {
  a.mn = __builtin_inff();
  a.mx = -__builtin_inff();
  a.nan = 0;
  a.sa = a.s1 = a.s2 = 0.0;
}

// fminf/fmaxf skip NaN operands; NaNs are counted separately.  nv valid lanes.
__device__ __forceinline__ void obs_add4(ObsAcc &a, f4 v, int nv) {
  if (nv < 4) {   // tail group: replicate element 0 for min/max, zero for the sums
    const float z0 = v.x;
    v.y = nv > 1 ? v.y : z0;
    v.z = nv > 2 ? v.z : z0;
    v.w = nv > 3 ? v.w : z0;
  }
  a.mn = fminf(fminf(a.mn, v.x), fminf(fminf(v.y, v.z), v.w));
  a.mx = fmaxf(fmaxf(a.mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
  const float wy = nv > 1 ? 1.f : 0.f, wz = nv > 2 ? 1.f : 0.f, ww = nv > 3 ? 1.f : 0.f;
  a.nan += (v.x != v.x) + (nv > 1 && v.y != v.y) + (nv > 2 && v.z != v.z) + (nv > 3 && v.w != v.w);
  // fp32 partial over the 4 lanes of the group, float64 across groups
  const float vy = v.y * wy, vz = v.z * wz, vw = v.w * ww;   // NaN*0 stays NaN: sums go NaN, fine
  const float pa = (__builtin_fabsf(v.x) + __builtin_fabsf(vy)) +
                   (__builtin_fabsf(vz) + __builtin_fabsf(vw));
  const float p1 = (v.x + vy) + (vz + vw);
  const float p2 = (v.x * v.x + vy * vy) + (vz * vz + vw * vw);   // fp32 over 4, f64 across groups
  a.sa += (double)pa;
  a.s1 += (double)p1;
  a.s2 += (double)p2;
}

// the wave's accumulators -> the wave's, in every lane (DPP only)
__device__ __forceinline__ void obs_wave_reduce(ObsAcc &a) {
  a.mn = wave_reduce(a.mn, MinOp());
  a.mx = wave_reduce(a.mx, MaxOp());
  a.nan = wave_reduce(a.nan, AddU());
  a.sa = wave_reduce(a.sa, AddD());
  a.s1 = wave_reduce(a.s1, AddD());
  a.s2 = wave_reduce(a.s2, AddD());
}

// folds over records {min, max, nan count, sum|x|, sum x, sum x^2}
struct ObsFold {
  static constexpr int K = 6;
  __device__ static void init(double (&a)[6]) {
    a[0] = __builtin_inf(); a[1] = -__builtin_inf();
    a[2] = a[3] = a[4] = a[5] = 0.0;
  }
  __device__ static void add(double (&a)[6], const double (&r)[6]) {
    a[0] = __builtin_fmin(a[0], r[0]); a[1] = __builtin_fmax(a[1], r[1]);
    a[2] += r[2]; a[3] += r[3]; a[4] += r[4]; a[5] += r[5];
  }
  __device__ static void wave(double (&a)[6]) {
    a[0] = wave_reduce(a[0], MinD()); a[1] = wave_reduce(a[1], MaxD());
#pragma unroll
    for (int k = 2; k < 6; ++k) a[k] = wave_reduce(a[k], AddD());
  }
};

// The fold of `nrec` K2p records by one 256-lane workgroup, in thread 0's `f`: thread t
// folds records t, t + 256, ... in that order, then fold_waves -- k_observe_fold_parts'
// order (its 8-deep load loop) and K10's (coherent loads), so all hold the same bits.
__device__ __forceinline__ void fold_records_block(const double *__restrict__ parts, int nrec, double (&f)[6],
                                                   double (&s_f)[kWaves][6]) {
  ObsFold::init(f);
  for (int i = threadIdx.x; i < nrec; i += kBlock) {
    const double *r = parts + (int64_t)i * VSIQ_PART_LEN;
    const double rr[6] = {r[0], r[1], r[2], r[3], r[4], r[5]};
    ObsFold::add(f, rr);
  }
  fold_waves<ObsFold>(f, s_f);
}

// `world` stats records gathered from the ranks (all_gather, rank order) -> the whole
// batch's record and element count: min / max exact, counts and sums in float64 in rank
// order, the same bits on every rank, in every workgroup and in both kernels that fold.
__device__ __forceinline__ void fold_rank_records(const double *__restrict__ gathered, int world, double (&f)[6],
                                                  double &n) {
  ObsFold::init(f);
  n = 0.0;
  for (int r = 0; r < world; ++r) {
    const double *g = gathered + (int64_t)r * VSIQ_ST_LEN;
    const double rr[6] = {g[VSIQ_ST_MIN], g[VSIQ_ST_MAX], g[VSIQ_ST_NAN], g[VSIQ_ST_SUMABS], g[VSIQ_ST_SUM],
                          g[VSIQ_ST_SUMSQ]};
    ObsFold::add(f, rr);
    n += g[VSIQ_ST_N];
  }
}

// ----------------------------------------------------------------------------
// The running update when EVERY workgroup of a fake-quant launch holds the call's folded
// record `f` (K9, K1r; K10 spells the same sequence out, its state read before its grid
// barrier): each derives the running update and the f64 qparams itself
// (minmax.py:42-74; s_qp = {scale, zero point}) from a copy of the running state, and
// workgroup 0 alone writes the state, the qparams record and the stats record.  The
// update is idempotent (min / max; a NaN call changes nothing, minmax.py:42-47), so a
// workgroup that reads the state after workgroup 0 has written it computes the same
// qparams.  Thread 0 only.
// ----------------------------------------------------------------------------
__device__ __forceinline__ void observer_update_all_blocks(const double (&f)[6], int64_t n,
                                                           float *__restrict__ run_minmax,
                                                           double *__restrict__ qp_out,
                                                           double *__restrict__ stats_out, int sym, double qden,
                                                           double eps, double (&s_qp)[2]) {
  float state[2] = {0.f, 0.f};
  if (run_minmax) { state[0] = run_minmax[0]; state[1] = run_minmax[1]; }
  const bool lead = blockIdx.x == 0;
  observer_update((float)f[0], (float)f[1], f[2] > 0.0, run_minmax ? state : nullptr, lead ? qp_out : nullptr, sym,
                  qden, eps, &s_qp[0], &s_qp[1]);
  if (lead) {
    if (run_minmax) { run_minmax[0] = state[0]; run_minmax[1] = state[1]; }
    if (stats_out) write_stats(stats_out, f, n);
  }
}

// K2: the workgroup's accumulators -> thread 0's (waves in order through LDS).  K2o's
// one-shot form and K8 write the same fold out at their own workgroup sizes: a shared LDS
// struct cost K2 up to 6 VGPRs and K8 up to 24 B of scratch (profiles/README.md, r08).
__device__ __forceinline__ void obs_block_reduce(ObsAcc &a) {
  __shared__ float s_mn[kWaves], s_mx[kWaves];
  __shared__ uint32_t s_nan[kWaves];
  __shared__ double s_sa[kWaves], s_s1[kWaves], s_s2[kWaves];
  obs_wave_reduce(a);
  const int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
  if (l == 0) {
    s_mn[w] = a.mn; s_mx[w] = a.mx; s_nan[w] = a.nan;
    s_sa[w] = a.sa; s_s1[w] = a.s1; s_s2[w] = a.s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kWaves; ++i) {
      a.mn = fminf(a.mn, s_mn[i]); a.mx = fmaxf(a.mx, s_mx[i]); a.nan += s_nan[i];
      a.sa += s_sa[i]; a.s1 += s_s1[i]; a.s2 += s_s2[i];
    }
  }
  __syncthreads();
}

// Block partial -> workspace record; the workgroup holding the fold of every record
// writes the stats record and applies the running update.
__device__ __forceinline__ void observe_epilogue(ObsAcc &a, int64_t n, double *__restrict__ stats_out,
                                                 float *__restrict__ run_minmax,
                                                 double *__restrict__ qp_out, int sym, double qden,
                                                 double eps, double *__restrict__ ws,
                                                 uint32_t *__restrict__ counter) {
  obs_block_reduce(a);
  double f[6];
  if (gridDim.x == 1) {   // one workgroup (small tensors): no records, no arrival
    f[0] = a.mn; f[1] = a.mx; f[2] = (double)a.nan; f[3] = a.sa; f[4] = a.s1; f[5] = a.s2;
    if (threadIdx.x == 0) {
      if (stats_out) write_stats(stats_out, f, n);
      observer_update((float)f[0], (float)f[1], f[2] > 0.0, run_minmax, qp_out, sym, qden, eps);
    }
    return;
  }
  if (threadIdx.x == 0) {
    double *r = ws + (int64_t)blockIdx.x * kPartials;
    partial_store(r + 0, a.mn); partial_store(r + 1, a.mx); partial_store(r + 2, (double)a.nan);
    partial_store(r + 3, a.sa); partial_store(r + 4, a.s1); partial_store(r + 5, a.s2);
  }
  if (!fold_arrivals<ObsFold>(ws, counter, f)) return;
  if (threadIdx.x == 0) {
    if (stats_out) write_stats(stats_out, f, n);
    observer_update((float)f[0], (float)f[1], f[2] > 0.0, run_minmax, qp_out, sym, qden, eps);
    *counter = 0u;   // ready for the next stream-ordered launch
  }
}

// Grid-stride accumulation of a fixed grid over x (U groups per lane per step): the
// body shared by k_observe_loop and k_observe_part.
// Block `blk` of an `nblk`-block grid over x (the multi-tensor K2m runs the same body
// on its tensors' block ranges).
template <bool VEC, bool NT, int ACT, int U, typename T = float>
__device__ __forceinline__ void observe_stride_b(const T *__restrict__ x, int64_t n, ObsAcc &a,
                                                 int64_t blk, int64_t nblk, const SiluLay &L) {
  obs_init(a);
  const int64_t ng = cdiv(n, 4);
  const int64_t nfull = n / 4;
  const int64_t step = nblk * kBlock * U;
  for (int64_t b = blk * kBlock * U; b < ng; b += step) {
    f4 v[U];
    if (VEC && b + (int64_t)kBlock * U <= nfull) {
      // every group of this step is whole (block-uniform): one uniform base pointer and
      // 32-bit lane offsets (no per-group 64-bit clamp / address arithmetic: -16 VGPRs,
      // -40 instructions per step at U = 8), straight-line, no per-group exec-mask
      // branches (they were ~1/3 of the K2p instruction stream)
      const T *xb = x + 4 * b;
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = ld4<NT>(xb + 4 * (threadIdx.x + k * kBlock));
#pragma unroll
      for (int k = 0; k < U; ++k) obs_add4(a, act_fwd4_at<ACT>(v[k], 4 * (b + threadIdx.x + k * kBlock), L), 4);
      continue;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = load_group_c<VEC, NT>(x, b + threadIdx.x + k * kBlock, ng, n);
    if (b + (int64_t)kBlock * U <= nfull) {
#pragma unroll
      for (int k = 0; k < U; ++k) obs_add4(a, act_fwd4_at<ACT>(v[k], 4 * (b + threadIdx.x + k * kBlock), L), 4);
    } else {
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int64_t i = b + threadIdx.x + k * kBlock;
        if (i < nfull) obs_add4(a, act_fwd4_at<ACT>(v[k], 4 * i, L), 4);
        else if (i < ng) obs_add4(a, act_fwd4_at<ACT>(v[k], 4 * i, L), valid_in_group(i, n));
      }
    }
  }
}

// One K2p record per WAVE (DPP reductions only): no LDS round trip and no barrier in
// the tail of the grid (C5 observe phase 263 -> 253-258 us on MI355X).  Record {min, max, nan count, sum|x|, sum x, sum x^2, n,
// records} of wave w of block blk.
__device__ __forceinline__ void store_part_record(ObsAcc &a, double *__restrict__ parts, int64_t blk,
                                                  int64_t nblk, int64_t n) {
  obs_wave_reduce(a);
  if (threadIdx.x % kWave == 0) {
    double *r = parts + (blk * kWaves + threadIdx.x / kWave) * VSIQ_PART_LEN;
    r[0] = a.mn; r[1] = a.mx; r[2] = (double)a.nan; r[3] = a.sa;
    r[4] = a.s1; r[5] = a.s2; r[6] = (double)n; r[7] = (double)nblk * kWaves;
  }
}

// sizes and grids that more than one file needs (all fixed per n: deterministic)
// K8: one 1024-lane workgroup holds the whole tensor in registers, <= 16 groups per lane
constexpr int kSmallBlock = 1024;
constexpr int kSmallGroups = 16;
constexpr int64_t kSmallMax = (int64_t)kSmallBlock * kSmallGroups * 4;

constexpr int kK2oGroups = 2;                  // K2o one-shot: groups per lane (default)
constexpr int kK2oBlock = 256;                 // K2o one-shot: lanes per workgroup (default)
constexpr int kFoldFqGrid = 32;                 // K9 / K10's K2p workgroups: <= 128 records per fold
constexpr int kFoldFqU = 4;                     // K9 / K10's K2p groups per lane per step
constexpr int64_t kFoldFqMax = (int64_t)1 << 18;   // largest n (fq grid <= 128 workgroups)

// K10's grid barrier: counter words (after arrive_last's 0..32)
constexpr int kGridBarArrive = 1 + kArriveGroups;
constexpr int kGridBarDepart = 2 + kArriveGroups;
constexpr int kGridBarErrors = 3 + kArriveGroups;
static_assert(kGridBarErrors < VSIQ_COUNTER_WORDS, "counter words");
static_assert(kGridBarErrors == VSIQ_COUNTER_GRID_ERRORS, "include/vsiq.h names this word");
constexpr uint64_t kGridBarTimeout = 1ull << 22;    // wall-clock ticks (100 MHz)

// K2p groups per lane per step: 8 while the grid reaches 512 workgroups, else fewer so
// that small layers still spread over >= ~512 workgroups (all CUs issuing; a 1.6M-
// element layer at 8 per lane was 200 workgroups).  Fixed per n: deterministic.
inline int observe_part_u(int64_t n) {
  const int64_t units = cdiv(cdiv(n, 4), (int64_t)kBlock);   // lanes' worth of groups
  return units >= 512 * 8 ? 8 : (units >= 512 * 4 ? 4 : 2);
}

// K2p grid (fixed per n), at most VSIQ_PART_MAX_RECORDS / kWaves workgroups (a record per wave)
inline int64_t observe_part_grid(int64_t n) {
  const int64_t units = cdiv(cdiv(n, 4), (int64_t)kBlock);
  const int u = observe_part_u(n);
  // large tensors: kObsGrid workgroups striding over the tensor; small: one step each
  static_assert(kObsGrid <= VSIQ_PART_MAX_RECORDS / kWaves, "K2p records");
  const int64_t cap = u == 8 ? kObsGrid : VSIQ_PART_MAX_RECORDS / kWaves;
  return std::min<int64_t>(cap, std::max<int64_t>(1, cdiv(units, u)));
}

// K9 / K10's K2p grid
inline int64_t fold_fq_part_grid(int64_t n) {
  const int64_t units = cdiv(cdiv(n, 4), (int64_t)kBlock);
  return std::min<int64_t>(kFoldFqGrid, std::max<int64_t>(1, cdiv(units, kFoldFqU)));
}

// K2o one-shot shape: G groups per lane (k2o_groups knob, default 2) and BS lanes per
// workgroup (k2o_block knob, default kK2oBlock); fixed per n and knobs: deterministic
inline int k2o_groups() {
  const int t = g_tune.k2o_groups;
  return t ? t : kK2oGroups;
}

inline int k2o_block() {
  const int t = g_tune.k2o_block;
  return t ? t : kK2oBlock;
}

inline int64_t k2o_records(int64_t n) {
  if (g_tune.k2o_form == 1) return observe_part_grid(n) * kWaves;
  return cdiv(cdiv(n, 4), (int64_t)k2o_block() * k2o_groups());
}

// K9's first launch: K2p over x at kFoldFqU groups per lane per step on `grid`
// workgroups (k_observe.hip, where k_observe_part is instantiated)
void launch_observe_part_fold_fq(int act, bool vec, bool nt, const float *x, int64_t n, double *parts, int64_t grid,
                                 const SiluLay &L, hipStream_t st);

}  // namespace vsiq
