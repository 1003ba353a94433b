// k_observe.hip — the per-tensor observer kernels: K2 (optionally over a fused ReLU / SiLU),
// K2p (records only), K2o (records + the activation written), K2m (many tensors per launch),
// the deferred fold of K2p records and the finalize kernels, with their C ABI entry points.
// The pieces they share with the observe + fake-quant fusions are in k_observe.cuh; K2's kernels
// and launcher, over the element type, in k_observe_k2.cuh (bf16 / fp16: k_observe_half.hip).
#include "k_observe_k2.cuh"

namespace vsiq {

// K2p: the grid-stride pass of k_observe_loop WITHOUT the cross-workgroup fold.  Each
// wave stores its record {min, max, nan count, sum|x|, sum x, sum x^2, n, records}
// (VSIQ_PART_LEN doubles, plain stores) and exits: no arrival atomics, no
// last-block fold, no running update.  For calibration, where nothing consumes an
// observer's result before the calibration ends: k_observe_fold_parts folds every
// call's records at once (deferred sync), and the running min/max is replayed there.
template <bool VEC, bool NT, int ACT, int U>
__global__ __launch_bounds__(kBlock) void k_observe_part(const float *__restrict__ x, int64_t n,
                                                          double *__restrict__ parts, SiluLay L) {
  ObsAcc a;
  observe_stride<VEC, NT, ACT, U>(x, n, a, L);
  store_part_record(a, parts, blockIdx.x, gridDim.x, n);
}

// ----------------------------------------------------------------------------
// K2o: a calibration forward of a fused layer in ONE pass -- y = act(c), the tensor the
// next layer consumes (modules/fused.py:133), and the deferred observer's K2p records of
// act(c) (minmax.py:42-43 + qm.py:66-68) -- instead of an activation pass that writes y
// and an observer pass that reads it again (8 instead of 12 B per element) and with
// nothing queued that user code could modify before it is observed.  Same grid, groups
// per lane and accumulation order as k_observe_part, so the records are the same bits.
// ----------------------------------------------------------------------------
template <bool VEC, bool NT, int ACT, int U>
__global__ __launch_bounds__(kBlock) void k_observe_part_out(const float *__restrict__ x, float *__restrict__ y,
                                                              int64_t n, double *__restrict__ parts, SiluLay L) {
  ObsAcc a;
  obs_init(a);
  const int64_t ng = cdiv(n, 4);
  const int64_t nfull = n / 4;
  const int64_t step = (int64_t)gridDim.x * kBlock * U;
  for (int64_t b = (int64_t)blockIdx.x * kBlock * U; b < ng; b += step) {
    f4 v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) v[k] = load_group_c<VEC, NT>(x, b + threadIdx.x + k * kBlock, ng, n);
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = b + threadIdx.x + k * kBlock;
      v[k] = act_fwd4_at<ACT>(v[k], 4 * i, L);
      if (i < nfull) obs_add4(a, v[k], 4);
      else if (i < ng) obs_add4(a, v[k], valid_in_group(i, n));
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = b + threadIdx.x + k * kBlock;
      if (i < ng) store_group<VEC, NT>(y, i, n, v[k]);
    }
  }
  store_part_record(a, parts, blockIdx.x, gridDim.x, n);
}

// K2o one-shot form (the default): workgroup b (BS lanes) takes groups
// [b*BS*G, (b+1)*BS*G) -- G loads per lane issued at once, act + observer terms in
// registers, the workgroup's record through LDS, then the G stores: no loop, so no store
// shares a vmcnt wait with a later load (a grid-stride step waits for its own stores
// before the next step's loads can be consumed: hipcc's s_waitcnt treats mixed load /
// store counts as out of order).  One record per WORKGROUP (k2o_records(n)); the block
// reduction runs before the stores (no fence between the y stores and the barrier).
// Measured on MI355X (profiles/r04b_k2o_*): G = 2 streams best at every C5 size (52M
// elements: 68.1 us = 0.77 of 8 TB/s, vs 76.8 us at G = 16 and 96 % of the activation
// alone); BS trades the record count (the sync's fold) against the tail.  `gate`: the
// one-round G = 9 form's store gate (round 5, launch_k2o_gated; 0 = none), like K1's.
template <bool VEC, bool NT, int ACT, int G, int BS>
__global__ __launch_bounds__(BS) void k_observe_part_out1(const float *__restrict__ x, float *__restrict__ y,
                                                           int64_t n, double *__restrict__ parts, SiluLay L,
                                                           uint32_t gate) {
  const GateClk gc = gate_begin(gate);
  constexpr int NW = BS / kWave;
  __shared__ float s_mn[NW], s_mx[NW];
  __shared__ uint32_t s_nan[NW];
  __shared__ double s_sa[NW], s_s1[NW], s_s2[NW];
  const int64_t ng = cdiv(n, 4);
  const int64_t nfull = n / 4;
  const int64_t base = (int64_t)blockIdx.x * BS * G;
  ObsAcc a;
  obs_init(a);
  f4 v[G];
  const bool whole = VEC && base + (int64_t)BS * G <= nfull;   // block-uniform
  if (whole) {
    const float *xb = x + 4 * base;
#pragma unroll
    for (int k = 0; k < G; ++k) v[k] = ld4<NT>(xb + 4 * (threadIdx.x + k * BS));
#pragma unroll
    for (int k = 0; k < G; ++k) {
      v[k] = act_fwd4_at<ACT>(v[k], 4 * (base + threadIdx.x + k * BS), L);
      obs_add4(a, v[k], 4);
    }
  } else {
#pragma unroll
    for (int k = 0; k < G; ++k) v[k] = load_group_c<VEC, NT>(x, base + threadIdx.x + k * BS, ng, n);
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const int64_t i = base + threadIdx.x + k * BS;
      v[k] = act_fwd4_at<ACT>(v[k], 4 * i, L);
      if (i < nfull) obs_add4(a, v[k], 4);
      else if (i < ng) obs_add4(a, v[k], valid_in_group(i, n));
    }
  }
  obs_wave_reduce(a);
  const int w = threadIdx.x / kWave;
  if (threadIdx.x % kWave == 0) {
    s_mn[w] = a.mn; s_mx[w] = a.mx; s_nan[w] = a.nan;
    s_sa[w] = a.sa; s_s1[w] = a.s1; s_s2[w] = a.s2;
  }
  __syncthreads();
  gate_pass(gate, gc);
  if (whole) {
    float *yb = y + 4 * base;
#pragma unroll
    for (int k = 0; k < G; ++k) st4<NT>(yb + 4 * (threadIdx.x + k * BS), v[k]);
  } else {
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const int64_t i = base + threadIdx.x + k * BS;
      if (i < ng) store_group<VEC, NT>(y, i, n, v[k]);
    }
  }
  if (threadIdx.x == 0) {   // waves in order: fixed per n
    double f[6] = {s_mn[0], s_mx[0], (double)s_nan[0], s_sa[0], s_s1[0], s_s2[0]};
    for (int i = 1; i < NW; ++i) {
      f[0] = fminf((float)f[0], s_mn[i]); f[1] = fmaxf((float)f[1], s_mx[i]); f[2] += s_nan[i];
      f[3] += s_sa[i]; f[4] += s_s1[i]; f[5] += s_s2[i];
    }
    double *r = parts + (int64_t)blockIdx.x * VSIQ_PART_LEN;
    r[0] = f[0]; r[1] = f[1]; r[2] = f[2]; r[3] = f[3];
    r[4] = f[4]; r[5] = f[5]; r[6] = (double)n; r[7] = (double)gridDim.x;
  }
}

template <int ACT, int U>
void launch_observe_part_u(bool vec, bool nt, const float *x, int64_t n, double *parts, int64_t grid,
                           const SiluLay &L, hipStream_t st) {   // K2p launch at U groups per lane per step
  with_vec_nt(vec, nt, [&](auto V, auto N) {
    hipLaunchKernelGGL((k_observe_part<decltype(V)::value, decltype(N)::value, ACT, U>), dim3((unsigned)grid),
                       dim3(kBlock), 0, st, x, n, parts, L);
  });
}

void launch_observe_part_fold_fq(int act, bool vec, bool nt, const float *x, int64_t n, double *parts, int64_t grid,
                                 const SiluLay &L, hipStream_t st) {
  with_act(act, [&](auto A) { launch_observe_part_u<decltype(A)::value, kFoldFqU>(vec, nt, x, n, parts, grid, L, st); });
}

// ----------------------------------------------------------------------------
// K2m: many deferred observer calls (K2p) in ONE launch.  Block b of the launch runs
// block b - blk0[t] of tensor t's own K2p grid (same grid, groups per lane and body as
// vsiq_act_observe_part_f32 for that n), so every tensor's records are bit-identical
// to its single-tensor K2p launch; only the ~3 us launch floor and the grid tail are
// paid once per batch instead of once per layer (C5: 27 layers per calibration batch).
// ----------------------------------------------------------------------------
constexpr int kPartMulti = 32;   // tensors per launch (descriptor table in the kernel arguments)

struct PTensor {
  const float *x;
  double *parts;
  int64_t n;
  uint32_t grid;
  int u;      // groups per lane per step (observe_part_u)
  int vec;
};

struct PBatch {
  PTensor t[kPartMulti];
  uint32_t blk0[kPartMulti + 1];
  int count;
  SiluRef sref;   // SiLU: the reference CPU layout (each tensor's chunks from its own n)
};

// ALLVEC: every tensor of the batch takes the 16-byte path (the usual case: activation
// tensors of n % 4 == 0), so the scalar-path variants, which set the register budget
// of the generic kernel (152 VGPRs: 3 waves per SIMD), are not compiled in.
template <bool NT, int ACT, bool ALLVEC>
__global__ __launch_bounds__(kBlock) void k_observe_part_multi(const PBatch b) {
  int t = 0;
  const uint32_t blk = blockIdx.x;
  while (t + 1 < b.count && blk >= b.blk0[t + 1]) ++t;   // scalar: blk0 is a kernel argument
  const PTensor &T = b.t[t];
  const int64_t lb = (int64_t)blk - b.blk0[t], nb = T.grid;
  SiluLay L{};
  if constexpr (ACT == kActSilu) L = silu_lay(T.n, b.sref);
  ObsAcc a;
  if (ALLVEC || T.vec) {
    if (T.u == 8) observe_stride_b<true, NT, ACT, 8>(T.x, T.n, a, lb, nb, L);
    else if (T.u == 4) observe_stride_b<true, NT, ACT, 4>(T.x, T.n, a, lb, nb, L);
    else observe_stride_b<true, NT, ACT, 2>(T.x, T.n, a, lb, nb, L);
  } else {
    if (T.u == 8) observe_stride_b<false, false, ACT, 8>(T.x, T.n, a, lb, nb, L);
    else if (T.u == 4) observe_stride_b<false, false, ACT, 4>(T.x, T.n, a, lb, nb, L);
    else observe_stride_b<false, false, ACT, 2>(T.x, T.n, a, lb, nb, L);
  }
  store_part_record(a, T.parts, lb, nb, T.n);
}

// Fold of deferred K2p records: workgroup c folds call c's records (call_stride doubles
// apart; the count is the grid stored in every record) in a fixed order -> its stats
// record (VSIQ_ST_LEN).  Deterministic; min/max exact, sums in float64.
__global__ __launch_bounds__(kBlock) void k_observe_fold_parts(const double *__restrict__ parts,
                                                               int64_t call_stride,
                                                               double *__restrict__ stats_out) {
  const double *P = parts + (int64_t)blockIdx.x * call_stride;
  const int64_t maxrec = call_stride / VSIQ_PART_LEN;
  const double dg = P[7], dn = P[6];
  // a slot that was never written (or garbage) folds nothing instead of reading out of range
  const int64_t nrec = (dg >= 1.0 && dg <= (double)maxrec) ? (int64_t)dg : 0;
  double f[6];
  ObsFold::init(f);
  // thread t folds records t, t + 256, t + 512, ... in that order; kFoldU of them are loaded
  // at once (a one-shot K2o call has up to n / 2048 records: one load round trip per
  // record would make the sync latency-bound)
  constexpr int kFoldU = 8;
  for (int64_t i0 = threadIdx.x; i0 < nrec; i0 += (int64_t)kBlock * kFoldU) {
    double rr[kFoldU][6];
#pragma unroll
    for (int u = 0; u < kFoldU; ++u) {
      const int64_t i = i0 + (int64_t)u * kBlock;
      const double *r = P + (i < nrec ? i : nrec - 1) * VSIQ_PART_LEN;
#pragma unroll
      for (int k = 0; k < 6; ++k) rr[u][k] = r[k];
    }
#pragma unroll
    for (int u = 0; u < kFoldU; ++u)
      if (i0 + (int64_t)u * kBlock < nrec) ObsFold::add(f, rr[u]);
  }
  __shared__ double s_f[kWaves][6];
  fold_waves<ObsFold>(f, s_f);
  if (threadIdx.x == 0) write_stats(stats_out + (int64_t)blockIdx.x * VSIQ_ST_LEN, f, nrec ? (int64_t)dn : 0);
}

// Finalize from an externally reduced stats record (multi-GPU: stats all-reduced
// over RCCL with MAX on [-min, max] and SUM on the counts, then this 1-lane kernel).
__global__ void k_observe_finalize(const double *__restrict__ stats, float *__restrict__ run_minmax,
                                   double *__restrict__ qp_out, int sym, double qden, double eps) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  observer_update((float)stats[VSIQ_ST_MIN], (float)stats[VSIQ_ST_MAX], stats[VSIQ_ST_NAN] > 0.0,
                  run_minmax, qp_out, sym, qden, eps);
}

// Per-call multi-GPU observer exchange, the fold side: `world` stats records gathered
// from the ranks (all_gather, rank order) -> the whole batch's record (min / max exact,
// counts and sums in float64 in rank order: the same bits on every rank) -> fp32 means /
// std (qm.py:66-68) -> running update + f64 qparams (minmax.py:42-74).  One launch
// instead of two all-reduces plus the host-side finish of round 1.
__global__ void k_observe_finalize_ranks(const double *__restrict__ gathered, int world,
                                         double *__restrict__ stats_out, float *__restrict__ run_minmax,
                                         double *__restrict__ qp_out, int sym, double qden, double eps) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double f[6], n;
  fold_rank_records(gathered, world, f, n);
  if (stats_out) write_stats(stats_out, f, (int64_t)n);
  observer_update((float)f[0], (float)f[1], f[2] > 0.0, run_minmax, qp_out, sym, qden, eps);
}

void launch_observe_part(int act, bool vec, bool nt, const float *x, int64_t n, double *parts, int64_t grid,
                         hipStream_t st) {
  const SiluLay L = act_lay(act, n);
  with_act(act, [&](auto A) {
    with_int<8, 4, 2>(observe_part_u(n), [&](auto U) {
      launch_observe_part_u<decltype(A)::value, decltype(U)::value>(vec, nt, x, n, parts, grid, L, st);
    });
  });
}

void launch_k2o1(int act, bool vec, bool nt, int g, int bs, int64_t grid, const float *c, float *y, int64_t n,
                 double *parts, const SiluLay &L, hipStream_t st) {
  with_act(act, [&](auto A) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      with_int<1024, 512, 256>(bs, [&](auto BS) {
        with_int<1, 2, 4, 8, 16>(g, [&](auto G) {
          hipLaunchKernelGGL((k_observe_part_out1<decltype(V)::value, decltype(N)::value, decltype(A)::value,
                                                  decltype(G)::value, decltype(BS)::value>),
                             dim3((unsigned)grid), dim3(decltype(BS)::value), 0, st, c, y, n, parts, L, 0u);
        });
      });
    });
  });
}

// K2o's one-round forms (round 5): where 9 groups per lane of 256 lanes make a grid of
// 2..occ workgroups per CU (every workgroup resident at once; on MI355X 4.7M..18.9M
// elements -- C5's 6.6M / 13M layers), one pass of loads, the record, the store gate
// (tuned online per site like K1's, gate_tune.hip), then the stores: reads and writes as
// two phases instead of interleaved.  Smaller calls whose default 2-groups-per-lane grid
// is one round (C5's 1.6M / 3.3M layers) get the gate on that grid.  The form is chosen
// by the shape alone (not by the gate), so a call's records are fixed per n; the gate
// is only a delay.  Records: one per workgroup, never more than the G = 2 form's that
// size the slot (k2o_records).
template <int ACT, bool VEC, bool NT, int G>
bool launch_k2o_gated_g(const float *c, float *y, int64_t n, double *parts, const SiluLay &L, hipStream_t st) {
  constexpr int kBS = 256;
  const int64_t ng = cdiv(n, 4);
  const int64_t grid = cdiv(ng, (int64_t)kBS * G);
  const void *kern = reinterpret_cast<const void *>(k_observe_part_out1<VEC, NT, ACT, G, kBS>);
  static const int occ = occupancy_blocks(kern, kBS);
  const int64_t cus = device_cus();
  if (grid < 2 * cus || grid > (int64_t)occ * cus || grid * kBS * G - ng > ng / 8) return false;
  GateSel gs = store_gate_select("k2o_observe_out", kern, grid, occ, 4 * n, st);
  hipLaunchKernelGGL((k_observe_part_out1<VEC, NT, ACT, G, kBS>), dim3((unsigned)grid), dim3(kBS), 0, st, c, y, n,
                     parts, L, gs.gate);
  store_gate_launched(gs, st);
  return true;
}

bool launch_k2o_gated(int act, bool vec, bool nt, const float *c, float *y, int64_t n, double *parts, const SiluLay &L,
                      hipStream_t st) {
  static_assert(kK2oGroups == 2 && kK2oBlock == 256, "the G = 2 gated form is the default grid");
  return with_act(act, [&](auto A) {
    return with_vec_nt(vec, nt, [&](auto V, auto N) {
      constexpr int kA = decltype(A)::value;
      constexpr bool kV = decltype(V)::value, kN = decltype(N)::value;
      // (a 16-groups form is not one round at 26M: 5 workgroups per CU by its registers)
      return launch_k2o_gated_g<kA, kV, kN, 2>(c, y, n, parts, L, st) ||
             launch_k2o_gated_g<kA, kV, kN, 9>(c, y, n, parts, L, st);
    });
  });
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_observe_f32(const float *x, int64_t n, double *stats_out, float *run_minmax,
                     double *qp_out, int symmetric, double qden, double eps, double *ws,
                     int64_t ws_len, uint32_t *counter, void *stream) {
  return observe<float>(x, n, kActNone, stats_out, run_minmax, qp_out, symmetric, qden, eps, ws, ws_len,
                 counter, stream);
}

int vsiq_act_observe_f32(const float *c, int64_t n, int act, double *stats_out, float *run_minmax,
                         double *qp_out, int symmetric, double qden, double eps, double *ws,
                         int64_t ws_len, uint32_t *counter, void *stream) {
  if (!act_ok(act)) return VSIQ_E_ARG;
  return observe<float>(c, n, act, stats_out, run_minmax, qp_out, symmetric, qden, eps, ws, ws_len, counter,
                        stream);
}

int vsiq_act_observe_t(const void *c, int64_t n, int dtype, int act, double *stats_out, float *run_minmax,
                       double *qp_out, int symmetric, double qden, double eps, double *ws,
                       int64_t ws_len, uint32_t *counter, void *stream) {
  if (!dtype_ok(dtype)) return VSIQ_E_ARG;
  if (n == 0) return 0;
  return with_dtype(dtype, [&](auto D) {
    using T = typename decltype(D)::type;
    return observe<T>((const T *)c, n, act, stats_out, run_minmax, qp_out, symmetric, qden, eps, ws, ws_len,
                      counter, stream);
  });
}

int64_t vsiq_observe_part_records(int64_t n) {
  if (n <= 0) return VSIQ_E_ARG;
  return observe_part_grid(n) * kWaves;
}

int vsiq_act_observe_part_f32(const float *c, int64_t n, int act, double *parts, int64_t parts_len,
                              void *stream) {
  if (n <= 0 || !c || !parts || !act_ok(act)) return VSIQ_E_ARG;
  const int64_t grid = observe_part_grid(n);
  if (parts_len < grid * kWaves * VSIQ_PART_LEN) return VSIQ_E_WS;
  const bool vec = aligned16(c) && n % 4 == 0;
  launch_observe_part(act, vec, g_tune.nontemporal != 0, c, n, parts, grid, (hipStream_t)stream);
  return launch_rc();
}

int64_t vsiq_observe_part_out_records(int64_t n) {
  if (n <= 0) return VSIQ_E_ARG;
  return k2o_records(n);
}

int vsiq_act_observe_part_out_f32(const float *c, float *y, int64_t n, int act, double *parts, int64_t parts_len,
                                  void *stream) {
  if (n <= 0 || !c || !y || !parts || !act_ok(act)) return VSIQ_E_ARG;
  const bool vec = aligned16(c) && aligned16(y) && n % 4 == 0;
  const bool nt = g_tune.nontemporal != 0;
  const SiluLay L = act_lay(act, n);
  const hipStream_t st = (hipStream_t)stream;
  if (g_tune.k2o_form != 1) {
    const int64_t grid = k2o_records(n);
    if (grid > 0x7fffffffLL) return VSIQ_E_ARG;
    if (parts_len < grid * VSIQ_PART_LEN) return VSIQ_E_WS;
    // default shape knobs: the one-round gated form where the size allows it
    if (g_tune.k2o_groups == 0 && g_tune.k2o_block == 0 && launch_k2o_gated(act, vec, nt, c, y, n, parts, L, st))
      return launch_rc();
    launch_k2o1(act, vec, nt, k2o_groups(), k2o_block(), grid, c, y, n, parts, L, st);
    return launch_rc();
  }
  const int64_t grid = observe_part_grid(n);
  if (parts_len < grid * kWaves * VSIQ_PART_LEN) return VSIQ_E_WS;
  with_act(act, [&](auto A) {
    with_int<8, 4, 2>(observe_part_u(n), [&](auto U) {
      with_vec_nt(vec, nt, [&](auto V, auto N) {
        hipLaunchKernelGGL((k_observe_part_out<decltype(V)::value, decltype(N)::value, decltype(A)::value,
                                               decltype(U)::value>),
                           dim3((unsigned)grid), dim3(kBlock), 0, st, c, y, n, parts, L);
      });
    });
  });
  return launch_rc();
}

int vsiq_act_observe_part_multi_f32(const vsiq_part_tensor *tensors, int count, int act, void *stream) {
  if (count < 0 || (count > 0 && !tensors) || !act_ok(act)) return VSIQ_E_ARG;
  for (int i = 0; i < count; ++i) {
    const vsiq_part_tensor &T = tensors[i];
    if (T.n <= 0 || !T.c || !T.parts) return VSIQ_E_ARG;
    if (T.parts_len < observe_part_grid(T.n) * kWaves * VSIQ_PART_LEN) return VSIQ_E_WS;
  }
  const bool nt = g_tune.nontemporal != 0;
  for (int i0 = 0; i0 < count; i0 += kPartMulti) {
    PBatch b{};
    b.count = std::min(kPartMulti, count - i0);
    b.sref = act_ref(act);
    uint32_t blk = 0;
    for (int k = 0; k < b.count; ++k) {
      const vsiq_part_tensor &T = tensors[i0 + k];
      PTensor &P = b.t[k];
      P.x = T.c;
      P.parts = T.parts;
      P.n = T.n;
      P.grid = (uint32_t)observe_part_grid(T.n);
      P.u = observe_part_u(T.n);
      P.vec = aligned16(T.c) && T.n % 4 == 0;
      b.blk0[k] = blk;
      blk += P.grid;
    }
    b.blk0[b.count] = blk;
    const hipStream_t st = (hipStream_t)stream;
    bool allvec = true;
    for (int k = 0; k < b.count; ++k) allvec = allvec && b.t[k].vec;
    with_act(act, [&](auto A) {
      with_bool2(nt, allvec, [&](auto N, auto AV) {
        hipLaunchKernelGGL((k_observe_part_multi<decltype(N)::value, decltype(A)::value, decltype(AV)::value>),
                           dim3(blk), dim3(kBlock), 0, st, b);
      });
    });
    const int rc = launch_rc();
    if (rc) return rc;
  }
  return 0;
}

int vsiq_observe_fold_parts(const double *parts, int64_t ncalls, int64_t call_stride, double *stats_out,
                            void *stream) {
  if (ncalls < 0 || ncalls > 0x7fffffffLL) return VSIQ_E_ARG;
  if (ncalls == 0) return 0;
  if (!parts || !stats_out || call_stride < VSIQ_PART_LEN) return VSIQ_E_ARG;
  hipLaunchKernelGGL(k_observe_fold_parts, dim3((unsigned)ncalls), dim3(kBlock), 0, (hipStream_t)stream,
                     parts, call_stride, stats_out);
  return launch_rc();
}

int vsiq_observe_finalize(const double *stats, float *run_minmax, double *qp_out, int symmetric,
                          double qden, double eps, void *stream) {
  if (!stats) return VSIQ_E_ARG;
  hipLaunchKernelGGL(k_observe_finalize, dim3(1), dim3(kWave), 0, (hipStream_t)stream, stats,
                     run_minmax, qp_out, symmetric, qden, eps);
  return launch_rc();
}

int vsiq_observe_finalize_ranks(const double *gathered, int world, double *stats_out, float *run_minmax,
                                double *qp_out, int symmetric, double qden, double eps, void *stream) {
  if (!gathered || world <= 0) return VSIQ_E_ARG;
  hipLaunchKernelGGL(k_observe_finalize_ranks, dim3(1), dim3(kWave), 0, (hipStream_t)stream, gathered, world,
                     stats_out, run_minmax, qp_out, symmetric, qden, eps);
  return launch_rc();
}

}  // extern "C"
