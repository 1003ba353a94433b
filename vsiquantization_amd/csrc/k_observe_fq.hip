// k_observe_fq.hip — per-tensor observe + qparams + fake quant fused: K8 (one workgroup),
// K9 (K2p records, then the fold in every workgroup of the fake-quant launch), K10 (K9 in one
// launch behind a grid barrier) and K1r (the multi-GPU exchange's fold + fake quant), with
// their C ABI entry points.  The observer pieces are in k_observe.cuh.
#include "dispatch.cuh"
#include "k_body.cuh"   // K1 block body (K9, K1r); includes vsiq_common.cuh
#include "k_observe.cuh"

namespace vsiq {

// ----------------------------------------------------------------------------
// K8: per-tensor observe + qparams + fake quant of a SMALL tensor in one launch.  One
// 1024-lane workgroup holds the whole tensor in registers (<= 16 groups per lane,
// 65536 elements): it reduces min / max / NaN / sums (the K2 stats record), applies the
// running update and the f64 qparams (minmax.py:42-74, qm.py:66-68) and fake-quantizes
// from registers (uniform.py:55,95) -- K2 + K1 (two launches, the qparams through
// memory) in one.  The reference's per-call observe+quantize of a small tensor
// (quantization_manager.py:73-90; a calibration call on a weight, BASELINE C1).
// ----------------------------------------------------------------------------
template <bool VEC, bool NT, int ACT, bool MASK, bool CODES, int U>
__global__ __launch_bounds__(kSmallBlock) void k_observe_fq_small(
    const float *__restrict__ x, float *__restrict__ y, uint8_t *__restrict__ codes,
    uint64_t *__restrict__ mask, int64_t n, double *__restrict__ stats_out, float *__restrict__ run_minmax,
    double *__restrict__ qp_out, int sym, double qden, double eps, float lo, float hi, SiluLay L) {
  constexpr int NW = kSmallBlock / kWave;
  __shared__ float s_mn[NW], s_mx[NW];
  __shared__ uint32_t s_nan[NW];
  __shared__ double s_sa[NW], s_s1[NW], s_s2[NW];
  __shared__ double s_qp[2];
  const int64_t ng = cdiv(n, 4);
  f4 v[U];
#pragma unroll
  for (int k = 0; k < U; ++k)
    v[k] = act_fwd4_at<ACT>(load_group_c<VEC, NT>(x, threadIdx.x + k * kSmallBlock, ng, n),
                            4 * (int64_t)(threadIdx.x + k * kSmallBlock), L);
  ObsAcc a;
  obs_init(a);
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const int64_t i = threadIdx.x + k * kSmallBlock;
    if (i < ng) obs_add4(a, v[k], valid_in_group(i, n));
  }
  obs_wave_reduce(a);
  const int w = threadIdx.x / kWave;
  if (threadIdx.x % kWave == 0) {
    s_mn[w] = a.mn; s_mx[w] = a.mx; s_nan[w] = a.nan;
    s_sa[w] = a.sa; s_s1[w] = a.s1; s_s2[w] = a.s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double f[6] = {s_mn[0], s_mx[0], (double)s_nan[0], s_sa[0], s_s1[0], s_s2[0]};
    for (int i = 1; i < NW; ++i) {   // fixed order
      f[0] = fminf((float)f[0], s_mn[i]); f[1] = fmaxf((float)f[1], s_mx[i]); f[2] += s_nan[i];
      f[3] += s_sa[i]; f[4] += s_s1[i]; f[5] += s_s2[i];
    }
    if (stats_out) write_stats(stats_out, f, n);
    observer_update((float)f[0], (float)f[1], f[2] > 0.0, run_minmax, qp_out, sym, qden, eps, &s_qp[0],
                    &s_qp[1]);
  }
  __syncthreads();
  const QP p = make_qp((float)s_qp[0], (float)s_qp[1], lo, hi, 0);
  // every load was consumed before the barrier: each group is stored as soon as it is
  // quantized (no output array held in registers, no vmcnt hazard)
  uint32_t mlo = 0, mhi = 0;
  const int lane = threadIdx.x % kWave;
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const int64_t i = threadIdx.x + k * kSmallBlock;
    const GroupOut go = fq_out_flat<VEC, CODES, MASK>(v[k], p, i, n);
    if (MASK) mask_put(mlo, mhi, k, go.b);
    if (i - lane < ng) fq_store_out<VEC, NT, CODES>(y, codes, i, ng, n, go);   // wave-uniform test
  }
  if (MASK && lane < 4 * U) {   // lane 4k+j: word j of slot k's chunk
    const int64_t first = (int64_t)threadIdx.x - lane + (lane >> 2) * kSmallBlock;
    if (first < ng) mask[4 * (first / kWave) + (lane & 3)] = ((uint64_t)mhi << 32) | mlo;
  }
}

void launch_observe_fq_small(int act, bool vec, bool nt, const float *x, float *y, uint8_t *c, uint64_t *m, int64_t n,
                             double *st, float *run, double *qp, int sym, double qden, double eps, float lo, float hi,
                             hipStream_t s) {
  const SiluLay L = act_lay(act, n);
  // groups per lane: 2 up to 8192 elements (no clamped duplicate loads), else 16
  const int u = n <= (int64_t)kSmallBlock * 2 * 4 ? 2 : kSmallGroups;
  with_act(act, [&](auto A) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      with_bool2(m != nullptr, c != nullptr, [&](auto M, auto C) {
        with_int<2, kSmallGroups>(u, [&](auto U) {
          hipLaunchKernelGGL((k_observe_fq_small<decltype(V)::value, decltype(N)::value, decltype(A)::value,
                                                 decltype(M)::value, decltype(C)::value, decltype(U)::value>),
                             dim3(1), dim3(kSmallBlock), 0, s, x, y, c, m, n, st, run, qp, sym, qden, eps, lo, hi, L);
        });
      });
    });
  });
}

// ----------------------------------------------------------------------------
// K9: per-call observe + fake quant of a mid-size tensor (K8's limit .. kFoldFqMax) in
// two launches and WITHOUT K2's cross-workgroup arrival chain (~3 us of atomics, fence
// and last-block fold at C1's 65536 elements, profiles/r02p_c1_sweep.txt).  K2p writes
// one record per wave (plain stores); then every workgroup of the fake-quant launch
// folds all of them in the same fixed order (the same bits in every workgroup), derives
// the running update and the f64 qparams itself (minmax.py:42-74) and quantizes its
// share with K1's block body (uniform.py:55,95).  Workgroup 0 alone writes the running
// state, the qparams record and the stats record (observer_update_all_blocks).
// ----------------------------------------------------------------------------
template <bool VEC, bool NT, bool CODES, bool MASK, int ACT>
__global__ __launch_bounds__(kBlock) void k_fold_fq_fwd(
    const float *__restrict__ x, float *__restrict__ y, uint8_t *__restrict__ codes,
    uint64_t *__restrict__ mask, int64_t n, const double *__restrict__ parts, int nrec,
    double *__restrict__ stats_out, float *__restrict__ run_minmax, double *__restrict__ qp_out, int sym,
    double qden, double eps, float lo, float hi, SiluLay L) {
  __shared__ double s_f[kWaves][6];
  __shared__ double s_qp[2];
  double f[6];
  fold_records_block(parts, nrec, f, s_f);
  if (threadIdx.x == 0) {
    observer_update_all_blocks(f, n, run_minmax, qp_out, stats_out, sym, qden, eps, s_qp);
  }
  __syncthreads();
  const QP p = make_qp((float)s_qp[0], (float)s_qp[1], lo, hi, 0);
  fq_fwd_block<VEC, NT, CODES, MASK, ACT, kFlatU>(x, y, codes, mask, n, p, blockIdx.x, GateClk{0}, 0u, L);
}

void launch_fold_fq(int act, bool vec, bool nt, const float *x, float *y, uint8_t *c, uint64_t *m, int64_t n,
                    double *parts, double *st, float *run, double *qp, int sym, double qden, double eps, float lo,
                    float hi, hipStream_t s) {
  const SiluLay L = act_lay(act, n);
  const int64_t pgrid = fold_fq_part_grid(n);
  const int nrec = (int)(pgrid * kWaves);
  const dim3 grid((unsigned)oneshot_grid(cdiv(n, 4)));
  launch_observe_part_fold_fq(act, vec, nt, x, n, parts, pgrid, L, s);
  with_act(act, [&](auto A) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      with_bool2(c != nullptr, m != nullptr, [&](auto C, auto M) {
        hipLaunchKernelGGL((k_fold_fq_fwd<decltype(V)::value, decltype(N)::value, decltype(C)::value,
                                          decltype(M)::value, decltype(A)::value>),
                           grid, dim3(kBlock), 0, s, x, y, c, m, n, parts, nrec, st, run, qp, sym, qden, eps, lo, hi, L);
      });
    });
  });
}

// ----------------------------------------------------------------------------
// K10: K9 in ONE launch.  The grid is K2p's (fold_fq_part_grid(n) <= 32 workgroups,
// kFoldFqU groups per lane per step, <= 2 steps up to kFoldFqMax), so every workgroup
// holds its share of act(x) in registers (<= 8 groups per lane), accumulates it in
// k_observe_part's order and stores its per-wave records write-through -- the same bits
// as K9's K2p launch.  A grid barrier on two counter words replaces the kernel
// boundary: arrive, spin (s_sleep) until every workgroup has arrived, fold all records
// in K9's fixed order, derive the running update + f64 qparams (minmax.py:42-74) and
// quantize from registers (uniform.py:55,95).  The running state is read BEFORE the
// arrival, so workgroup 0's write after the barrier cannot race a reader; the last
// workgroup to leave resets both words (stream-ordered reuse).  The grid is tiny
// (<= 32 workgroups of 256 lanes on 256 CUs): co-resident with room to spare; a
// workgroup that waits longer than kGridBarTimeout (42 ms) stops waiting, counts the
// event in counter word kGridBarErrors and writes NaN, so no wave can spin forever.
// ----------------------------------------------------------------------------
template <bool VEC, bool NT, bool CODES, bool MASK, int ACT, int S>
__global__ __launch_bounds__(kBlock) void k_observe_fq_grid(
    const float *__restrict__ x, float *__restrict__ y, uint8_t *__restrict__ codes,
    uint64_t *__restrict__ mask, int64_t n, double *__restrict__ parts, uint32_t *__restrict__ counter,
    double *__restrict__ stats_out, float *__restrict__ run_minmax, double *__restrict__ qp_out, int sym,
    double qden, double eps, float lo, float hi, SiluLay L) {
  constexpr int U = kFoldFqU;
  __shared__ double s_f[kWaves][6];
  __shared__ double s_qp[2];
  __shared__ int s_ok;
  const int64_t ng = cdiv(n, 4);
  const int64_t nfull = n / 4;
  const int64_t step = (int64_t)gridDim.x * kBlock * U;
  const int64_t b0 = (int64_t)blockIdx.x * kBlock * U;
  const int64_t base = b0 + threadIdx.x;
  const int lane = threadIdx.x % kWave, w = threadIdx.x / kWave;
  float state[2] = {0.f, 0.f};
  if (run_minmax && threadIdx.x == 0) { state[0] = run_minmax[0]; state[1] = run_minmax[1]; }
  f4 v[S * U];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int k = 0; k < U; ++k) v[s * U + k] = load_group_c<VEC, NT>(x, base + s * step + k * kBlock, ng, n);
  ObsAcc a;
  obs_init(a);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (b0 + s * step >= ng) break;   // block-uniform: observe_stride_b's loop condition
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int64_t i = base + s * step + k * kBlock;
      v[s * U + k] = act_fwd4_at<ACT>(v[s * U + k], 4 * i, L);
      if (i < nfull) obs_add4(a, v[s * U + k], 4);
      else if (i < ng) obs_add4(a, v[s * U + k], valid_in_group(i, n));
    }
  }
  // store_part_record's reductions, the record stored write-through and drained
  obs_wave_reduce(a);
  if (lane < 6) {   // the reduced fields are wave-uniform: lane k stores field k (one 48-B write)
    double *r = parts + ((int64_t)blockIdx.x * kWaves + w) * VSIQ_PART_LEN;
    const double fv = lane == 0 ? (double)a.mn : lane == 1 ? (double)a.mx : lane == 2 ? (double)a.nan
                    : lane == 3 ? a.sa : lane == 4 ? a.s1 : a.s2;
    partial_store(r + lane, fv);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  if (threadIdx.x == 0) {   // grid barrier
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(counter + kGridBarArrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t t0 = wall_clock64();
    int ok = 1;
    while (__hip_atomic_load(counter + kGridBarArrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x) {
      if (wall_clock64() - t0 > kGridBarTimeout) {
        ok = 0;
        __hip_atomic_fetch_add(counter + kGridBarErrors, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    s_ok = ok;
  }
  __syncthreads();
  // fold_records_block's fold with coherent loads and observer_update_all_blocks' sequence on the
  // state read above, spelled out: through the helpers this kernel took 2 to 11 more VGPRs
  double f[6];
  const int nrec = (int)gridDim.x * kWaves;
  ObsFold::init(f);
  for (int i = threadIdx.x; i < nrec; i += kBlock) {
    const double *r = parts + (int64_t)i * VSIQ_PART_LEN;
    const double rr[6] = {partial_load(r + 0), partial_load(r + 1), partial_load(r + 2),
                          partial_load(r + 3), partial_load(r + 4), partial_load(r + 5)};
    ObsFold::add(f, rr);
  }
  ObsFold::wave(f);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s_f[w][k] = f[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kWaves; ++i) {
      const double rr[6] = {s_f[i][0], s_f[i][1], s_f[i][2], s_f[i][3], s_f[i][4], s_f[i][5]};
      ObsFold::add(f, rr);
    }
  }
  if (threadIdx.x == 0) {
    const bool lead = blockIdx.x == 0;
    observer_update((float)f[0], (float)f[1], f[2] > 0.0, run_minmax ? state : nullptr, lead ? qp_out : nullptr,
                    sym, qden, eps, &s_qp[0], &s_qp[1]);
    if (lead) {
      if (run_minmax) { run_minmax[0] = state[0]; run_minmax[1] = state[1]; }
      if (stats_out) write_stats(stats_out, f, n);
    }
    // leave the barrier; the last workgroup out resets it for the next launch
    if (__hip_atomic_fetch_add(counter + kGridBarDepart, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
        gridDim.x - 1) {
      __hip_atomic_store(counter + kGridBarArrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(counter + kGridBarDepart, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
  const QP p = make_qp(s_ok ? (float)s_qp[0] : __builtin_nanf(""), (float)s_qp[1], lo, hi, 0);
  GroupOut go[S * U];
  uint32_t mlo = 0, mhi = 0;
#pragma unroll
  for (int sl = 0; sl < S * U; ++sl) {
    go[sl] = fq_out_flat<VEC, CODES, MASK>(v[sl], p, base + (sl / U) * step + (sl % U) * kBlock, n);
    if (MASK) mask_put(mlo, mhi, sl, go[sl].b);
  }
#pragma unroll
  for (int sl = 0; sl < S * U; ++sl) {   // group indices increase with sl
    const int64_t i = base + (sl / U) * step + (sl % U) * kBlock;
    if (i - lane >= ng) break;   // whole wave past the end (uniform)
    fq_store_out<VEC, NT, CODES>(y, codes, i, ng, n, go[sl]);
  }
  if (MASK && lane < 4 * S * U) {   // lane 4 sl + j: word j of slot sl's chunk
    const int sl = lane >> 2;
    const int64_t first = base - lane + (sl / U) * step + (sl % U) * kBlock;
    if (first < ng) mask[4 * (first / kWave) + (lane & 3)] = ((uint64_t)mhi << 32) | mlo;
  }
}

inline int observe_fq_grid_steps(int64_t n) {
  return cdiv(cdiv(n, 4), fold_fq_part_grid(n) * kBlock * kFoldFqU) <= 1 ? 1 : 2;
}

void launch_observe_fq_grid(int act, bool vec, bool nt, const float *x, float *y, uint8_t *c, uint64_t *m, int64_t n,
                            double *parts, uint32_t *counter, double *st, float *run, double *qp, int sym,
                            double qden, double eps, float lo, float hi, hipStream_t s) {
  const SiluLay L = act_lay(act, n);
  const dim3 grid((unsigned)fold_fq_part_grid(n));
  with_act(act, [&](auto A) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      with_bool2(c != nullptr, m != nullptr, [&](auto C, auto M) {
        with_int<1, 2>(observe_fq_grid_steps(n), [&](auto S) {
          hipLaunchKernelGGL((k_observe_fq_grid<decltype(V)::value, decltype(N)::value, decltype(C)::value,
                                                decltype(M)::value, decltype(A)::value, decltype(S)::value>),
                             grid, dim3(kBlock), 0, s, x, y, c, m, n, parts, counter, st, run, qp, sym, qden, eps, lo,
                             hi, L);
        });
      });
    });
  });
}

// ----------------------------------------------------------------------------
// K1r: the per-call multi-GPU observer exchange's fold + fake quant in ONE launch.  The
// ranks' stats records (one K2 pass over each rank's shard, then one all_gather, rank
// order) are folded by EVERY workgroup in rank order -- min / max exact, counts and sums
// in float64, the same bits on every rank and in every workgroup -- into the running
// update and the f64 qparams (minmax.py:42-74), and the workgroup quantizes its share
// (uniform.py:55,95).  Workgroup 0 alone writes the running state, the qparams record and
// the batch's stats record (observer_update_all_blocks).  Replaces k_observe_finalize_ranks
// + K1 (two launches, the qparams through memory) of the round-2 exchange.
// ----------------------------------------------------------------------------
template <bool VEC, bool NT, bool CODES, bool MASK, int ACT>
__global__ __launch_bounds__(kBlock) void k_ranks_fq_fwd(
    const float *__restrict__ x, float *__restrict__ y, uint8_t *__restrict__ codes,
    uint64_t *__restrict__ mask, int64_t n, const double *__restrict__ gathered, int world,
    double *__restrict__ stats_out, float *__restrict__ run_minmax, double *__restrict__ qp_out, int sym,
    double qden, double eps, float lo, float hi, SiluLay L) {
  __shared__ double s_qp[2];
  if (threadIdx.x == 0) {
    double f[6], nn;
    fold_rank_records(gathered, world, f, nn);   // k_observe_finalize_ranks' fold
    observer_update_all_blocks(f, (int64_t)nn, run_minmax, qp_out, stats_out, sym, qden, eps, s_qp);
  }
  __syncthreads();
  const QP p = make_qp((float)s_qp[0], (float)s_qp[1], lo, hi, 0);
  fq_fwd_block<VEC, NT, CODES, MASK, ACT, kFlatU>(x, y, codes, mask, n, p, blockIdx.x, GateClk{0}, 0u, L);
}

void launch_ranks_fq(int act, bool vec, bool nt, const float *x, float *y, uint8_t *c, uint64_t *m, int64_t n,
                     const double *gathered, int world, double *st, float *run, double *qp, int sym, double qden,
                     double eps, float lo, float hi, hipStream_t s) {
  const SiluLay L = act_lay(act, n);
  const dim3 grid((unsigned)oneshot_grid(cdiv(n, 4)));
  with_act(act, [&](auto A) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      with_bool2(c != nullptr, m != nullptr, [&](auto C, auto M) {
        hipLaunchKernelGGL((k_ranks_fq_fwd<decltype(V)::value, decltype(N)::value, decltype(C)::value,
                                           decltype(M)::value, decltype(A)::value>),
                           grid, dim3(kBlock), 0, s, x, y, c, m, n, gathered, world, st, run, qp, sym, qden, eps, lo,
                           hi, L);
      });
    });
  });
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int64_t vsiq_observe_fq_max_elems(void) { return kSmallMax; }

int64_t vsiq_observe_fq_parts_max_elems(void) { return kFoldFqMax; }

int vsiq_act_observe_fq_parts_f32(const float *c, float *y, void *codes, uint64_t *mask, int64_t n, int act,
                                  double *stats_out, float *run_minmax, double *qp_out, int symmetric,
                                  double qden, double eps, int qmin, int qmax, double *ws, int64_t ws_len,
                                  void *stream) {
  if (n <= 0 || n > kFoldFqMax || !c || !y || !ws || qmin > qmax || !act_ok(act))
    return VSIQ_E_ARG;
  if (ws_len < fold_fq_part_grid(n) * kWaves * VSIQ_PART_LEN) return VSIQ_E_WS;
  if (mask && !aligned8(mask)) return VSIQ_E_ALIGN;
  const bool vec = n % 4 == 0 && aligned16(c) && aligned16(y) && (!codes || aligned4(codes));
  launch_fold_fq(act, vec, g_tune.nontemporal != 0, c, y, (uint8_t *)codes, mask, n, ws, stats_out, run_minmax,
                 qp_out, symmetric, qden, eps, (float)qmin, (float)qmax, (hipStream_t)stream);
  return launch_rc();
}

int vsiq_act_observe_fq_grid_f32(const float *c, float *y, void *codes, uint64_t *mask, int64_t n, int act,
                                 double *stats_out, float *run_minmax, double *qp_out, int symmetric,
                                 double qden, double eps, int qmin, int qmax, double *ws, int64_t ws_len,
                                 uint32_t *counter, void *stream) {
  if (n <= 0 || n > kFoldFqMax || !c || !y || !ws || !counter || qmin > qmax || !act_ok(act))
    return VSIQ_E_ARG;
  if (ws_len < fold_fq_part_grid(n) * kWaves * VSIQ_PART_LEN) return VSIQ_E_WS;
  if (mask && !aligned8(mask)) return VSIQ_E_ALIGN;
  if (!aligned4(counter)) return VSIQ_E_ALIGN;
  const bool vec = n % 4 == 0 && aligned16(c) && aligned16(y) && (!codes || aligned4(codes));
  launch_observe_fq_grid(act, vec, g_tune.nontemporal != 0, c, y, (uint8_t *)codes, mask, n, ws, counter, stats_out,
                         run_minmax, qp_out, symmetric, qden, eps, (float)qmin, (float)qmax, (hipStream_t)stream);
  return launch_rc();
}

int vsiq_act_fq_fwd_ranks_f32(const float *c, float *y, void *codes, uint64_t *mask, int64_t n, int act,
                              const double *gathered, int world, double *stats_out, float *run_minmax,
                              double *qp_out, int symmetric, double qden, double eps, int qmin, int qmax,
                              void *stream) {
  if (n <= 0 || !c || !y || !gathered || world <= 0 || qmin > qmax || !act_ok(act)) return VSIQ_E_ARG;
  if (oneshot_grid(cdiv(n, 4)) > 0x7fffffffLL) return VSIQ_E_ARG;
  if (mask && !aligned8(mask)) return VSIQ_E_ALIGN;
  const bool vec = n % 4 == 0 && aligned16(c) && aligned16(y) && (!codes || aligned4(codes));
  launch_ranks_fq(act, vec, g_tune.nontemporal != 0, c, y, (uint8_t *)codes, mask, n, gathered, world, stats_out,
                  run_minmax, qp_out, symmetric, qden, eps, (float)qmin, (float)qmax, (hipStream_t)stream);
  return launch_rc();
}

int vsiq_act_observe_fq_f32(const float *c, float *y, void *codes, uint64_t *mask, int64_t n, int act,
                            double *stats_out, float *run_minmax, double *qp_out, int symmetric, double qden,
                            double eps, int qmin, int qmax, void *stream) {
  if (n <= 0 || n > kSmallMax || !c || !y || qmin > qmax || !act_ok(act))
    return VSIQ_E_ARG;
  if (mask && !aligned8(mask)) return VSIQ_E_ALIGN;
  const bool vec = n % 4 == 0 && aligned16(c) && aligned16(y) && (!codes || aligned4(codes));
  launch_observe_fq_small(act, vec, g_tune.nontemporal != 0, c, y, (uint8_t *)codes, mask, n, stats_out, run_minmax,
                          qp_out, symmetric, qden, eps, (float)qmin, (float)qmax, (hipStream_t)stream);
  return launch_rc();
}

}  // extern "C"
