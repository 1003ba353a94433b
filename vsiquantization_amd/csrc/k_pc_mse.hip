// k_pc_mse.hip — the per-channel MSE observer (PerChannelMSEObserver, observers/
// per_channel_mse.py): row c of a [rows, rowlen] view is the per-tensor search of
// k_observe_mse.hip on W[c] alone -- the row's own min / max / NaN flag, K candidate ranges,
// every candidate's summed squared error, the pick, the running update of (run_min[c],
// run_max[c]), the f64 qparams and optionally the fake-quantized row -- in ONE launch and one
// read of the tensor: a row never spans workgroups, so there is no workspace and no arrival
// counter.  The arithmetic is the per-tensor pass's (k_observe_mse.cuh, k_mse_step.cuh); the
// order of a row's f64 sums is fixed per (rowlen, count): the same bits run to run.
//
// Three forms, chosen on the host by rowlen alone:
//   wave   rowlen <= kPcMseWaveMax: a wave holds its row in registers, kWaves rows per
//          workgroup, no LDS and no barrier (a wave past the last row just leaves);
//   block  rowlen <= kPcMseBlockMax: a workgroup holds its row in registers, wave w the
//          contiguous groups [w * G, (w + 1) * G), the waves' sums added in wave order;
//   long   beyond: three passes over the row (min / max, search, quantize), the later two
//          served from L2 like k_pc_observe_fq_long.
// A search step scores kPcMseU groups per lane (one step of the short wave form: 1); a step
// whose groups all lie past the row end is skipped, one with a ragged end takes the masked
// step.  Every barrier of the block / long forms is reached by every thread: whether the row
// falls back to min / max is decided after the barrier that publishes the row's min / max,
// the same in every thread.
#include "dispatch.cuh"
#include "k_mse_step.cuh"
#include "k_pc.cuh"

namespace vsiq {

constexpr int kPcMseU = 3;             // groups per lane of one search step
constexpr int kPcMseWaveChunks = 2;    // wave form: up to this many steps hold a row
constexpr int kPcMseBlockChunks = 4;   // block form: up to this many steps per wave hold a row
constexpr int64_t kPcMseWaveShort = 4 * kWave;                                    // one group per lane
constexpr int64_t kPcMseWaveMax = 4 * kWave * kPcMseU * kPcMseWaveChunks;          // elements
constexpr int64_t kPcMseBlockMax = 4 * kBlock * kPcMseU * kPcMseBlockChunks;       // elements

struct PcMseArgs {
  int64_t rows, rowlen;
  int count;
  float *run_min, *run_max;
  double *scale_out, *zp_out;
  double *clip_out;    // [rows][2]
  double *err_out;     // [rows][count] (nullable)
  int32_t *pick_out;   // [rows]
  double *row_stats;   // [rows][3] (nullable)
  int sym;
  float lo, hi;
  double qden, eps;
};

__device__ __forceinline__ double lane_f64(double v, int lane) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// a lane's share of its row's min / max / NaN flag (and sums): group i of the row
struct PcRowAcc {
  float mn, mx;
  uint32_t nan;
  RowSums rs;
};

__device__ __forceinline__ PcRowAcc pc_rowacc() {
  return PcRowAcc{__builtin_inff(), -__builtin_inff(), 0u, RowSums{0.0, 0.0, 0.0}};
}

template <bool VEC>
__device__ __forceinline__ void pc_rowacc_add(PcRowAcc &r, f4 w, int64_t i, int64_t ng, int64_t rowlen, bool stats) {
  if (i >= ng) return;   // (a clamped load: the last group again)
  r.mn = fminf(r.mn, fminf(fminf(w.x, w.y), fminf(w.z, w.w)));   // invalid tail lanes replicate element 0
  r.mx = fmaxf(r.mx, fmaxf(fmaxf(w.x, w.y), fmaxf(w.z, w.w)));
  r.nan |= (w.x != w.x) | (w.y != w.y) | (w.z != w.z) | (w.w != w.w);
  if (stats) rowsums_add4(r.rs, w, VEC ? 4 : valid_in_group(i, rowlen));
}

// Lane l's two candidates l and l + 64 of the row's (mn, mx), as the per-tensor kernel
// builds them.
__device__ __forceinline__ void pc_mse_cands(float mn, float mx, const MseRatios &R, const PcMseArgs &a,
                                             float (&ps)[2], float (&pr)[2], float (&pz)[2], uint32_t (&pf)[2]) {
  const int lane = threadIdx.x % kWave;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = lane + h * kWave;
    const MseCand c = mse_candidate(mn, mx, R.r[k < a.count ? k : 0], a.sym, a.qden, a.eps);
    const QP p = make_qp(c.s, c.z, a.lo, a.hi, 0);
    ps[h] = p.s;
    pr[h] = p.d.r;
    pz[h] = p.z;
    pf[h] = (k < a.count && c.valid) ? (kMseValid | (p.fast ? kMseFast : 0u)) : 0u;
  }
}

// One search step of a wave: its U groups i0 + k * 64 + lane (i0 wave-uniform).  Skipped
// when the whole step lies past the row end; masked when its end is ragged.
template <int U>
__device__ __forceinline__ void pc_mse_chunk(const f4 (&v)[U], int64_t i0, int64_t ng, int64_t rowlen, int count,
                                             const float (&ps)[2], const float (&pr)[2], const float (&pz)[2],
                                             const uint32_t (&pf)[2], float qlo, float qhi, double (&acc)[2]) {
  if (i0 >= ng) return;
  if (4 * (i0 + (int64_t)U * kWave) <= rowlen) {
    mse_step<false, U>(v, 0u, count, ps, pr, pz, pf, qlo, qhi, acc);
    return;
  }
  const int lane = threadIdx.x % kWave;
  uint32_t vm = 0u;
#pragma unroll
  for (int k = 0; k < U; ++k) vm |= ((1u << valid_in_group(i0 + k * kWave + lane, rowlen)) - 1u) << (4 * k);
  mse_step<true, U>(v, vm, count, ps, pr, pz, pf, qlo, qhi, acc);
}

// The end of a row, computed by every thread that calls it (only `writer` stores): the
// picked candidate's range -- or the row's min / max when the row fell back -- through the
// running update of (run_min[row], run_max[row]) and the f64 qparams (hist_finish).  Returns
// the element parameters of the row's fake quant, as K3 builds them.
__device__ __forceinline__ QP pc_mse_finish(float mn, float mx, uint32_t nan, bool fallback, int pick, int64_t row,
                                            const MseRatios &R, const PcMseArgs &a, bool writer) {
  float lo = mn, hi = mx;
  if (!fallback) mse_range(mn, mx, R.r[pick], &lo, &hi);
  float st[2] = {a.run_min[row], a.run_max[row]};
  double qp[VSIQ_QP_LEN], clip[2];
  hist_finish(lo, hi, nan != 0u, st, qp, clip, a.sym, a.qden, a.eps);
  if (writer) {
    a.run_min[row] = st[0];
    a.run_max[row] = st[1];
    a.scale_out[row] = qp[VSIQ_QP_SCALE];
    a.zp_out[row] = qp[VSIQ_QP_ZP];
    a.clip_out[2 * row] = clip[0];
    a.clip_out[2 * row + 1] = clip[1];
    a.pick_out[row] = pick;
  }
  QP p = make_qp((float)qp[VSIQ_QP_SCALE], (float)qp[VSIQ_QP_ZP], a.lo, a.hi, 0);
  // the fast path also needs the whole row finite and in range (QP::fast)
  p.fast = (p.fast && !nan && __builtin_fmaxf(__builtin_fabsf(mn), __builtin_fabsf(mx)) <= 0x1p62f) ? 1u : 0u;
  return p;
}

// group i of the row fake-quantized and stored (y, codes, the wave's mask chunk)
template <bool VEC, bool NT>
__device__ __forceinline__ void pc_mse_quant(f4 w, const QP &p, int64_t i, int64_t ng, int64_t rowlen,
                                             float *__restrict__ yr, uint8_t *__restrict__ cr,
                                             uint64_t *__restrict__ mr) {
  const int lane = threadIdx.x % kWave;
  if (i - lane >= ng) return;   // the whole wave past the row end (uniform)
  const bool in = i < ng;
  Elem e0, e1, e2, e3;
  fq_group_row(w, p, e0, e1, e2, e3);
  const int nv = in ? valid_in_group(i, rowlen) : 0;
  if (in) {
    f4 o;
    o.x = e0.y; o.y = e1.y; o.z = e2.y; o.w = e3.y;
    store_group<VEC, NT>(yr, i, rowlen, o);
    if (cr) {
      const uint32_t c = e0.code | (e1.code << 8) | (e2.code << 16) | (e3.code << 24);
      for (int j = 0; j < nv; ++j) cr[4 * i + j] = (uint8_t)(c >> (8 * j));
    }
  }
  if (mr) store_mask_chunk(mr + 4 * (i / kWave), e0.m && nv > 0, e1.m && nv > 1, e2.m && nv > 2, e3.m && nv > 3);
}

// ----------------------------------------------------------------------------
// wave per row: no LDS, no barrier
// ----------------------------------------------------------------------------
template <int U, int NC, bool VEC, bool NT>
__global__ __launch_bounds__(kBlock) void k_pc_mse_wave(const float *__restrict__ x, float *__restrict__ y,
                                                         uint8_t *__restrict__ codes, uint64_t *__restrict__ mask,
                                                         MseRatios R, PcMseArgs a) {
  const int lane = threadIdx.x % kWave;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int64_t row = (int64_t)blockIdx.x * kWaves + wave;
  if (row >= a.rows) return;   // a wave past the last row: nobody waits for it
  const float *xr = x + row * a.rowlen;
  const int64_t ng = cdiv(a.rowlen, 4);
  f4 v[NC][U];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < U; ++k) v[c][k] = load_group_c<VEC, NT>(xr, (c * U + k) * kWave + lane, ng, a.rowlen);
  const bool stats = a.row_stats != nullptr;
  PcRowAcc r = pc_rowacc();
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < U; ++k) pc_rowacc_add<VEC>(r, v[c][k], (c * U + k) * kWave + lane, ng, a.rowlen, stats);
  const float mn = wave_reduce(r.mn, MinOp()), mx = wave_reduce(r.mx, MaxOp());
  const uint32_t nan = wave_reduce(r.nan, OrU());
  if (stats) {
    const double sa = wave_reduce(r.rs.sa, AddD()), s1 = wave_reduce(r.rs.s1, AddD()),
                 s2 = wave_reduce(r.rs.s2, AddD());
    if (lane == 0) {
      a.row_stats[row * 3 + 0] = sa;
      a.row_stats[row * 3 + 1] = s1;
      a.row_stats[row * 3 + 2] = s2;
    }
  }

  const bool fallback = mse_fallback(mn, mx, nan != 0u, a.count);   // the row's own: wave-uniform
  double e[2] = {__builtin_inf(), __builtin_inf()};
  int pick = 0;
  if (!fallback) {
    float ps[2], pr[2], pz[2];
    uint32_t pf[2];
    pc_mse_cands(mn, mx, R, a, ps, pr, pz, pf);
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < NC; ++c)
      pc_mse_chunk<U>(v[c], (int64_t)c * U * kWave, ng, a.rowlen, a.count, ps, pr, pz, pf, a.lo, a.hi, acc);
    e[0] = (pf[0] & kMseValid) ? acc[0] : __builtin_inf();
    e[1] = (pf[1] & kMseValid) ? acc[1] : __builtin_inf();
    // mse_pick's scan over the wave's sums, read lane by lane (the same in every lane)
    double best = lane_f64(e[0], 0);
    for (int k = 1; k < a.count; ++k) {
      const double ek = k < kWave ? lane_f64(e[0], k) : lane_f64(e[1], k - kWave);
      if (ek < best) {
        best = ek;
        pick = k;
      }
    }
  }
  if (a.err_out) {
    if (lane < a.count) a.err_out[row * a.count + lane] = e[0];
    if (lane + kWave < a.count) a.err_out[row * a.count + lane + kWave] = e[1];
  }
  const QP p = pc_mse_finish(mn, mx, nan, fallback, pick, row, R, a, lane == 0);
  if (!y) return;
  float *yr = y + row * a.rowlen;
  uint8_t *cr = codes ? codes + row * a.rowlen : nullptr;
  uint64_t *mr = mask ? mask + row * mask_words_per_row(a.rowlen) : nullptr;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < U; ++k)
      pc_mse_quant<VEC, NT>(v[c][k], p, (c * U + k) * kWave + lane, ng, a.rowlen, yr, cr, mr);
}

// ----------------------------------------------------------------------------
// workgroup per row
// ----------------------------------------------------------------------------
struct PcMseRow {
  float mn, mx;
  uint32_t nan;
  bool fallback;
};

// The row's min / max / NaN flag from every lane's share, the same in every thread (one
// barrier); thread 0 writes the row's sums.
__device__ __forceinline__ PcMseRow pc_mse_row_reduce(PcRowAcc r, int64_t row, const PcMseArgs &a) {
  __shared__ float s_mn[kWaves], s_mx[kWaves];
  __shared__ uint32_t s_nan[kWaves];
  __shared__ double s_rs[3][kWaves];
  const bool stats = a.row_stats != nullptr;
  const float wmn = wave_reduce(r.mn, MinOp()), wmx = wave_reduce(r.mx, MaxOp());
  const uint32_t wnan = wave_reduce(r.nan, OrU());
  const int w = threadIdx.x / kWave;
  if (stats) {
    const double sa = wave_reduce(r.rs.sa, AddD()), s1 = wave_reduce(r.rs.s1, AddD()),
                 s2 = wave_reduce(r.rs.s2, AddD());
    if (threadIdx.x % kWave == 0) { s_rs[0][w] = sa; s_rs[1][w] = s1; s_rs[2][w] = s2; }
  }
  if (threadIdx.x % kWave == 0) { s_mn[w] = wmn; s_mx[w] = wmx; s_nan[w] = wnan; }
  __syncthreads();
  PcMseRow o{s_mn[0], s_mx[0], s_nan[0], false};
#pragma unroll
  for (int i = 1; i < kWaves; ++i) {
    o.mn = fminf(o.mn, s_mn[i]); o.mx = fmaxf(o.mx, s_mx[i]); o.nan |= s_nan[i];
  }
  if (stats && threadIdx.x == 0) {
    double sa = s_rs[0][0], s1 = s_rs[1][0], s2 = s_rs[2][0];
    for (int i = 1; i < kWaves; ++i) { sa += s_rs[0][i]; s1 += s_rs[1][i]; s2 += s_rs[2][i]; }
    a.row_stats[row * 3 + 0] = sa;
    a.row_stats[row * 3 + 1] = s1;
    a.row_stats[row * 3 + 2] = s2;
  }
  o.fallback = mse_fallback(o.mn, o.mx, o.nan != 0u, a.count);   // the same in every thread
  return o;
}

// The waves' sums added in wave order (candidate k in thread k), the errors out, the pick
// and the row's end.  Two barriers, reached by every thread whether the row searched or not.
__device__ __forceinline__ QP pc_mse_block_end(const PcMseRow &m, const double (&acc)[2], const uint32_t (&pf)[2],
                                               int64_t row, const MseRatios &R, const PcMseArgs &a) {
  __shared__ double s_w[kWaves][kMseMaxCand];
  __shared__ double s_e[kMseMaxCand];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  s_w[wave][lane] = acc[0];
  s_w[wave][lane + kWave] = acc[1];
  __syncthreads();
  const int k = threadIdx.x;
  if (k < a.count) {
    const bool valid = !m.fallback && ((k < kWave ? pf[0] : pf[1]) & kMseValid) != 0u;   // candidate k: this lane's own
    double e = 0.0;
    for (int w = 0; w < kWaves; ++w) e += s_w[w][k];
    if (!valid) e = __builtin_inf();
    s_e[k] = e;
    if (a.err_out) a.err_out[row * a.count + k] = e;
  }
  __syncthreads();
  const int pick = m.fallback ? 0 : mse_pick(s_e, a.count);
  return pc_mse_finish(m.mn, m.mx, m.nan, m.fallback, pick, row, R, a, threadIdx.x == 0);
}

// The row in registers: wave w holds the contiguous groups [w * G, (w + 1) * G), G = 64 * U * NC.
template <int NC, bool VEC, bool NT>
__global__ __launch_bounds__(kBlock) void k_pc_mse_block(const float *__restrict__ x, float *__restrict__ y,
                                                          uint8_t *__restrict__ codes, uint64_t *__restrict__ mask,
                                                          MseRatios R, PcMseArgs a) {
  constexpr int U = kPcMseU;
  const int lane = threadIdx.x % kWave;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int64_t row = blockIdx.x;
  const float *xr = x + row * a.rowlen;
  const int64_t ng = cdiv(a.rowlen, 4);
  const int64_t w0 = (int64_t)wave * (kWave * U * NC);   // the wave's first group
  f4 v[NC][U];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < U; ++k) v[c][k] = load_group_c<VEC, NT>(xr, w0 + (c * U + k) * kWave + lane, ng, a.rowlen);
  const bool stats = a.row_stats != nullptr;
  PcRowAcc r = pc_rowacc();
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < U; ++k)
      pc_rowacc_add<VEC>(r, v[c][k], w0 + (c * U + k) * kWave + lane, ng, a.rowlen, stats);
  const PcMseRow m = pc_mse_row_reduce(r, row, a);

  float ps[2] = {0.f, 0.f}, pr[2] = {0.f, 0.f}, pz[2] = {0.f, 0.f};
  uint32_t pf[2] = {0u, 0u};
  double acc[2] = {0.0, 0.0};
  if (!m.fallback) {   // uniform over the workgroup; no barrier inside
    pc_mse_cands(m.mn, m.mx, R, a, ps, pr, pz, pf);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      pc_mse_chunk<U>(v[c], w0 + (int64_t)c * U * kWave, ng, a.rowlen, a.count, ps, pr, pz, pf, a.lo, a.hi, acc);
  }
  const QP p = pc_mse_block_end(m, acc, pf, row, R, a);
  if (!y) return;
  float *yr = y + row * a.rowlen;
  uint8_t *cr = codes ? codes + row * a.rowlen : nullptr;
  uint64_t *mr = mask ? mask + row * mask_words_per_row(a.rowlen) : nullptr;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < U; ++k)
      pc_mse_quant<VEC, NT>(v[c][k], p, w0 + (c * U + k) * kWave + lane, ng, a.rowlen, yr, cr, mr);
}

// Rows too long for registers: min / max, then the search in tiles of kBlock * U groups
// (wave w the tile's groups [w * 64 * U, (w + 1) * 64 * U)), then the fake quant; the second
// and third pass read the row from L2.
template <bool VEC, bool NT>
__global__ __launch_bounds__(kBlock) void k_pc_mse_long(const float *__restrict__ x, float *__restrict__ y,
                                                         uint8_t *__restrict__ codes, uint64_t *__restrict__ mask,
                                                         MseRatios R, PcMseArgs a) {
  constexpr int U = kPcMseU;
  const int lane = threadIdx.x % kWave;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int64_t row = blockIdx.x;
  const float *xr = x + row * a.rowlen;
  const int64_t ng = cdiv(a.rowlen, 4);
  const bool stats = a.row_stats != nullptr;
  PcRowAcc r = pc_rowacc();
  for (int64_t i = threadIdx.x; i < ng; i += kBlock)
    pc_rowacc_add<VEC>(r, load_group<VEC, false>(xr, i, a.rowlen), i, ng, a.rowlen, stats);
  const PcMseRow m = pc_mse_row_reduce(r, row, a);

  float ps[2] = {0.f, 0.f}, pr[2] = {0.f, 0.f}, pz[2] = {0.f, 0.f};
  uint32_t pf[2] = {0u, 0u};
  double acc[2] = {0.0, 0.0};
  if (!m.fallback) {   // uniform over the workgroup; no barrier inside
    pc_mse_cands(m.mn, m.mx, R, a, ps, pr, pz, pf);
    for (int64_t base = 0; base < ng; base += (int64_t)kBlock * U) {
      const int64_t i0 = base + (int64_t)wave * (kWave * U);
      f4 v[U];
#pragma unroll
      for (int k = 0; k < U; ++k) v[k] = load_group_c<VEC, false>(xr, i0 + k * kWave + lane, ng, a.rowlen);
      pc_mse_chunk<U>(v, i0, ng, a.rowlen, a.count, ps, pr, pz, pf, a.lo, a.hi, acc);
    }
  }
  const QP p = pc_mse_block_end(m, acc, pf, row, R, a);
  if (!y) return;
  float *yr = y + row * a.rowlen;
  uint8_t *cr = codes ? codes + row * a.rowlen : nullptr;
  uint64_t *mr = mask ? mask + row * mask_words_per_row(a.rowlen) : nullptr;
  for (int64_t base = 0; base < ng; base += kBlock) {
    const int64_t i = base + threadIdx.x;
    pc_mse_quant<VEC, NT>(load_group_c<VEC, NT>(xr, i, ng, a.rowlen), p, i, ng, a.rowlen, yr, cr, mr);
  }
}

template <bool VEC, bool NT>
void launch_pc_mse(const float *x, float *y, uint8_t *c, uint64_t *m, const MseRatios &R, const PcMseArgs &a,
                   hipStream_t st) {
  const dim3 block(kBlock);
  if (a.rowlen <= kPcMseWaveMax) {
    const dim3 grid((unsigned)cdiv(a.rows, kWaves));
    if (a.rowlen <= kPcMseWaveShort)
      hipLaunchKernelGGL((k_pc_mse_wave<1, 1, VEC, NT>), grid, block, 0, st, x, y, c, m, R, a);
    else
      with_int_le<1, kPcMseWaveChunks>(cdiv(a.rowlen, 4 * kWave * kPcMseU), [&](auto NC) {
        hipLaunchKernelGGL((k_pc_mse_wave<kPcMseU, decltype(NC)::value, VEC, NT>), grid, block, 0, st, x, y, c, m,
                           R, a);
      });
    return;
  }
  const dim3 grid((unsigned)a.rows);
  if (a.rowlen <= kPcMseBlockMax)
    with_int_le<1, 2, 3, kPcMseBlockChunks>(cdiv(a.rowlen, 4 * kBlock * kPcMseU), [&](auto NC) {
      hipLaunchKernelGGL((k_pc_mse_block<decltype(NC)::value, VEC, NT>), grid, block, 0, st, x, y, c, m, R, a);
    });
  else
    hipLaunchKernelGGL((k_pc_mse_long<VEC, NT>), grid, block, 0, st, x, y, c, m, R, a);
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_pc_observe_mse_f32(const float *x, float *y, void *codes, uint64_t *mask, int64_t rows, int64_t rowlen,
                            const double *ratios, int count, float *run_min, float *run_max, double *scale_out,
                            double *zp_out, double *clip_out, double *err_out, int32_t *pick_out, double *row_stats,
                            int symmetric, int qmin, int qmax, double qden, double eps, void *stream) {
  if (rows <= 0 || rowlen <= 0 || rows > 0x7fffffffLL) return VSIQ_E_ARG;
  if (!x || !run_min || !run_max || !scale_out || !zp_out || !clip_out || !pick_out) return VSIQ_E_ARG;
  if (!y && (codes || mask)) return VSIQ_E_ARG;
  if (!mse_ratios_ok(ratios, count) || qmin >= qmax) return VSIQ_E_ARG;
  if (mask && !aligned8(mask)) return VSIQ_E_ALIGN;
  MseRatios R{};
  for (int k = 0; k < count; ++k) R.r[k] = ratios[k];
  const PcMseArgs a{rows,     rowlen,   count,     run_min,   run_max,      scale_out,    zp_out, clip_out,
                    err_out,  pick_out, row_stats, symmetric, (float)qmin, (float)qmax, qden,   eps};
  const bool vec = (rowlen % 4 == 0) && aligned16(x) && (!y || aligned16(y));
  const bool nt = g_tune.nontemporal != 0;
  with_vec_nt(vec, nt, [&](auto V, auto N) {
    launch_pc_mse<decltype(V)::value, decltype(N)::value>(x, y, (uint8_t *)codes, mask, R, a, (hipStream_t)stream);
  });
  return launch_rc();
}

}  // extern "C"
