// k_adaround.hip — AdaRound's two launches per optimisation step (arithmetic: k_adaround.cuh,
// statement: include/vsiq.h):
//   k_adaround_fwd   reads w and V once, writes y (soft or hard) and, when asked, folds the
//                    f64 regulariser R = sum(1 - |2h - 1|^beta) (per-workgroup records + one
//                    fold by the last workgroup to arrive: fold_arrivals, no host sync)
//   k_adaround_bwd   reads g, w and V, writes grad_V
// Grid (rows, chunks) as the per-channel forward (k_pc.hip): a workgroup takes kFlatU groups
// per lane of ONE row, so the row's qparams are wave-uniform and read with scalar loads
// after the streaming loads are issued.  A per-tensor call is one row of n elements.  Rows
// of any length: rowlen % 4 != 0 (or unaligned tensors) takes the per-element path of
// load_group / store_group.  No LDS beyond the fold's, no scratch.
#include "dispatch.cuh"
#include "k_adaround.cuh"

namespace vsiq {

struct AdaArgs {
  int64_t rowlen;
  const double *scale, *zp;   // f64 [1] or [rows]; zp nullable: 0
  int zp_round, perrow;
  float lo, hi;
};

// `row` is wave-uniform: scalar loads (ld_uniform_f64)
__device__ __forceinline__ QP ada_qp(const AdaArgs &a, int64_t row) {
  const int64_t c = a.perrow ? row : 0;
  const QPSrc s{nullptr, a.scale + c, a.zp ? a.zp + c : nullptr, 0.0, 0.0, a.lo, a.hi, a.zp_round, 0};
  return load_qp<true>(s);
}

// the forward kernels' quotient and add: RN(RN(w / s) + z), IEEE division where the
// Markstein path does not apply
__device__ __forceinline__ float ada_t(float w, const QP &p) { return fdiv(w, p.d) + p.z; }

struct AdaFold {   // partial record {sum of regulariser terms}
  static constexpr int K = 1;
  __device__ static void init(double (&a)[1]) { a[0] = 0.0; }
  __device__ static void add(double (&a)[1], const double (&r)[1]) { a[0] += r[0]; }
  __device__ static void wave(double (&a)[1]) { a[0] = wave_reduce(a[0], AddD()); }
};

template <bool VEC, bool NT, int MODE>
__global__ __launch_bounds__(kBlock) void k_adaround_fwd(const float *__restrict__ w, const float *__restrict__ v,
                                                         float *__restrict__ y, uint32_t chunks, AdaArgs a,
                                                         double beta, double *__restrict__ reg_out,
                                                         double *__restrict__ ws, uint32_t *__restrict__ counter) {
  constexpr int U = kFlatU;
  constexpr bool WY = MODE != kAdaRegOnly, REG = MODE == kAdaSoftReg || MODE == kAdaRegOnly;
  const int64_t row = blockIdx.x / chunks;
  const int64_t chunk = blockIdx.x % chunks;
  const int64_t ng = cdiv(a.rowlen, 4);
  const int64_t base = chunk * kBlock * U + threadIdx.x;
  const float *vr = v + row * a.rowlen;
  f4 vv[U], vw[U];
#pragma unroll
  for (int u = 0; u < U; ++u) vv[u] = load_group_c<VEC, NT>(vr, base + u * kBlock, ng, a.rowlen);
  QP p{};
  if constexpr (WY) {
    const float *wr = w + row * a.rowlen;
#pragma unroll
    for (int u = 0; u < U; ++u) vw[u] = load_group_c<VEC, NT>(wr, base + u * kBlock, ng, a.rowlen);
    p = ada_qp(a, row);   // after the streaming loads are issued, on lgkmcnt
  }
  double acc = 0.0;
  f4 o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + u * kBlock;
    const int nv = i < ng ? valid_in_group(i, a.rowlen) : 0;
    const float ev[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
    float h[4], yo[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = MODE == kAdaHard ? ada_hard(ev[j]) : ada_soft(ev[j]).h;
    if constexpr (REG) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) acc += ada_reg(h[j], beta);
    }
    if constexpr (WY) {
      const float ew[4] = {vw[u].x, vw[u].y, vw[u].z, vw[u].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) yo[j] = ada_out(ada_t(ew[j], p), h[j], p.s, p.z, p.lo, p.hi).y;
    }
    o[u].x = yo[0]; o[u].y = yo[1]; o[u].z = yo[2]; o[u].w = yo[3];
  }
  if constexpr (WY) {
    float *yr = y + row * a.rowlen;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * kBlock;
      if (i < ng) store_group<VEC, NT>(yr, i, a.rowlen, o[u]);
    }
  }
  if constexpr (REG) {
    __shared__ double s_w[kWaves][1];
    double r[1] = {acc}, f[1];
    fold_waves<AdaFold>(r, s_w);   // thread 0: the workgroup's sum
    if (gridDim.x == 1) {          // one workgroup: no record, no arrival
      if (threadIdx.x == 0) *reg_out = r[0];
      return;
    }
    if (threadIdx.x == 0) partial_store(ws + (int64_t)blockIdx.x * kPartials, r[0]);
    if (!fold_arrivals<AdaFold>(ws, counter, f)) return;
    if (threadIdx.x == 0) {
      *reg_out = f[0];
      *counter = 0u;   // ready for the next stream-ordered launch
    }
  }
}

template <bool VEC, bool NT>
__global__ __launch_bounds__(kBlock) void k_adaround_bwd(const float *__restrict__ g, const float *__restrict__ w,
                                                         const float *__restrict__ v, float *__restrict__ gv,
                                                         uint32_t chunks, AdaArgs a, double lam, double beta) {
  constexpr int U = kFlatU;
  const int64_t row = blockIdx.x / chunks;
  const int64_t chunk = blockIdx.x % chunks;
  const int64_t ng = cdiv(a.rowlen, 4);
  const int64_t base = chunk * kBlock * U + threadIdx.x;
  const int64_t off = row * a.rowlen;
  f4 vg[U], vw[U], vv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    vg[u] = load_group_c<VEC, NT>(g + off, base + u * kBlock, ng, a.rowlen);
    vw[u] = load_group_c<VEC, NT>(w + off, base + u * kBlock, ng, a.rowlen);
    vv[u] = load_group_c<VEC, NT>(v + off, base + u * kBlock, ng, a.rowlen);
  }
  const QP p = ada_qp(a, row);   // after the streaming loads are issued, on lgkmcnt
  f4 o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float eg[4] = {vg[u].x, vg[u].y, vg[u].z, vg[u].w};
    const float ew[4] = {vw[u].x, vw[u].y, vw[u].z, vw[u].w};
    const float ev[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = ada_grad(eg[j], ada_t(ew[j], p), ev[j], p.s, p.z, p.lo, p.hi, lam, beta);
    o[u].x = r[0]; o[u].y = r[1]; o[u].z = r[2]; o[u].w = r[3];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t i = base + u * kBlock;
    if (i < ng) store_group<VEC, NT>(gv + off, i, a.rowlen, o[u]);
  }
}

// the (rows, chunks) grid of both kernels; 0 when it does not fit a 31-bit block index
inline int64_t ada_grid(int64_t rows, int64_t rowlen, int64_t *chunks) {
  *chunks = oneshot_grid(cdiv(rowlen, 4));
  if (rows > 0 && *chunks > 0x7fffffffLL / rows) return 0;
  return rows * *chunks;
}

// shared argument checks (before any pointer is looked at)
inline int ada_check(int64_t rows, int64_t rowlen, int64_t nq, int qmin, int qmax) {
  if (rows < 0 || rowlen <= 0 || qmin > qmax) return VSIQ_E_ARG;
  if (rows > 0 && nq != 1 && nq != rows) return VSIQ_E_ARG;
  return 0;
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int64_t vsiq_adaround_workspace_doubles(int64_t rows, int64_t rowlen) {
  int64_t chunks;
  if (rows < 0 || rowlen <= 0) return VSIQ_E_ARG;
  const int64_t grid = ada_grid(rows, rowlen, &chunks);
  if (rows > 0 && grid == 0) return VSIQ_E_ARG;
  return fold_records(std::max<int64_t>(grid, 1)) * kPartials;
}

int vsiq_adaround_fwd_f32(const float *w, const float *v, float *y, int64_t rows, int64_t rowlen,
                          const double *scale, const double *zp, int64_t nq, int zp_round, int qmin, int qmax,
                          int hard, double beta, double *reg_out, double *ws, int64_t ws_len, uint32_t *counter,
                          void *stream) {
  if (const int e = ada_check(rows, rowlen, nq, qmin, qmax)) return e;
  if (rows == 0) return 0;
  if (!v || (!y && !reg_out) || (y && (!w || !scale))) return VSIQ_E_ARG;
  if (reg_out && (hard || !(beta > 0.0) || !ws || !counter)) return VSIQ_E_ARG;
  int64_t chunks;
  const int64_t grid = ada_grid(rows, rowlen, &chunks);
  if (grid == 0) return VSIQ_E_ARG;
  if (reg_out && ws_len < fold_records(grid) * kPartials) return VSIQ_E_WS;
  const AdaArgs a{rowlen, scale, zp, zp_round, nq != 1, (float)qmin, (float)qmax};
  const bool vec = rowlen % 4 == 0 && aligned16(v) && (!y || (aligned16(w) && aligned16(y)));
  const bool nt = g_tune.nontemporal != 0;
  const int mode = !y ? kAdaRegOnly : hard ? kAdaHard : reg_out ? kAdaSoftReg : kAdaSoft;
  const dim3 gd((unsigned)grid), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  with_int<kAdaSoft, kAdaSoftReg, kAdaHard, kAdaRegOnly>(mode, [&](auto M) {
    with_vec_nt(vec, nt, [&](auto V, auto N) {
      hipLaunchKernelGGL((k_adaround_fwd<decltype(V)::value, decltype(N)::value, decltype(M)::value>), gd, block, 0,
                         st, w, v, y, (uint32_t)chunks, a, beta, reg_out, ws, counter);
    });
  });
  return launch_rc();
}

int vsiq_adaround_bwd_f32(const float *g, const float *w, const float *v, float *grad_v, int64_t rows,
                          int64_t rowlen, const double *scale, const double *zp, int64_t nq, int zp_round, int qmin,
                          int qmax, double lam, double beta, void *stream) {
  if (const int e = ada_check(rows, rowlen, nq, qmin, qmax)) return e;
  if (rows == 0) return 0;
  if (!g || !w || !v || !grad_v || !scale || !(beta > 0.0) || lam != lam) return VSIQ_E_ARG;
  int64_t chunks;
  const int64_t grid = ada_grid(rows, rowlen, &chunks);
  if (grid == 0) return VSIQ_E_ARG;
  const AdaArgs a{rowlen, scale, zp, zp_round, nq != 1, (float)qmin, (float)qmax};
  const bool vec = rowlen % 4 == 0 && aligned16(g) && aligned16(w) && aligned16(v) && aligned16(grad_v);
  const bool nt = g_tune.nontemporal != 0;
  const dim3 gd((unsigned)grid), block(kBlock);
  hipStream_t st = (hipStream_t)stream;
  with_vec_nt(vec, nt, [&](auto V, auto N) {
    hipLaunchKernelGGL((k_adaround_bwd<decltype(V)::value, decltype(N)::value>), gd, block, 0, st, g, w, v, grad_v,
                       (uint32_t)chunks, a, lam, beta);
  });
  return launch_rc();
}

}  // extern "C"
