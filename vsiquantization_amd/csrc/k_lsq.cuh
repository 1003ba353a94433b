// k_lsq.cuh — K4 learnable (LSQ) backward of one tensor: the kernel, its launcher and the
// argument checks, over the element type T of g / x / gx.  k_lsq.hip instantiates fp32
// (and holds the records-only, per-channel and C ABI parts); k_lsq_half.hip instantiates
// bf16 / fp16.
#pragma once
#include "dispatch.cuh"
#include "k_body.cuh"

namespace vsiq {

// PART: the block record {sum t, sum z} goes to ws[2 * block] with a plain store and
// the block leaves -- no drain, no arrival, no fold (vsiq_act_lsq_bwd_part_f32: the
// fold of every layer's records runs later in one launch, k_lsq_fold_multi).  `gate`:
// the one-round PART grids' store gate (round 5, launch_lsq_g; 0 = none).
template <bool VEC, bool NT, bool ZPL, int ACT, int G, bool PART, typename T>
__device__ __forceinline__ void lsq_bwd_body(const T *__restrict__ g, const T *__restrict__ x,
                                             T *__restrict__ gx, int64_t n, const QPSrc &src, double gscale,
                                             const SiluLay &L, double *__restrict__ grad_out,
                                             double *__restrict__ ws, uint32_t *__restrict__ counter,
                                             uint32_t gate) {
  const GateClk gc = gate_begin(gate);
  LsqAcc c{0.0, 0.0};
  f4 o[G];
  // G <= 2 (C4's small one-round layers): the kernel-uniform qparams as scalar loads after
  // the first x / g loads are issued (round 6).  Deeper grids keep them first: the late
  // loads cost 2 VGPRs there, one wave per SIMD at G = 4 / 8 (C3's K4: 98 VGPRs, 4 waves),
  // and measured equal at C3 (profiles/r06/r06x_k4_late_qparams.txt).
  QP p;
  if constexpr (G <= 2) {
    p = lsq_bwd_block<VEC, NT, ZPL, ACT, G>(g, x, n, [&] { return load_qp<true>(src); }, blockIdx.x, c, o, L);
  } else {
    p = load_qp(src);
    (void)lsq_bwd_block<VEC, NT, ZPL, ACT, G>(g, x, n, p, blockIdx.x, c, o, L);
  }
  if (PART) {
    // no arrival to order against: every wave issues its grad_x stores first, so the
    // block reduction runs while they drain (the one-round grids of small layers end
    // with it otherwise on the critical path)
    gate_pass(gate, gc);
    lsq_store_block<VEC, NT, G>(gx, n, blockIdx.x, o);
    double rec[2];
    if (!lsq_block_record<VEC, NT, G, false>(c, gx, n, blockIdx.x, o, rec)) return;
    if (threadIdx.x == 0) {
      // a NaN sum leaves as the canonical quiet NaN: which operand's payload an add of two
      // NaNs keeps depends on the operand order the compiler picked for this instance, and
      // the records of a 16-bit call are the fp32 call's bits for NaN sums too
      ws[2 * (int64_t)blockIdx.x] = rec[0] != rec[0] ? __builtin_nan("") : rec[0];
      ws[2 * (int64_t)blockIdx.x + 1] = rec[1] != rec[1] ? __builtin_nan("") : rec[1];
    }
    return;
  }
  double rec[2], f[2];
  if (!lsq_block_record<VEC, NT, G>(c, gx, n, blockIdx.x, o, rec)) return;   // waves 1..3 done
  const bool last = wave_arrive<LsqFold>(ws, 0, gridDim.x, blockIdx.x, counter, rec, f, [&]() {
    lsq_store_block<VEC, NT, G>(gx, n, blockIdx.x, o);   // wave 0's grad_x, after its arrival
  });
  if (!last) return;
  if (threadIdx.x == 0) {
    grad_out[0] = f[0] * gscale;
    grad_out[1] = ZPL ? lsq_grad_zp(f[1], src, p, gscale) : 0.0;
    *counter = 0u;
  }
}

// The fp32 kernel keeps its name and signature (saved gate tables and kernel traces name
// it); k_lsq_bwd_t is the same body on 16-bit tensors and k_lsq_bwd_part_t its records-only
// (PART) form -- a kernel of its own, so k_lsq_bwd_t's symbols stay what they were.
template <bool VEC, bool NT, bool ZPL, int ACT, int G, bool PART = false>
__global__ __launch_bounds__(kBlock) void k_lsq_bwd(const float *__restrict__ g,
                                                    const float *__restrict__ x,
                                                    float *__restrict__ gx, int64_t n,
                                                    QPSrc src, double gscale, SiluLay L,
                                                    double *__restrict__ grad_out,
                                                    double *__restrict__ ws,
                                                    uint32_t *__restrict__ counter, uint32_t gate) {
  lsq_bwd_body<VEC, NT, ZPL, ACT, G, PART>(g, x, gx, n, src, gscale, L, grad_out, ws, counter, gate);
}

template <typename T, bool VEC, bool NT, bool ZPL, int ACT, int G>
__global__ __launch_bounds__(kBlock) void k_lsq_bwd_t(const T *__restrict__ g, const T *__restrict__ x,
                                                      T *__restrict__ gx, int64_t n, QPSrc src,
                                                      double gscale, SiluLay L,
                                                      double *__restrict__ grad_out,
                                                      double *__restrict__ ws,
                                                      uint32_t *__restrict__ counter, uint32_t gate) {
  lsq_bwd_body<VEC, NT, ZPL, ACT, G, false>(g, x, gx, n, src, gscale, L, grad_out, ws, counter, gate);
}

template <typename T, bool VEC, bool NT, bool ZPL, int ACT, int G>
__global__ __launch_bounds__(kBlock) void k_lsq_bwd_part_t(const T *__restrict__ g, const T *__restrict__ x,
                                                           T *__restrict__ gx, int64_t n, QPSrc src,
                                                           double gscale, SiluLay L,
                                                           double *__restrict__ grad_out,
                                                           double *__restrict__ ws,
                                                           uint32_t *__restrict__ counter, uint32_t gate) {
  lsq_bwd_body<VEC, NT, ZPL, ACT, G, true>(g, x, gx, n, src, gscale, L, grad_out, ws, counter, gate);
}

template <typename T, bool VEC, bool NT, bool ZPL, int ACT, int G>
constexpr auto lsq_bwd_kernel() {
  if constexpr (std::is_same_v<T, float>) return &k_lsq_bwd<VEC, NT, ZPL, ACT, G>;
  else return &k_lsq_bwd_t<T, VEC, NT, ZPL, ACT, G>;
}

template <typename T, bool VEC, bool NT, bool ZPL, int ACT, int G>
constexpr auto lsq_bwd_part_kernel() {
  if constexpr (std::is_same_v<T, float>) return &k_lsq_bwd<VEC, NT, ZPL, ACT, G, true>;
  else return &k_lsq_bwd_part_t<T, VEC, NT, ZPL, ACT, G>;
}

template <int ACT, bool VEC, bool NT, int G, typename T>
void launch_lsq_g(const T *g, const T *x, T *gx, int64_t n, const QPSrc &src, int zpl,
                  double gscale, double *grad_out, double *ws, uint32_t *counter, int64_t grid,
                  const SiluLay &L, hipStream_t st) {
  if (!counter) {   // records only (PART)
    // a one-round grid (store_gate_select takes grids of 2..occ workgroups per CU only):
    // the tuned store gate between the read and the write phase.  One site label for
    // every T; the read bytes (x and g) and the occupancy are the instance's own.
    const auto kt = lsq_bwd_part_kernel<T, VEC, NT, true, ACT, G>();
    const auto kf = lsq_bwd_part_kernel<T, VEC, NT, false, ACT, G>();
    static const int occ_t = occupancy_blocks(reinterpret_cast<const void *>(kt), kBlock);
    static const int occ_f = occupancy_blocks(reinterpret_cast<const void *>(kf), kBlock);
    const void *kern = zpl ? reinterpret_cast<const void *>(kt) : reinterpret_cast<const void *>(kf);
    GateSel gs = store_gate_select("k4d_lsq_bwd_part", kern, grid, zpl ? occ_t : occ_f,
                                   2 * (int64_t)sizeof(T) * n, st);
    if (zpl)
      hipLaunchKernelGGL(kt, dim3((unsigned)grid), dim3(kBlock), 0, st, g, x, gx, n, src, gscale, L, grad_out, ws,
                         counter, gs.gate);
    else
      hipLaunchKernelGGL(kf, dim3((unsigned)grid), dim3(kBlock), 0, st, g, x, gx, n, src, gscale, L, grad_out, ws,
                         counter, gs.gate);
    store_gate_launched(gs, st);
    return;
  }
  if (zpl)
    hipLaunchKernelGGL((lsq_bwd_kernel<T, VEC, NT, true, ACT, G>()), dim3((unsigned)grid), dim3(kBlock), 0, st, g,
                       x, gx, n, src, gscale, L, grad_out, ws, counter, 0u);
  else
    hipLaunchKernelGGL((lsq_bwd_kernel<T, VEC, NT, false, ACT, G>()), dim3((unsigned)grid), dim3(kBlock), 0, st, g,
                       x, gx, n, src, gscale, L, grad_out, ws, counter, 0u);
}

// Records-only K4 (K4d): groups per lane 2.  Without an arrival chain more, smaller
// workgroups cost nothing and stream better at every C4 size (MI355X kernel trace, 3.3M
// -> 105M elements: 9.9 / 16.2 / 28.0 / 51.7 / 101.0 / 205.3 us at 2 per lane against
// 11.1 / 16.6 / 28.4 / 54.2 / 103.2 / 207.9 us at K4's 4 / 8, profiles/r03g_c4_groups.txt);
// the 4x larger record count is folded by the two-stage k_lsq_fold_chunks.
// (1 group per lane for the small layers measured slower still: 10.4 against 9.8 us at
// 3.3M elements, 214 against 201 us at 105M, profiles/r04h_c4_k4d.txt.)
// Round 5 (per-dispatch kernel trace of the C4 leg at 2 / 4 / 8 / 16 groups per lane,
// every one-round grid gated -- launch_lsq_g --, profiles/r05/r05p_k4d_groups.txt): 2 per
// lane is best or level up to 26M elements (3.3M 8.7 us gated against 9.6-10.6 for 4-16;
// 6.6M / 13M / 26M within 1 % of 4 per lane; the one-round 8 / 16 grids of 13M / 26M are
// slower even gated), 4 per lane from ~50M (52M 98.5 against 100.0 us, 105M 195.9
// against 204.8).
inline int lsq_part_groups_per_lane(int64_t n) {
  const int g = g_tune.lsq_groups;
  return g > 0 ? g : (n >= ((int64_t)48 << 20) ? 4 : 2);
}

// all four (VEC, NT) pairs: the scalar path streams its loads and stores non-temporally too
template <typename T>
void launch_lsq(int act, bool vec, bool nt, const T *g, const T *x, T *gx, int64_t n, const QPSrc &src,
                int zpl, double gscale, double *grad_out, double *ws, uint32_t *counter, int64_t grid, hipStream_t st) {
  const SiluLay L = act_lay(act, n);
  const int per_lane = counter ? lsq_groups_per_lane(cdiv(n, 4)) : lsq_part_groups_per_lane(n);
  with_act(act, [&](auto A) {
    with_vec_nt4(vec, nt, [&](auto V, auto N) {
      with_int<kLsqGroups, 8, 4, 2>(per_lane, [&](auto G) {
        launch_lsq_g<decltype(A)::value, decltype(V)::value, decltype(N)::value, decltype(G)::value>(
            g, x, gx, n, src, zpl, gscale, grad_out, ws, counter, grid, L, st);
      });
    });
  });
}

template <typename T>
int lsq_bwd(const T *g, const T *x, T *gx, int64_t n, int act, const double *scale_dev,
            double scale_host, const double *zp_dev, double zp_host, int zp_learn, int qmin, int qmax,
            double gscale, double *grad_out, double *ws, int64_t ws_len, uint32_t *counter,
            void *stream) {
  if (n <= 0 || !g || !x || !gx || !grad_out || !ws || !counter || qmin > qmax || !act_ok(act))
    return VSIQ_E_ARG;
  const bool vec = (n % 4 == 0) && aligned_vec<T>(g) && aligned_vec<T>(x) && aligned_vec<T>(gx);
  const int64_t grid = lsq_grid(cdiv(n, 4));
  if (grid > 0x7fffffffLL) return VSIQ_E_ARG;
  if (ws_len < fold_records(grid) * kPartials) return VSIQ_E_WS;
  // learnable zp (1): the forward used clamp(rint(zp)); 0 / 2: zp as given (2: with its gradient)
  if (zp_learn < 0 || zp_learn > 2) return VSIQ_E_ARG;
  QPSrc src{nullptr, scale_dev, zp_dev, scale_host, zp_host, (float)qmin, (float)qmax, zp_learn == 1, 0};
  const bool nt = g_tune.nontemporal != 0;
  launch_lsq(act, vec, nt, g, x, gx, n, src, zp_learn != 0, gscale, grad_out, ws, counter, grid, (hipStream_t)stream);
  return launch_rc();
}

// Records-only K4 (PART, K4d): lsq_bwd's per-element code and block records on a grid of
// lsq_part_groups_per_lane(n) groups per lane -- a function of n only, so a 16-bit call
// writes the records of the fp32 call on the widened tensors.
template <typename T>
int lsq_bwd_part(const T *g, const T *x, T *gx, int64_t n, int act, const double *scale_dev,
                 double scale_host, const double *zp_dev, double zp_host, int zp_learn, int qmin, int qmax,
                 double *records, int64_t records_len, void *stream) {
  if (n <= 0 || !g || !x || !gx || !records || qmin > qmax || !act_ok(act))
    return VSIQ_E_ARG;
  const bool vec = (n % 4 == 0) && aligned_vec<T>(g) && aligned_vec<T>(x) && aligned_vec<T>(gx);
  const int64_t grid = lsq_grid(cdiv(n, 4), lsq_part_groups_per_lane(n));
  if (grid > 0x7fffffffLL) return VSIQ_E_ARG;
  if (records_len < 2 * grid) return VSIQ_E_WS;
  if (zp_learn < 0 || zp_learn > 1) return VSIQ_E_ARG;   // the deferred fold knows modes 0 / 1 only
  QPSrc src{nullptr, scale_dev, zp_dev, scale_host, zp_host, (float)qmin, (float)qmax, zp_learn, 0};
  const bool nt = g_tune.nontemporal != 0;
  launch_lsq(act, vec, nt, g, x, gx, n, src, zp_learn, 0.0, nullptr, records, nullptr, grid, (hipStream_t)stream);
  return launch_rc();
}

#define VSIQ_LSQ_BWD_INST(T)                                                                                  \
  template int lsq_bwd<T>(const T *, const T *, T *, int64_t, int, const double *, double, const double *, \
                          double, int, int, int, double, double *, double *, int64_t, uint32_t *, void *)
#define VSIQ_LSQ_BWD_PART_INST(T)                                                                              \
  template int lsq_bwd_part<T>(const T *, const T *, T *, int64_t, int, const double *, double, const double *, \
                               double, int, int, int, double *, int64_t, void *)
extern VSIQ_LSQ_BWD_INST(bf16_t);
extern VSIQ_LSQ_BWD_INST(f16_t);
extern VSIQ_LSQ_BWD_PART_INST(bf16_t);
extern VSIQ_LSQ_BWD_PART_INST(f16_t);

}  // namespace vsiq
