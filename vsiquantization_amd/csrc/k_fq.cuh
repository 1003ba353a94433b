// k_fq.cuh — K1 per-tensor fake-quant forward (optionally behind a fused ReLU/SiLU, K5):
// the kernel, its launcher and the argument checks, over the element type T.  k_fq.hip
// instantiates fp32 and holds the C ABI; k_fq_half.hip instantiates bf16 / fp16.
#pragma once
#include "dispatch.cuh"
#include "k_body.cuh"

namespace vsiq {

// K1 kernel: one tensor, block body in k_body.cuh.  The fp32 kernel keeps its name and
// signature (saved gate tables and kernel traces name it); k_fq_fwd_t is the same body on
// a 16-bit tensor.
template <bool VEC, bool NT, bool CODES, bool MASK, int ACT, int U>
__global__ __launch_bounds__(kBlock) void k_fq_fwd(const float *__restrict__ x, float *__restrict__ y,
                                                   uint8_t *__restrict__ codes,
                                                   uint64_t *__restrict__ mask, int64_t n,
                                                   QPSrc src, uint32_t gate, SiluLay L) {
  const GateClk gc = gate_begin(gate);
  // the kernel-uniform qparams as scalar loads, after the x loads are issued
  fq_fwd_block<VEC, NT, CODES, MASK, ACT, U>(x, y, codes, mask, n, [&] { return load_qp<true>(src); }, blockIdx.x,
                                             gc, gate, L);
}

template <typename T, bool VEC, bool NT, bool CODES, bool MASK, int ACT, int U>
__global__ __launch_bounds__(kBlock) void k_fq_fwd_t(const T *__restrict__ x, T *__restrict__ y,
                                                     uint8_t *__restrict__ codes,
                                                     uint64_t *__restrict__ mask, int64_t n,
                                                     QPSrc src, uint32_t gate, SiluLay L) {
  const GateClk gc = gate_begin(gate);
  fq_fwd_block<VEC, NT, CODES, MASK, ACT, U>(x, y, codes, mask, n, [&] { return load_qp<true>(src); }, blockIdx.x,
                                             gc, gate, L);
}

template <typename T, bool VEC, bool NT, bool CODES, bool MASK, int ACT, int U>
constexpr auto fq_fwd_kernel() {
  if constexpr (std::is_same_v<T, float>) return &k_fq_fwd<VEC, NT, CODES, MASK, ACT, U>;
  else return &k_fq_fwd_t<T, VEC, NT, CODES, MASK, ACT, U>;
}

// One-round grids get the store gate (store_gate_select: >= 2 workgroups per CU, all
// resident): the kFlatU grid where it is one round (round 5: C4's 3.3M / 6.6M-element
// layers), else 9 groups per lane where that is (13M), else kFlatU ungated.
template <bool VEC, bool NT, bool CODES, bool MASK, int ACT, typename T>
void launch_fq_k(const T *x, T *y, uint8_t *codes, uint64_t *mask, int64_t n,
                 const QPSrc &src, const SiluLay &L, hipStream_t st) {
  const int64_t ng = cdiv(n, 4);
  const int64_t grid9 = cdiv(ng, (int64_t)kBlock * 9), gridu = oneshot_grid(ng);
  const auto k9 = fq_fwd_kernel<T, VEC, NT, CODES, MASK, ACT, 9>();
  const auto ku = fq_fwd_kernel<T, VEC, NT, CODES, MASK, ACT, kFlatU>();
  const void *kern9 = reinterpret_cast<const void *>(k9);
  const void *kernu = reinterpret_cast<const void *>(ku);
  static const int occ9 = occupancy_blocks(kern9, kBlock);
  static const int occu = occupancy_blocks(kernu, kBlock);
  const int64_t cus = device_cus();
  const int64_t bytes = (int64_t)sizeof(T) * n;   // the read phase the gate waits out
  GateSel gs;
  if (g_tune.store_gate != 0 && gridu >= 2 * cus && gridu <= (int64_t)occu * cus) {
    gs = store_gate_select("k1_fq_fwd_flat", kernu, gridu, occu, bytes, st);
  } else if (g_tune.store_gate != 0 && grid9 * kBlock * 9 - ng <= ng / 8 && grid9 >= 2 * cus &&
             grid9 <= (int64_t)occ9 * cus) {
    gs = store_gate_select("k1_fq_fwd", kern9, grid9, occ9, bytes, st);
    if (gs.gate) {
      hipLaunchKernelGGL(k9, dim3((unsigned)grid9), dim3(kBlock), 0, st, x, y, codes, mask, n, src, gs.gate, L);
      store_gate_launched(gs, st);
      return;
    }
  }
  hipLaunchKernelGGL(ku, dim3((unsigned)gridu), dim3(kBlock), 0, st, x, y, codes, mask, n, src, gs.gate, L);
  store_gate_launched(gs, st);   // for the 9-group site: a tuning sample of "no gate" times the kFlatU grid
}

template <typename T>
int fq_fwd(const T *x, T *y, void *codes, uint64_t *mask, int64_t n, int act,
           const double *qp_dev, const double *scale_dev, double scale_host, const double *zp_dev,
           double zp_host, int zp_round, int discrete, int qmin, int qmax, void *stream) {
  if (n < 0 || qmin > qmax || (n > 0 && (!x || !y)) || !act_ok(act))
    return VSIQ_E_ARG;
  if (n == 0) return 0;
  if (mask && !aligned8(mask)) return VSIQ_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  QPSrc src{qp_dev, scale_dev, zp_dev, scale_host, zp_host, (float)qmin, (float)qmax,
            qp_dev ? 0 : zp_round, discrete ? 1 : 0};
  const bool vec = (n % 4 == 0) && aligned_vec<T>(x) && aligned_vec<T>(y) && (!codes || aligned4(codes));
  const bool nt = g_tune.nontemporal != 0;
  uint8_t *c = (uint8_t *)codes;
  const SiluLay L = act_lay(act, n);
  with_act(act, [&](auto A) {   // all four (VEC, NT) pairs: the scalar path is non-temporal too
    with_vec_nt4(vec, nt, [&](auto V, auto N) {
      with_bool2(c != nullptr, mask != nullptr, [&](auto C, auto M) {
        launch_fq_k<decltype(V)::value, decltype(N)::value, decltype(C)::value, decltype(M)::value,
                    decltype(A)::value>(x, y, c, mask, n, src, L, st);
      });
    });
  });
  return launch_rc();
}

#define VSIQ_FQ_FWD_INST(T)                                                                                     \
  template int fq_fwd<T>(const T *, T *, void *, uint64_t *, int64_t, int, const double *, const double *,     \
                         double, const double *, double, int, int, int, int, void *)
extern VSIQ_FQ_FWD_INST(bf16_t);
extern VSIQ_FQ_FWD_INST(f16_t);

}  // namespace vsiq
