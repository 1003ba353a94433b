// k_fq.hip — K1 per-tensor fake-quant forward (optionally behind a fused ReLU/SiLU,
// K5): the fp32 kernels and the C ABI entry points (kernel and launcher: k_fq.cuh; the
// bf16 / fp16 kernels: k_fq_half.hip).
#include "k_fq.cuh"

using namespace vsiq;

extern "C" {

int vsiq_fq_fwd_f32(const float *x, float *y, void *codes, uint64_t *mask, int64_t n,
                    const double *qp_dev, const double *scale_dev, double scale_host,
                    const double *zp_dev, double zp_host, int zp_round, int discrete, int qmin,
                    int qmax, void *stream) {
  return fq_fwd<float>(x, y, codes, mask, n, kActNone, qp_dev, scale_dev, scale_host, zp_dev, zp_host,
                       zp_round, discrete, qmin, qmax, stream);
}

int vsiq_act_fq_fwd_f32(const float *c, float *y, void *codes, uint64_t *mask, int64_t n, int act,
                        const double *qp_dev, const double *scale_dev, double scale_host,
                        const double *zp_dev, double zp_host, int zp_round, int discrete, int qmin,
                        int qmax, void *stream) {
  return vsiq_act_fq_fwd_t(c, y, codes, mask, n, VSIQ_DT_F32, act, qp_dev, scale_dev, scale_host, zp_dev,
                           zp_host, zp_round, discrete, qmin, qmax, stream);
}

int vsiq_act_fq_fwd_t(const void *c, void *y, void *codes, uint64_t *mask, int64_t n, int dtype, int act,
                      const double *qp_dev, const double *scale_dev, double scale_host,
                      const double *zp_dev, double zp_host, int zp_round, int discrete, int qmin,
                      int qmax, void *stream) {
  if (!dtype_ok(dtype)) return VSIQ_E_ARG;
  return with_dtype(dtype, [&](auto D) {
    using T = typename decltype(D)::type;
    return fq_fwd<T>((const T *)c, (T *)y, codes, mask, n, act, qp_dev, scale_dev, scale_host, zp_dev, zp_host,
                     zp_round, discrete, qmin, qmax, stream);
  });
}

}  // extern "C"
