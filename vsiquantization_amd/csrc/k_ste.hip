// k_ste.hip — straight-through backward from the saved 1-bit mask: the fp32 kernels and
// the C ABI (kernel and launcher: k_ste.cuh; the bf16 / fp16 kernels: k_ste_half.hip).
#include "k_ste.cuh"

using namespace vsiq;

extern "C" {

int vsiq_ste_bwd_f32(const float *g, const uint64_t *mask, float *gx, int64_t n,
                     const double *scale_dev, int64_t rowlen, double scale_host, void *stream) {
  return ste_bwd<float>(g, mask, nullptr, gx, n, kActNone, scale_dev, rowlen, scale_host, stream);
}

int vsiq_act_ste_bwd_f32(const float *g, const uint64_t *mask, const float *c, float *gc, int64_t n,
                         int act, const double *scale_dev, int64_t rowlen, double scale_host,
                         void *stream) {
  return vsiq_act_ste_bwd_t(g, mask, c, gc, n, VSIQ_DT_F32, act, scale_dev, rowlen, scale_host, stream);
}

int vsiq_act_ste_bwd_t(const void *g, const uint64_t *mask, const void *c, void *gc, int64_t n, int dtype,
                       int act, const double *scale_dev, int64_t rowlen, double scale_host, void *stream) {
  if (!dtype_ok(dtype)) return VSIQ_E_ARG;
  return with_dtype(dtype, [&](auto D) {
    using T = typename decltype(D)::type;
    return ste_bwd<T>((const T *)g, mask, (const T *)c, (T *)gc, n, act, scale_dev, rowlen, scale_host, stream);
  });
}

}  // extern "C"
