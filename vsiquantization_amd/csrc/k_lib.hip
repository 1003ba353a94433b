// k_lib.hip — the library-level C ABI: tuning, ABI version, error strings, workspace / mask
// sizes, the device attribute caches, and the two exhaustive self-tests (division, fast paths).
#include "vsiq_common.cuh"

namespace vsiq {

Tuning g_tune;

// ----------------------------------------------------------------------------
// exhaustive check of fdiv against the IEEE division: every 32-bit pattern a,
// for each divisor b[k]; counts bitwise mismatches (NaNs compare by NaN-ness)
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_selftest_div(const float *__restrict__ bs, int nb,
                                                         unsigned long long *__restrict__ bad) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (int k = 0; k < nb; ++k) {
    const FastDiv d = make_fastdiv(bs[k]);
    uint32_t cnt = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < (1ull << 32); i += stride) {
      const float a = __uint_as_float((uint32_t)i);
      const float q = fdiv(a, d), w = a / d.b;
      const bool same = (__float_as_uint(q) == __float_as_uint(w)) || (q != q && w != w);
      cnt += same ? 0u : 1u;
    }
    cnt = wave_reduce(cnt, AddU());
    if (threadIdx.x % kWave == 0 && cnt) atomicAdd(bad + k, (unsigned long long)cnt);
  }
}


// exhaustive check of the no-check fast paths, every 32-bit input pattern:
//   mode 0: quantizer code c = clamp(rint(x/s + zp)) (value, sign, STE mask bit)
//           of fq_elem_fast vs the IEEE element, for x with fq_x_ok(x), per
//           (scales[k], zps[k]) inside fq_fast_qp;
//   mode 1: STE quotient ste_quot(g) vs RN(RN(g*s)/s), for g with ste_ok(g).
// counts[2k] = mismatches, counts[2k+1] = inputs checked (0 if the qparams are
// outside the fast domain).
__global__ __launch_bounds__(kBlock) void k_selftest_fq(int mode, const float *__restrict__ ss,
                                                        const float *__restrict__ zs, int nk, float lo,
                                                        float hi, unsigned long long *__restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (int k = 0; k < nk; ++k) {
    const QP p = make_qp(ss[k], mode == 0 ? zs[k] : 0.f, lo, hi, 1);
    const SteDiv sd = make_stediv(p.s);
    const bool dom = mode == 0 ? p.fast != 0 : sd.fast != 0;
    uint32_t bad = 0, seen = 0;
    if (dom) {
      for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = __uint_as_float((uint32_t)i);
        if (mode == 0) {
          if (!fq_x_ok(x)) continue;
          const Elem f = fq_elem_fast(x, p), w = fq_elem<true>(x, p);
          bad += (__float_as_uint(f.y) != __float_as_uint(w.y) || f.m != w.m) ? 1u : 0u;
        } else {
          if (!ste_ok(x)) continue;
          const float f = ste_quot(x, sd), w = ste_ieee(x, true, sd);
          bad += (__float_as_uint(f) != __float_as_uint(w) && !(f != f && w != w)) ? 1u : 0u;
        }
        ++seen;
      }
    }
    bad = wave_reduce(bad, AddU());
    seen = wave_reduce(seen, AddU());
    if (threadIdx.x % kWave == 0) {
      if (bad) atomicAdd(out + 2 * k, (unsigned long long)bad);
      if (seen) atomicAdd(out + 2 * k + 1, (unsigned long long)seen);
    }
  }
}

// CU count of the current device (cached; 256 on MI355X)
int occupancy_blocks(const void *kernel, int block) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block, 0) != hipSuccess) return 0;
  return n;
}

// per-device attribute caches: relaxed atomics (any thread may fill them; the value
// is the same whoever wins)
int device_wall_clock_khz() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 100000;
  return device_wall_clock_khz(dev);
}

int device_wall_clock_khz(int dev) {
  static std::atomic<int> khz[64];
  if (dev < 0 || dev >= 64) return 100000;
  if (!khz[dev]) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, dev) != hipSuccess || v <= 0) v = 100000;
    khz[dev] = v;
  }
  return khz[dev];
}

int device_cus() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  return device_cus(dev);
}

int device_cus(int dev) {
  static std::atomic<int> cus[64];
  if (dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cus[dev] = v;
  }
  return cus[dev];
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_abi_version(void) { return VSIQ_ABI_VERSION; }

const char *vsiq_error_string(int code) {
  switch (code) {
    case 0: return "success";
    case VSIQ_E_ARG: return "vsiq: invalid argument";
    case VSIQ_E_ALIGN: return "vsiq: misaligned pointer";
    case VSIQ_E_WS: return "vsiq: workspace too small";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "vsiq: unknown error";
  }
}

int64_t vsiq_workspace_doubles(int64_t n) {
  // the largest reducing grid any kernel / tuning can use for n: 2 groups per lane (K4
  // and the one-shot K2 at VSIQ_TUNE_LSQ_GROUPS 2; the one-shot K2 runs K4's 8 as 4)
  const int64_t g = std::max<int64_t>(kMaxReduceGrid, lsq_grid(cdiv(std::max<int64_t>(n, 0), 4), 2));
  return (g + kArriveGroups) * kPartials;
}

int64_t vsiq_mask_words(int64_t rows, int64_t rowlen) {
  if (rows < 0 || rowlen < 0) return VSIQ_E_ARG;
  return rows * mask_words_per_row(rowlen);
}

int vsiq_set_tuning(int key, int value) {
  switch (key) {
    case VSIQ_TUNE_NONTEMPORAL: g_tune.nontemporal = value; return 0;
    case VSIQ_TUNE_OBS_KERNEL:
      if (value < 0 || value > 2) return VSIQ_E_ARG;
      g_tune.obs_kernel = value;
      return 0;
    case VSIQ_TUNE_LSQ_GROUPS:
      if (value != 0 && value != 2 && value != 4 && value != 8 && value != 16) return VSIQ_E_ARG;
      g_tune.lsq_groups = value;
      return 0;
    case VSIQ_TUNE_STORE_DEFER:
      if (value < -1 || value > 64) return VSIQ_E_ARG;
      g_tune.store_defer = value;
      return 0;
    case VSIQ_TUNE_PC_PACKED:
      if (value < 0 || value > 2) return VSIQ_E_ARG;
      g_tune.pc_packed = value;
      return 0;
    case VSIQ_TUNE_STORE_GATE:
      if (value < -1 || value > 4000) return VSIQ_E_ARG;
      g_tune.store_gate = value;
      return 0;
    case VSIQ_TUNE_GATE_AUTOTUNE:
      if (value != 0 && value != 1) return VSIQ_E_ARG;
      g_tune.gate_autotune = value;
      return 0;
    case VSIQ_TUNE_XCD_ORDER:
      if (value < 0 || value > 2) return VSIQ_E_ARG;
      g_tune.xcd_order = value;
      return 0;
    case VSIQ_TUNE_K2O_FORM:
      if (value != 0 && value != 1) return VSIQ_E_ARG;
      g_tune.k2o_form = value;
      return 0;
    case VSIQ_TUNE_K2O_GROUPS:
      if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8 && value != 16) return VSIQ_E_ARG;
      g_tune.k2o_groups = value;
      return 0;
    case VSIQ_TUNE_K2O_BLOCK:
      if (value != 0 && value != 256 && value != 512 && value != 1024) return VSIQ_E_ARG;
      g_tune.k2o_block = value;
      return 0;
    default: return VSIQ_E_ARG;
  }
}

int vsiq_selftest_div(const float *divisors, int count, unsigned long long *mismatches,
                      void *stream) {
  if (count < 0 || (count > 0 && (!divisors || !mismatches))) return VSIQ_E_ARG;
  if (count == 0) return 0;
  hipLaunchKernelGGL(k_selftest_div, dim3(256 * 16), dim3(kBlock), 0, (hipStream_t)stream,
                     divisors, count, mismatches);
  return launch_rc();
}

int vsiq_selftest_fq(int mode, const float *scales, const float *zero_points, int count,
                     float qmin, float qmax, unsigned long long *counts, void *stream) {
  if (mode != 0 && mode != 1) return VSIQ_E_ARG;
  if (count < 0 || (count > 0 && (!scales || !counts || (mode == 0 && !zero_points))))
    return VSIQ_E_ARG;
  if (count == 0) return 0;
  hipLaunchKernelGGL(k_selftest_fq, dim3(256 * 16), dim3(kBlock), 0, (hipStream_t)stream, mode,
                     scales, zero_points, count, qmin, qmax, counts);
  return launch_rc();
}

}  // extern "C"
