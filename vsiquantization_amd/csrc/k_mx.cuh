// k_mx.cuh — OCP Microscaling (MX v1.0) element arithmetic of the host loops (k_host.hip),
// written __host__ __device__ so that a device kernel can share it unchanged (none is built
// yet: DESIGN.md §7).  32 elements share one power-of-two E8M0 scale X = 2^E; each
// element is a 4-, 6- or 8-bit float.  Nothing here is approximate (include/vsiq.h has
// the full statement):
//   code(scale) = max(exp_field(amax) - emax, 0)       E = code - 127 (floor(log2 amax) - emax,
//                                                       clamped at -127; never above 125)
//   a  = |v| * 2^-E                                     exact (a < 2^(emax+1))
//   q  = RNE(a) on the element grid                     ONE fp32 add of the power of two
//        2^(max(exp(a), emin) - mbits + 23) and its subtraction: the add's round-to-nearest-
//        even IS the grid's (the sum's ulp is the grid step, subnormal steps included)
//   q > max normal: the overflow value was picked -> q = max normal, mask bit 0
//   y  = copysign(q * 2^E, v)                           exact
// Every step but the one add is exponent-field / bit arithmetic on the fp32 pattern; fp32
// denormals are kept (the host runs without FTZ / DAZ).
#pragma once
#include "vsiq_common.cuh"

namespace vsiq {

// per-format constants; exponents are fp32-biased (+127)
struct MxFmt {
  int32_t emax;       // exponent of the largest binade
  int32_t emin_b;     // biased exponent of the smallest normal
  int32_t mbits;      // mantissa bits
  int32_t sign_bit;   // position of the sign in the element code
  uint32_t maxn;      // fp32 pattern of the largest normal
};

inline bool mx_fmt_ok(int fmt) { return fmt >= VSIQ_MX_FP4_E2M1 && fmt <= VSIQ_MX_FP8_E5M2; }

inline MxFmt mx_fmt(int fmt) {
  switch (fmt) {
    case VSIQ_MX_FP4_E2M1: return MxFmt{2, 127, 1, 3, 0x40c00000u};        // 6
    case VSIQ_MX_FP6_E2M3: return MxFmt{2, 127, 3, 5, 0x40f00000u};        // 7.5
    case VSIQ_MX_FP6_E3M2: return MxFmt{4, 127 - 2, 2, 5, 0x41e00000u};    // 28
    case VSIQ_MX_FP8_E4M3: return MxFmt{8, 127 - 6, 3, 7, 0x43e00000u};    // 448
    default: return MxFmt{15, 127 - 14, 2, 7, 0x47600000u};                // FP8_E5M2: 57344
  }
}

// the block's shared scale from the largest |v| pattern of its elements (sign bit cleared;
// unsigned patterns order like magnitudes, NaN above Inf above every finite value)
struct MxScale {
  uint32_t code;   // E8M0 byte: E + 127; 255 for a block holding a NaN or an Inf
  float inv, x;    // 2^-E, 2^E
};

__host__ __device__ __forceinline__ MxScale mx_scale(uint32_t amax_bits, const MxFmt &f) {
  MxScale s;
  if (amax_bits >= 0x7f800000u) {
    s.code = 255u;
    s.inv = s.x = u2f(0x7fc00000u);
    return s;
  }
  const int32_t c = (int32_t)(amax_bits >> 23) - f.emax;   // an fp32-denormal amax: field 0, clamped
  s.code = (uint32_t)(c > 0 ? c : 0);
  s.inv = u2f((254u - s.code) << 23);                       // 2^(127 - code): always normal
  s.x = u2f(s.code ? s.code << 23 : 0x00400000u);           // 2^(code - 127); code 0: the denormal 2^-127
  return s;
}

struct MxElem {
  float y;
  uint32_t code;   // sign | exponent | mantissa fields of q
  bool m;          // 1 = rounding did not pick the overflow value
};

template <bool CODE>
__host__ __device__ __forceinline__ MxElem mx_elem(float v, const MxScale &s, const MxFmt &f) {
  MxElem o;
  if (s.code == 255u) {   // NaN scale: the whole block is NaN (block-uniform branch)
    o.y = u2f(0x7fc00000u);
    o.code = 0u;
    o.m = false;
    return o;
  }
  const uint32_t uv = f2u(v), sign = uv & 0x80000000u;
  const float a = u2f(uv & 0x7fffffffu) * s.inv;
  const int32_t ea = (int32_t)(f2u(a) >> 23);
  const float big = u2f((uint32_t)((ea > f.emin_b ? ea : f.emin_b) + 23 - f.mbits) << 23);
  const float r = (a + big) - big;
  const uint32_t ur = f2u(r);
  o.m = ur <= f.maxn;
  const uint32_t uq = o.m ? ur : f.maxn;
  o.y = u2f(f2u(u2f(uq) * s.x) | sign);
  o.code = 0u;
  if constexpr (CODE) {
    const int32_t eq = (int32_t)(uq >> 23);
    uint32_t c;
    if (eq >= f.emin_b) {   // normal: exponent field from 1, the top mantissa bits
      c = ((uint32_t)(eq - f.emin_b + 1) << f.mbits) | ((uq >> (23 - f.mbits)) & ((1u << f.mbits) - 1u));
    } else {                // subnormal or zero: q / 2^(emin - mbits) in the low bits of the sum
      const float sub = u2f((uint32_t)(f.emin_b + 23 - f.mbits) << 23);
      c = f2u(u2f(uq) + sub) & ((1u << f.mbits) - 1u);
    }
    o.code = c | ((sign >> 31) << f.sign_bit);
  }
  return o;
}

// scales of a [rows, rowlen] call: one per started block of 32 of every row
__host__ __device__ inline int64_t mx_row_blocks(int64_t rowlen) { return cdiv(rowlen, 32); }

}  // namespace vsiq
