// k_rot.cuh — hadamard_G (include/vsiq.h) on a lane's four values with the group spread over GL =
// G / 4 adjacent lanes, shared by k_rot.hip (the group-wise kernels) and k_mx_rot.hip (the MX
// row kernels, GL = 8).  k_rot.hip's header comment states where each stage's partner comes from.
#pragma once
#include "vsiq_common.cuh"

namespace vsiq {

// ----------------------------------------------------------------------------
// hadamard_G on the lane's four values
// ----------------------------------------------------------------------------
template <int GL>
struct RotC;   // c_G = (float)(1.0 / sqrt((double)G)), G = 4 * GL
template <> struct RotC<8> { static constexpr float c = (float)0.17677669529663688; };
template <> struct RotC<16> { static constexpr float c = 0.125f; };
template <> struct RotC<32> { static constexpr float c = (float)0.08838834764831845; };
template <> struct RotC<64> { static constexpr float c = 0.0625f; };

// the sign flips of the DPP / swizzle stages: bit 31 set in the lanes whose bit k is set
struct RotSign {
  uint32_t b0, b1, b2, b3;
};

__device__ __forceinline__ RotSign rot_sign() {
  const uint32_t lane = threadIdx.x % kWave;
  return {(lane & 1u) << 31, (lane & 2u) << 30, (lane & 4u) << 29, (lane & 8u) << 28};
}

__device__ __forceinline__ float rot_flip(float v, uint32_t s) { return __uint_as_float(__float_as_uint(v) ^ s); }

template <int CTRL>
__device__ __forceinline__ float rot_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// own + partner in the lanes with the stage's bit clear, partner - own in the others
template <int CTRL>
__device__ __forceinline__ void rot_stage_dpp(f4 &v, uint32_t s) {
  v.x = rot_dpp<CTRL>(v.x) + rot_flip(v.x, s);
  v.y = rot_dpp<CTRL>(v.y) + rot_flip(v.y, s);
  v.z = rot_dpp<CTRL>(v.z) + rot_flip(v.z, s);
  v.w = rot_dpp<CTRL>(v.w) + rot_flip(v.w, s);
}

__device__ __forceinline__ float rot_swz4(float v) {   // lane ^ 4: bit mode, and 0x1f, or 0, xor 4
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (4 << 10) | 0x1F));
}

__device__ __forceinline__ void rot_stage_swz4(f4 &v, uint32_t s) {
  v.x = rot_swz4(v.x) + rot_flip(v.x, s);
  v.y = rot_swz4(v.y) + rot_flip(v.y, s);
  v.z = rot_swz4(v.z) + rot_flip(v.z, s);
  v.w = rot_swz4(v.w) + rot_flip(v.w, s);
}

// lane ^ 16 (HALF false) or lane ^ 32 (HALF true) on two of the lane's elements at once
template <bool HALF>
__device__ __forceinline__ void rot_swap(uint32_t &a, uint32_t &b) {
  if constexpr (HALF) {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
  } else {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0];
    b = r[1];
  }
}

template <bool HALF>
__device__ __forceinline__ void rot_swap_pair(float &a, float &b) {
  uint32_t ua = __float_as_uint(a), ub = __float_as_uint(b);
  rot_swap<HALF>(ua, ub);   // ua: (a, b) of the lower lanes; ub: (a, b) of the upper lanes
  uint32_t s = __float_as_uint(__uint_as_float(ua) + __uint_as_float(ub));
  uint32_t d = __float_as_uint(__uint_as_float(ua) - __uint_as_float(ub));
  rot_swap<HALF>(s, d);     // s: a's sum and difference; d: b's
  a = __uint_as_float(s);
  b = __uint_as_float(d);
}

template <bool HALF>
__device__ __forceinline__ void rot_stage_swap(f4 &v) {
  float x = v.x, y = v.y, z = v.z, w = v.w;
  rot_swap_pair<HALF>(x, y);
  rot_swap_pair<HALF>(z, w);
  v.x = x; v.y = y; v.z = z; v.w = w;
}

template <int GL>
__device__ __forceinline__ f4 rot_hadamard(f4 v, const RotSign &g) {
  static_assert(GL == 8 || GL == 16 || GL == 32 || GL == 64, "lanes per group");
  f4 t;
  t.x = v.x + v.y; t.y = v.x - v.y; t.z = v.z + v.w; t.w = v.z - v.w;   // h = 1
  v.x = t.x + t.z; v.y = t.y + t.w; v.z = t.x - t.z; v.w = t.y - t.w;   // h = 2
  rot_stage_dpp<0xB1>(v, g.b0);    // h = 4: quad_perm [1,0,3,2]
  rot_stage_dpp<0x4E>(v, g.b1);    // h = 8: quad_perm [2,3,0,1]
  rot_stage_swz4(v, g.b2);         // h = 16
  if constexpr (GL >= 16) rot_stage_dpp<0x128>(v, g.b3);   // h = 32: row_ror:8
  if constexpr (GL >= 32) rot_stage_swap<false>(v);        // h = 64
  if constexpr (GL >= 64) rot_stage_swap<true>(v);         // h = 128
  constexpr float c = RotC<GL>::c;
  v.x *= c; v.y *= c; v.z *= c; v.w *= c;
  // A NaN result is the canonical quiet NaN.  Two NaNs of different sign can meet in an add (the
  // subtractions and the sign flips make them), and which one it returns depends on the operand
  // order the compiler picked; results that are not NaN never depend on one.  Wave-uniform test:
  // two v_cmp_u per lane, the rewrite only in a wave that holds a NaN.
  if (__ballot(__builtin_isunordered(v.x, v.y) | __builtin_isunordered(v.z, v.w))) {
    const float qnan = __uint_as_float(0x7FC00000u);
    v.x = v.x != v.x ? qnan : v.x;
    v.y = v.y != v.y ? qnan : v.y;
    v.z = v.z != v.z ? qnan : v.z;
    v.w = v.w != v.w ? qnan : v.w;
  }
  return v;
}

}  // namespace vsiq
