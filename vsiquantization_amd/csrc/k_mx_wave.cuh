// k_mx_wave.cuh — what the MX device kernels (k_mx.hip, k_mx_rot.hip) share around k_mx.cuh's
// element code: the block maximum's operands, a lane's four elements through mx_elem, and the
// wave's four mask ballots.
#pragma once
#include "k_mx.cuh"

namespace vsiq {

struct MxMaxBits {
  static __device__ uint32_t identity() { return 0u; }
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};

__device__ __forceinline__ uint32_t mx_abs_bits(float v) { return f2u(v) & 0x7fffffffu; }

// a lane's 4 elements with their scales: y, the 4 code bytes, the 4 mask bits
struct MxQuad {
  f4 y;
  uint32_t c;
  bool m[4];
};

template <bool CODES>
__device__ __forceinline__ MxQuad mx_quad(const f4 &v, const MxScale &s0, const MxScale &s1, const MxScale &s2,
                                          const MxScale &s3, const MxFmt &f) {
  const MxElem a = mx_elem<CODES>(v.x, s0, f), b = mx_elem<CODES>(v.y, s1, f), c = mx_elem<CODES>(v.z, s2, f),
               d = mx_elem<CODES>(v.w, s3, f);
  MxQuad q;
  q.y.x = a.y; q.y.y = b.y; q.y.z = c.y; q.y.w = d.y;
  q.c = a.code | (b.code << 8) | (c.code << 16) | (d.code << 24);
  q.m[0] = a.m; q.m[1] = b.m; q.m[2] = c.m; q.m[3] = d.m;
  return q;
}

// the wave's four ballots of (m[j] and element j of the lane exists: nv of its 4 do), word j in lane j
__device__ __forceinline__ uint64_t mx_mask_word(const bool (&m)[4], int nv) {
  const uint64_t b0 = __ballot(m[0] && nv > 0), b1 = __ballot(m[1] && nv > 1), b2 = __ballot(m[2] && nv > 2),
                 b3 = __ballot(m[3] && nv > 3);
  const uint32_t lane = threadIdx.x % kWave;
  return lane == 0 ? b0 : lane == 1 ? b1 : lane == 2 ? b2 : b3;
}

// columns: lanes along inner, every lane its 4 blocks' <= 32 channels in registers
struct MxCols {
  int64_t channels, inner;
  uint32_t cb, cpr, tasks;   // channel blocks, 256-position chunks of inner, outer * cb * cpr wave tasks
};

}  // namespace vsiq
