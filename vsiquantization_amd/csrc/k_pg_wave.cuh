// k_pg_wave.cuh — the wave-per-chunk lane mapping of the group-wise kernels, shared by
// k_pg.hip (observe + fake quant, fixed forward, STE and LSQ backward) and k_pg_mse.hip (the
// per-group MSE search): where a wave works (pg_task), the reduction over a group's lanes
// (pg_reduce) and a task's outputs between its arithmetic and its stores (pg_quantize,
// pg_store).  k_pg.hip's header comment states the mapping.
#pragma once
#include "k_body.cuh"
#include "k_pg.cuh"
#include "vsiq_common.cuh"

namespace vsiq {

struct PGView {
  int64_t rowlen, ngr;   // elements per row, groups per row
  uint32_t tasks, cpr;   // rows * cpr wave tasks, 256-element chunks per row
  uint32_t gl;           // lanes per group: group / 4 = 8, 16, 32, 64
};

// where a wave works: task t of the view (clamped into the grid; `live` false past it)
struct PGTask {
  int64_t row, i, ng;    // row, this lane's 4-element group in the row (unclamped), groups of 4 in the row
  int64_t qi;            // index of this lane's quantization group in the [rows, ngr] arrays (clamped)
  uint32_t chunk;
  bool live, qvalid;     // the wave's task exists; this lane's quantization group exists
};

template <int U>
__device__ __forceinline__ PGTask pg_task(const PGView &v, int u) {
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const uint32_t t = blockIdx.x * (uint32_t)(kWaves * U) + (uint32_t)u * kWaves + wave;   // <= tasks + 4U < 2^32
  PGTask k;
  k.live = t < v.tasks;
  const uint32_t tc = k.live ? t : v.tasks - 1;
  k.row = tc / v.cpr;
  k.chunk = tc % v.cpr;
  k.ng = cdiv(v.rowlen, 4);
  k.i = (int64_t)k.chunk * kWave + lane;
  const int64_t j = (int64_t)k.chunk * (kWave / v.gl) + lane / v.gl;
  k.qvalid = j < v.ngr;
  k.qi = k.row * v.ngr + (k.qvalid ? j : v.ngr - 1);
  return k;
}

// min / max (fp32) or sum (f64: every DPP step and lane read on both 32-bit halves) over the
// `gl` adjacent lanes of a group, returned to each of them, in a fixed tree.  Whole wave
// active (every call site is wave-uniform); gl is kernel-uniform.  No step reads a lane of
// another group, so one group's value never enters another's result.
template <typename T>
__device__ __forceinline__ T pg_readlane(T v, int lane) {
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
  } else {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
    return __builtin_bit_cast(T, ((uint64_t)hi << 32) | lo);
  }
}

template <typename T, typename Op>
__device__ __forceinline__ T pg_reduce(T v, uint32_t gl, Op op) {
  const T id = Op::identity();
  v = op(v, dpp<0xB1>(v, id));    // quad_perm [1,0,3,2]
  v = op(v, dpp<0x4E>(v, id));    // quad_perm [2,3,0,1]
  v = op(v, dpp<0x141>(v, id));   // row_half_mirror -> every lane: its 8 lanes'
  if (gl >= 16) v = op(v, dpp<0x140>(v, id));   // row_mirror -> its 16-lane row's
  if (gl >= 32) {
    const T r0 = pg_readlane(v, 0), r1 = pg_readlane(v, 16), r2 = pg_readlane(v, 32), r3 = pg_readlane(v, 48);
    const T a = op(r0, r1), b = op(r2, r3);
    v = gl == 64 ? op(a, b) : (threadIdx.x % kWave < 32 ? a : b);
  }
  return v;
}

// One task's outputs between its arithmetic and its stores: y, the 4 code bytes and, in lanes
// 0..3, the chunk's mask word 0..3 (the four ballots are wave-uniform SGPR pairs; each of the
// four storing lanes takes its own into a VGPR pair at once, so no ballot stays live across
// the other tasks' arithmetic).
struct PGOut {
  f4 o;
  uint32_t c;
  uint64_t mw;
};

template <bool VEC, bool CODES, bool MASK>
__device__ __forceinline__ PGOut pg_quantize(f4 e, const QP &p, const PGTask &k, const PGView &v) {
  const GroupOut g = fq_out_flat<VEC, CODES, MASK>(e, p, k.i, v.rowlen);
  const uint32_t lane = threadIdx.x % kWave;
  PGOut r;
  r.o = g.o;
  r.c = g.c;
  r.mw = MASK ? (lane == 0 ? g.b[0] : lane == 1 ? g.b[1] : lane == 2 ? g.b[2] : g.b[3]) : 0;
  return r;
}

template <bool VEC, bool CODES, bool MASK>
__device__ __forceinline__ void pg_store(const PGTask &k, const PGView &v, float *__restrict__ y,
                                         uint8_t *__restrict__ codes, uint64_t *__restrict__ mask,
                                         const PGOut &r) {
  if (!k.live) return;
  if (k.i < k.ng) {
    store_group<VEC, VEC>(y + k.row * v.rowlen, k.i, v.rowlen, r.o);
    if (CODES) {
      uint8_t *cr = codes + k.row * v.rowlen;
      if (VEC) reinterpret_cast<uint32_t *>(cr)[k.i] = r.c;
      else
        for (int j = 0; j < valid_in_group(k.i, v.rowlen); ++j) cr[4 * k.i + j] = (uint8_t)(r.c >> (8 * j));
    }
  }
  if (MASK && threadIdx.x % kWave < 4)
    mask[k.row * mask_words_per_row(v.rowlen) + 4 * (int64_t)k.chunk + threadIdx.x % kWave] = r.mw;
}

// host: rc 0 and the view, or an argument error (rows > 0 here)
inline int pg_view(int64_t rows, int64_t rowlen, int64_t group, PGView *v) {
  const int64_t cpr = cdiv(rowlen, 4 * kWave);
  if (rows > 0x7fffffffLL || cpr > 0x7fffffffLL || rows * cpr > 0x7fffffffLL) return VSIQ_E_ARG;
  v->rowlen = rowlen;
  v->ngr = pg_groups_per_row(rowlen, group);
  v->tasks = (uint32_t)(rows * cpr);
  v->cpr = (uint32_t)cpr;
  v->gl = (uint32_t)(group / 4);
  return 0;
}

// host: the grid of workgroups of kWaves * u tasks
inline dim3 pg_grid(const PGView &v, int u) { return dim3((unsigned)cdiv(v.tasks, (int64_t)kWaves * u), 1, 1); }

}  // namespace vsiq
