// k_pg_wave.cuh — the wave-per-chunk lane mapping of the group-wise kernels, shared by
// k_pg.hip (observe + fake quant, fixed forward, STE and LSQ backward) and k_pg_mse.hip (the
// per-group MSE search): where a wave works and what it loads (pg_task, pg_load), the reduction
// over a group's lanes (pg_reduce, pg_range), a task's outputs between its arithmetic and its
// stores (pg_quantize, pg_store_row, pg_store) and, on the host, what every entry opens with (pg_enter) and
// the launch forms (pg_grid, with_pg_form).  k_pg.hip's header comment states the mapping.
#pragma once
#include "dispatch.cuh"
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

// this lane's 4 elements of a task from the row-major tensor p; a lane past the row end loads
// (clamped) the row's last 4 elements
template <bool VEC>
__device__ __forceinline__ f4 pg_load(const float *__restrict__ p, const PGTask &k, const PGView &v) {
  return load_group_c<VEC, VEC>(p + k.row * v.rowlen, k.i, k.ng, v.rowlen);
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

// A group's min / max / NaN flag from its lanes' elements (lanes past the row end replicate
// members of the row's last group).  SEED: an all-NaN group gives (inf, -inf), as k_pc_mse.hip
// reduces a row; without it mn / mx of such a group are NaN and not to be read.  seg: the
// group's first lane, lane & ~(gl - 1); segmask: its gl lanes as a mask at bit 0 -- both by
// reference: by value, k_pg_mse's owner test comes out with its s_and operands swapped.
struct PGRange {
  float mn, mx;
  bool nan;
};

template <bool SEED>
__device__ __forceinline__ PGRange pg_range(const f4 &e, const PGView &v, const uint32_t &seg,
                                            const uint64_t &segmask) {
  float mn = fminf(fminf(e.x, e.y), fminf(e.z, e.w));
  float mx = fmaxf(fmaxf(e.x, e.y), fmaxf(e.z, e.w));
  if (SEED) {
    mn = fminf(__builtin_inff(), mn);
    mx = fmaxf(-__builtin_inff(), mx);
  }
  const bool nanl = (e.x != e.x) | (e.y != e.y) | (e.z != e.z) | (e.w != e.w);
  return {pg_reduce(mn, v.gl, MinOp()), pg_reduce(mx, v.gl, MaxOp()), ((__ballot(nanl) >> seg) & segmask) != 0};
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

// this lane's 4 elements of a live task into a row-major fp32 output; a lane past the row end stores nothing
template <bool VEC>
__device__ __forceinline__ void pg_store_row(const PGTask &k, const PGView &v, float *__restrict__ out, const f4 &o) {
  if (k.live && k.i < k.ng) store_group<VEC, VEC>(out + k.row * v.rowlen, k.i, v.rowlen, o);
}

template <bool VEC, bool CODES, bool MASK>
__device__ __forceinline__ void pg_store(const PGTask &k, const PGView &v, float *__restrict__ y,
                                         uint8_t *__restrict__ codes, uint64_t *__restrict__ mask,
                                         const PGOut &r) {
  pg_store_row<VEC>(k, v, y, r.o);
  if (!k.live) return;
  if (CODES && k.i < k.ng) {
    uint8_t *cr = codes + k.row * v.rowlen;
    if (VEC) reinterpret_cast<uint32_t *>(cr)[k.i] = r.c;
    else
      for (int j = 0; j < valid_in_group(k.i, v.rowlen); ++j) cr[4 * k.i + j] = (uint8_t)(r.c >> (8 * j));
  }
  if (MASK && threadIdx.x % kWave < 4)
    mask[k.row * mask_words_per_row(v.rowlen) + 4 * (int64_t)k.chunk + threadIdx.x % kWave] = r.mw;
}

// host: what every entry opens with.  False where the entry returns *rc at once, in this
// order: an argument error (`args_ok`: the entry's own value checks), 0 for no rows, an
// argument error for a missing pointer (`ptrs_ok`) or more than 2^31 - 1 tasks, the mask's
// alignment (null: no mask).  Else true, *rc 0 and the view.
inline bool pg_enter(int64_t rows, int64_t rowlen, int64_t group, bool args_ok, bool ptrs_ok, const void *mask,
                     PGView *v, int *rc) {
  const int64_t cpr = cdiv(rowlen, 4 * kWave);
  *rc = rows < 0 || rowlen <= 0 || !pg_group_ok(group) || !args_ok ? VSIQ_E_ARG
        : rows == 0 ? 0
        : !ptrs_ok || rows > 0x7fffffffLL || cpr > 0x7fffffffLL || rows * cpr > 0x7fffffffLL ? VSIQ_E_ARG
        : !aligned8(mask) ? VSIQ_E_ALIGN : 0;
  if (*rc || rows == 0) return false;
  *v = PGView{rowlen, pg_groups_per_row(rowlen, group), (uint32_t)(rows * cpr), (uint32_t)cpr, (uint32_t)(group / 4)};
  return true;
}

// host: the grid of workgroups of kWaves * u tasks
inline dim3 pg_grid(const PGView &v, int u) { return dim3((unsigned)cdiv(v.tasks, (int64_t)kWaves * u), 1, 1); }

constexpr int kPgU = 4;  // tasks per wave where the grid still fills the device (else 1)

inline int pg_per_wave(const PGView &v) {
  return (int64_t)v.tasks >= (int64_t)kWaves * kPgU * 4 * device_cus() ? kPgU : 1;
}

// host: f(VEC, U) over the three launch forms -- the scalar path, the vector path with 1 task
// per wave, the vector path with kPgU (dispatch.cuh's tags)
template <class F>
decltype(auto) with_pg_form(bool vec, const PGView &v, F &&f) {
  return !vec ? f(BoolC<false>{}, IntC<1>{})
              : pg_per_wave(v) == kPgU ? f(BoolC<true>{}, IntC<kPgU>{}) : f(BoolC<true>{}, IntC<1>{});
}

}  // namespace vsiq
