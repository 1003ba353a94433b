// k_pg.hip — group-wise (per-group) weight quantization: observe + qparams + fake quant in
// one launch (vsiq_pg_observe_fq_f32), the forward with given [rows, ngr] qparams
// (vsiq_pg_fq_fwd_f32), the STE backward (vsiq_pg_ste_bwd_f32) and the learnable (LSQ)
// backward with per-group scale / zero-point gradients (vsiq_pg_lsq_bwd_f32).  Layout: k_pg.cuh.
//
// Lane mapping (all three kernels).  A wave takes one 256-element chunk of one row: lane l
// of the wave on chunk c of row r owns elements 256c + 4l .. 256c + 4l + 3 of that row, the
// mapping the 1-bit mask layout is built on (include/vsiq.h), so the wave's four ballots ARE
// the chunk's four mask words and the mask keeps the whole tensor's (rows, rowlen) layout.
// A quantization group of G = 32 / 64 / 128 / 256 elements is G/4 = 8 / 16 / 32 / 64
// adjacent lanes of that wave and never crosses a wave, because 256 % G == 0 and groups
// restart with the row: its min / max is reduced with DPP steps and lane reads inside the
// wave (no LDS, no barrier, no exchange between workgroups).  The "tasks" (row, chunk) are
// numbered row-major, t = r * chunks_per_row + c, and a workgroup's four waves take 4 * U
// consecutive tasks: whole short rows, or a 256-aligned piece of a long row.  Every wave is
// full except on a row's last chunk, whose lanes past the row end load (clamped) the row's
// last 4 elements -- members of the row's last group, so they change neither its min / max
// nor its NaN flag -- and store nothing.  That is also how a row's short last group is
// handled: by lanes that do not store, not by a second launch.
//
// One store policy: the vector path streams with nontemporal loads and stores, the arm K3
// takes at the tuning knob's default; the scalar path (rowlen % 4 != 0 or unaligned
// pointers: per-element accesses of the same lanes) uses plain ones, as K3's does.  This
// file does not read the knob.
#include "k_body.cuh"
#include "k_pg.cuh"
#include "vsiq_common.cuh"

namespace vsiq {

struct PGView {
  int64_t rowlen, ngr;   // elements per row, groups per row
  uint32_t tasks, cpr;   // rows * cpr wave tasks, 256-element chunks per row
  uint32_t gl;           // lanes per group: group / 4 = 8, 16, 32, 64
};

struct PGObs {
  float *run_min, *run_max;
  double *scale_out, *zp_out;
  int sym;
  float lo, hi;
  double qden, eps;
};

struct PGFixed {
  const double *scale, *zp;
  int zp_round;
  float lo, hi;
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

// ----------------------------------------------------------------------------
// observe + qparams + fake quant: every group as a K3 row holding its elements
// ----------------------------------------------------------------------------
template <bool VEC, int U, bool QUANT, bool CODES, bool MASK>
__global__ __launch_bounds__(kBlock) void k_pg_observe_fq(const float *__restrict__ x, float *__restrict__ y,
                                                          uint8_t *__restrict__ codes,
                                                          uint64_t *__restrict__ mask, PGView v, PGObs a) {
  PGTask k[U];
  f4 w[U];
  float rmn[U], rmx[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {   // all loads of the workgroup's tasks in flight before the first reduction
    k[u] = pg_task<U>(v, u);
    w[u] = load_group_c<VEC, VEC>(x + k[u].row * v.rowlen, k[u].i, k[u].ng, v.rowlen);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    rmn[u] = a.run_min[k[u].qi];
    rmx[u] = a.run_max[k[u].qi];
  }
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t seg = lane & ~(v.gl - 1);
  const uint64_t segmask = v.gl == 64 ? ~0ull : ((1ull << v.gl) - 1ull);
  PGOut go[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const f4 e = w[u];   // lanes past the row end replicate members of the row's last group
    float mn = fminf(fminf(e.x, e.y), fminf(e.z, e.w));
    float mx = fmaxf(fmaxf(e.x, e.y), fmaxf(e.z, e.w));
    const bool nanl = (e.x != e.x) | (e.y != e.y) | (e.z != e.z) | (e.w != e.w);
    mn = pg_reduce(mn, v.gl, MinOp());
    mx = pg_reduce(mx, v.gl, MaxOp());
    const bool nan = ((__ballot(nanl) >> seg) & segmask) != 0;
    float lo = rmn[u], hi = rmx[u];
    if (!nan) {   // minmax.py:44-47, strict compares; a NaN group changes nothing
      if (mn < lo) lo = mn;
      if (mx > hi) hi = mx;
    }
    double s, z;
    minmax_qparams((double)lo, (double)hi, a.sym, a.qden, a.eps, &s, &z);
    if (k[u].live && k[u].qvalid && lane == seg) {
      a.run_min[k[u].qi] = lo;
      a.run_max[k[u].qi] = hi;
      a.scale_out[k[u].qi] = s;
      a.zp_out[k[u].qi] = z;
    }
    if (QUANT) {
      const QP p = make_qp((float)s, (float)z, a.lo, a.hi, 0);
      go[u] = pg_quantize<VEC, CODES, MASK>(e, p, k[u], v);
    }
  }
  if (QUANT) {
#pragma unroll
    for (int u = 0; u < U; ++u) pg_store<VEC, CODES, MASK>(k[u], v, y, codes, mask, go[u]);
  }
}

// ----------------------------------------------------------------------------
// forward with given [rows, ngr] f64 qparams
// ----------------------------------------------------------------------------
template <bool VEC, int U, bool CODES, bool MASK>
__global__ __launch_bounds__(kBlock) void k_pg_fq_fwd(const float *__restrict__ x, float *__restrict__ y,
                                                      uint8_t *__restrict__ codes, uint64_t *__restrict__ mask,
                                                      PGView v, PGFixed a) {
  PGTask k[U];
  f4 w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = pg_task<U>(v, u);
    w[u] = load_group_c<VEC, VEC>(x + k[u].row * v.rowlen, k[u].i, k[u].ng, v.rowlen);
  }
  PGOut go[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const QPSrc s{nullptr, a.scale + k[u].qi, a.zp + k[u].qi, 0.0, 0.0, a.lo, a.hi, a.zp_round, 0};
    const QP p = load_qp(s);
    go[u] = pg_quantize<VEC, CODES, MASK>(w[u], p, k[u], v);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) pg_store<VEC, CODES, MASK>(k[u], v, y, codes, mask, go[u]);
}

// ----------------------------------------------------------------------------
// STE backward: gx = (mask ? g*s : 0) / s with s = fp32(scale[r, j])
// ----------------------------------------------------------------------------
template <bool VEC, int U>
__global__ __launch_bounds__(kBlock) void k_pg_ste_bwd(const float *__restrict__ g,
                                                       const uint64_t *__restrict__ mask,
                                                       float *__restrict__ gx, PGView v,
                                                       const double *__restrict__ scale) {
  PGTask k[U];
  f4 w[U];
  uint64_t m[U][4];
  double sc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = pg_task<U>(v, u);
    w[u] = load_group_c<VEC, VEC>(g + k[u].row * v.rowlen, k[u].i, k[u].ng, v.rowlen);
    const uint64_t *mr = mask + k[u].row * mask_words_per_row(v.rowlen) + 4 * (int64_t)k[u].chunk;   // wave-uniform
#pragma unroll
    for (int j = 0; j < 4; ++j) m[u][j] = mr[j];
    sc[u] = scale[k[u].qi];
  }
  const uint32_t lane = threadIdx.x % kWave;
  f4 o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const SteDiv d = make_stediv((float)sc[u]);
    const bool m0 = (m[u][0] >> lane) & 1u, m1 = (m[u][1] >> lane) & 1u, m2 = (m[u][2] >> lane) & 1u,
               m3 = (m[u][3] >> lane) & 1u;
    o[u].x = m0 ? ste_quot(w[u].x, d) : 0.0f;
    o[u].y = m1 ? ste_quot(w[u].y, d) : 0.0f;
    o[u].z = m2 ? ste_quot(w[u].z, d) : 0.0f;
    o[u].w = m3 ? ste_quot(w[u].w, d) : 0.0f;
    if (!(d.fast & ste_ok(w[u].x) & ste_ok(w[u].y) & ste_ok(w[u].z) & ste_ok(w[u].w))) {
      o[u].x = ste_ieee(w[u].x, m0, d);   // rare
      o[u].y = ste_ieee(w[u].y, m1, d);
      o[u].z = ste_ieee(w[u].z, m2, d);
      o[u].w = ste_ieee(w[u].w, m3, d);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (k[u].live && k[u].i < k[u].ng) store_group<VEC, VEC>(gx + k[u].row * v.rowlen, k[u].i, v.rowlen, o[u]);
}

// ----------------------------------------------------------------------------
// learnable (LSQ) backward: gx and the [rows, ngr] f64 scale / zero-point gradients
// ----------------------------------------------------------------------------
// Every 4-element group runs K4's element code (k_body.cuh lsq_group_out, act none) with its
// quantization group's qparams.  lsq_group_out adds +0 for an element past the row's end --
// a lane past it (its clamped loads are copies of the row's last elements) or the tail of a
// partial 4-element group on the scalar path -- so such elements leave both sums unchanged.
// Each lane's up to 4 terms are summed in f64, the group's gl lanes folded by pg_reduce, and
// the group's first lane writes sum * gscale: no LDS, no workspace, no atomics, one launch.
template <bool VEC, int U, bool ZPL>
__global__ __launch_bounds__(kBlock) void k_pg_lsq_bwd(const float *__restrict__ g, const float *__restrict__ x,
                                                       float *__restrict__ gx, PGView v, PGFixed a, double gscale,
                                                       double *__restrict__ gs_out, double *__restrict__ gz_out) {
  PGTask k[U];
  f4 xv[U], gv[U];
  double sc[U], zc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = pg_task<U>(v, u);
    xv[u] = load_group_c<VEC, VEC>(x + k[u].row * v.rowlen, k[u].i, k[u].ng, v.rowlen);
    gv[u] = load_group_c<VEC, VEC>(g + k[u].row * v.rowlen, k[u].i, k[u].ng, v.rowlen);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    sc[u] = a.scale[k[u].qi];
    zc[u] = a.zp[k[u].qi];
  }
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t seg = lane & ~(v.gl - 1);
  f4 o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const QPSrc s{nullptr, nullptr, nullptr, sc[u], zc[u], a.lo, a.hi, ZPL, 0};
    const QP p = load_qp(s);   // ZPL: the forward's clamp(rint(zp))
    LsqAcc c{0.0, 0.0};
    o[u] = lsq_group_out<ZPL, kActNone>(k[u].i, k[u].ng, v.rowlen, xv[u], gv[u], p, c);
    c.t = pg_reduce(c.t, v.gl, AddD());
    if (ZPL) c.z = pg_reduce(c.z, v.gl, AddD());
    if (k[u].live && k[u].qvalid && lane == seg) {
      gs_out[k[u].qi] = c.t * gscale;
      if (gz_out) gz_out[k[u].qi] = ZPL ? lsq_grad_zp(c.z, s, p, gscale) : 0.0;
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (k[u].live && k[u].i < k[u].ng) store_group<VEC, VEC>(gx + k[u].row * v.rowlen, k[u].i, v.rowlen, o[u]);
}

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
constexpr int kPgU = 4;  // tasks per wave where the grid still fills the device (else 1)

// rc 0 and the view, or an argument error (rows > 0 here)
static int pg_view(int64_t rows, int64_t rowlen, int64_t group, PGView *v) {
  const int64_t cpr = cdiv(rowlen, 4 * kWave);
  if (rows > 0x7fffffffLL || cpr > 0x7fffffffLL || rows * cpr > 0x7fffffffLL) return VSIQ_E_ARG;
  v->rowlen = rowlen;
  v->ngr = pg_groups_per_row(rowlen, group);
  v->tasks = (uint32_t)(rows * cpr);
  v->cpr = (uint32_t)cpr;
  v->gl = (uint32_t)(group / 4);
  return 0;
}

// tasks per wave, and the grid of workgroups of kWaves * U tasks
static int pg_per_wave(const PGView &v) {
  return (int64_t)v.tasks >= (int64_t)kWaves * kPgU * 4 * device_cus() ? kPgU : 1;
}
static dim3 pg_grid(const PGView &v, int u) { return dim3((unsigned)cdiv(v.tasks, (int64_t)kWaves * u), 1, 1); }

template <bool VEC, int U>
static void launch_pg_observe(const float *x, float *y, uint8_t *c, uint64_t *m, const PGView &v, const PGObs &a,
                              hipStream_t st) {
  const dim3 grid = pg_grid(v, U), block(kBlock);
  if (!y) hipLaunchKernelGGL((k_pg_observe_fq<VEC, U, false, false, false>), grid, block, 0, st, x, y, c, m, v, a);
  else if (c && m) hipLaunchKernelGGL((k_pg_observe_fq<VEC, U, true, true, true>), grid, block, 0, st, x, y, c, m, v, a);
  else if (c) hipLaunchKernelGGL((k_pg_observe_fq<VEC, U, true, true, false>), grid, block, 0, st, x, y, c, m, v, a);
  else if (m) hipLaunchKernelGGL((k_pg_observe_fq<VEC, U, true, false, true>), grid, block, 0, st, x, y, c, m, v, a);
  else hipLaunchKernelGGL((k_pg_observe_fq<VEC, U, true, false, false>), grid, block, 0, st, x, y, c, m, v, a);
}

template <bool VEC, int U>
static void launch_pg_fixed(const float *x, float *y, uint8_t *c, uint64_t *m, const PGView &v, const PGFixed &a,
                            hipStream_t st) {
  const dim3 grid = pg_grid(v, U), block(kBlock);
  if (c && m) hipLaunchKernelGGL((k_pg_fq_fwd<VEC, U, true, true>), grid, block, 0, st, x, y, c, m, v, a);
  else if (c) hipLaunchKernelGGL((k_pg_fq_fwd<VEC, U, true, false>), grid, block, 0, st, x, y, c, m, v, a);
  else if (m) hipLaunchKernelGGL((k_pg_fq_fwd<VEC, U, false, true>), grid, block, 0, st, x, y, c, m, v, a);
  else hipLaunchKernelGGL((k_pg_fq_fwd<VEC, U, false, false>), grid, block, 0, st, x, y, c, m, v, a);
}

template <bool VEC, int U>
static void launch_pg_lsq(const float *g, const float *x, float *gx, const PGView &v, const PGFixed &a, double gscale,
                          double *gs, double *gz, hipStream_t st) {
  const dim3 grid = pg_grid(v, U), block(kBlock);
  if (a.zp_round) hipLaunchKernelGGL((k_pg_lsq_bwd<VEC, U, true>), grid, block, 0, st, g, x, gx, v, a, gscale, gs, gz);
  else hipLaunchKernelGGL((k_pg_lsq_bwd<VEC, U, false>), grid, block, 0, st, g, x, gx, v, a, gscale, gs, gz);
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_pg_observe_fq_f32(const float *x, float *y, void *codes, uint64_t *mask, int64_t rows, int64_t rowlen,
                           int64_t group, float *run_min, float *run_max, double *scale_out, double *zp_out,
                           int symmetric, int qmin, int qmax, double qden, double eps, void *stream) {
  if (rows < 0 || rowlen <= 0 || qmin > qmax || !pg_group_ok(group)) return VSIQ_E_ARG;
  if (rows == 0) return 0;
  if (!x || !run_min || !run_max || !scale_out || !zp_out) return VSIQ_E_ARG;
  if (!y && (codes || mask)) return VSIQ_E_ARG;
  PGView v;
  if (pg_view(rows, rowlen, group, &v)) return VSIQ_E_ARG;
  if (mask && !aligned8(mask)) return VSIQ_E_ALIGN;
  const PGObs a{run_min, run_max, scale_out, zp_out, symmetric, (float)qmin, (float)qmax, qden, eps};
  const bool vec = (rowlen % 4 == 0) && aligned16(x) && (!y || aligned16(y)) && (!codes || aligned4(codes));
  hipStream_t st = (hipStream_t)stream;
  uint8_t *c = (uint8_t *)codes;
  if (!vec) launch_pg_observe<false, 1>(x, y, c, mask, v, a, st);
  else if (pg_per_wave(v) == kPgU) launch_pg_observe<true, kPgU>(x, y, c, mask, v, a, st);
  else launch_pg_observe<true, 1>(x, y, c, mask, v, a, st);
  return launch_rc();
}

int vsiq_pg_fq_fwd_f32(const float *x, float *y, void *codes, uint64_t *mask, int64_t rows, int64_t rowlen,
                       int64_t group, const double *scale, const double *zp, int zp_round, int qmin, int qmax,
                       void *stream) {
  if (rows < 0 || rowlen <= 0 || qmin > qmax || !pg_group_ok(group)) return VSIQ_E_ARG;
  if (rows == 0) return 0;
  if (!x || !y || !scale || !zp) return VSIQ_E_ARG;
  PGView v;
  if (pg_view(rows, rowlen, group, &v)) return VSIQ_E_ARG;
  if (mask && !aligned8(mask)) return VSIQ_E_ALIGN;
  const PGFixed a{scale, zp, zp_round, (float)qmin, (float)qmax};
  const bool vec = (rowlen % 4 == 0) && aligned16(x) && aligned16(y) && (!codes || aligned4(codes));
  hipStream_t st = (hipStream_t)stream;
  uint8_t *c = (uint8_t *)codes;
  if (!vec) launch_pg_fixed<false, 1>(x, y, c, mask, v, a, st);
  else if (pg_per_wave(v) == kPgU) launch_pg_fixed<true, kPgU>(x, y, c, mask, v, a, st);
  else launch_pg_fixed<true, 1>(x, y, c, mask, v, a, st);
  return launch_rc();
}

int vsiq_pg_ste_bwd_f32(const float *g, const uint64_t *mask, float *gx, int64_t rows, int64_t rowlen,
                        int64_t group, const double *scale, void *stream) {
  if (rows < 0 || rowlen <= 0 || !pg_group_ok(group)) return VSIQ_E_ARG;
  if (rows == 0) return 0;
  if (!g || !mask || !gx || !scale) return VSIQ_E_ARG;
  PGView v;
  if (pg_view(rows, rowlen, group, &v)) return VSIQ_E_ARG;
  if (!aligned8(mask)) return VSIQ_E_ALIGN;
  const bool vec = (rowlen % 4 == 0) && aligned16(g) && aligned16(gx);
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(kBlock);
  if (!vec) hipLaunchKernelGGL((k_pg_ste_bwd<false, 1>), pg_grid(v, 1), block, 0, st, g, mask, gx, v, scale);
  else if (pg_per_wave(v) == kPgU)
    hipLaunchKernelGGL((k_pg_ste_bwd<true, kPgU>), pg_grid(v, kPgU), block, 0, st, g, mask, gx, v, scale);
  else hipLaunchKernelGGL((k_pg_ste_bwd<true, 1>), pg_grid(v, 1), block, 0, st, g, mask, gx, v, scale);
  return launch_rc();
}

int vsiq_pg_lsq_bwd_f32(const float *g, const float *x, float *gx, int64_t rows, int64_t rowlen, int64_t group,
                        const double *scale, const double *zp, int zp_learn, int qmin, int qmax, double gscale,
                        double *grad_scale_out, double *grad_zp_out, void *stream) {
  if (rows < 0 || rowlen <= 0 || qmin > qmax || !pg_group_ok(group) || zp_learn < 0 || zp_learn > 1)
    return VSIQ_E_ARG;
  if (rows == 0) return 0;
  if (!g || !x || !gx || !scale || !zp || !grad_scale_out) return VSIQ_E_ARG;
  PGView v;
  if (pg_view(rows, rowlen, group, &v)) return VSIQ_E_ARG;
  const PGFixed a{scale, zp, zp_learn, (float)qmin, (float)qmax};
  const bool vec = (rowlen % 4 == 0) && aligned16(g) && aligned16(x) && aligned16(gx);
  hipStream_t st = (hipStream_t)stream;
  if (!vec) launch_pg_lsq<false, 1>(g, x, gx, v, a, gscale, grad_scale_out, grad_zp_out, st);
  else if (pg_per_wave(v) == kPgU) launch_pg_lsq<true, kPgU>(g, x, gx, v, a, gscale, grad_scale_out, grad_zp_out, st);
  else launch_pg_lsq<true, 1>(g, x, gx, v, a, gscale, grad_scale_out, grad_zp_out, st);
  return launch_rc();
}

}  // extern "C"
