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
#include "k_pg_wave.cuh"   // the lane mapping's code, the entry checks and the launch forms

namespace vsiq {

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
    w[u] = pg_load<VEC>(x, k[u], v);
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
    const PGRange r = pg_range<false>(w[u], v, seg, segmask);
    float lo = rmn[u], hi = rmx[u];
    if (!r.nan) {   // minmax.py:44-47, strict compares; a NaN group changes nothing (r.mn, r.mx unread)
      if (r.mn < lo) lo = r.mn;
      if (r.mx > hi) hi = r.mx;
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
      go[u] = pg_quantize<VEC, CODES, MASK>(w[u], p, k[u], v);
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
    w[u] = pg_load<VEC>(x, k[u], v);
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
    w[u] = pg_load<VEC>(g, k[u], v);
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
  for (int u = 0; u < U; ++u) pg_store_row<VEC>(k[u], v, gx, o[u]);
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
    xv[u] = pg_load<VEC>(x, k[u], v);
    gv[u] = pg_load<VEC>(g, k[u], v);
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
  for (int u = 0; u < U; ++u) pg_store_row<VEC>(k[u], v, gx, o[u]);
}

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
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
  PGView v;
  int rc;
  if (!pg_enter(rows, rowlen, group, qmin <= qmax,
                x && run_min && run_max && scale_out && zp_out && (y || (!codes && !mask)), mask, &v, &rc))
    return rc;
  const PGObs a{run_min, run_max, scale_out, zp_out, symmetric, (float)qmin, (float)qmax, qden, eps};
  const bool vec = (rowlen % 4 == 0) && aligned16(x) && (!y || aligned16(y)) && (!codes || aligned4(codes));
  with_pg_form(vec, v, [&](auto V, auto U) {
    launch_pg_observe<decltype(V)::value, decltype(U)::value>(x, y, (uint8_t *)codes, mask, v, a, (hipStream_t)stream);
  });
  return launch_rc();
}

int vsiq_pg_fq_fwd_f32(const float *x, float *y, void *codes, uint64_t *mask, int64_t rows, int64_t rowlen,
                       int64_t group, const double *scale, const double *zp, int zp_round, int qmin, int qmax,
                       void *stream) {
  PGView v;
  int rc;
  if (!pg_enter(rows, rowlen, group, qmin <= qmax, x && y && scale && zp, mask, &v, &rc)) return rc;
  const PGFixed a{scale, zp, zp_round, (float)qmin, (float)qmax};
  const bool vec = (rowlen % 4 == 0) && aligned16(x) && aligned16(y) && (!codes || aligned4(codes));
  with_pg_form(vec, v, [&](auto V, auto U) {
    launch_pg_fixed<decltype(V)::value, decltype(U)::value>(x, y, (uint8_t *)codes, mask, v, a, (hipStream_t)stream);
  });
  return launch_rc();
}

int vsiq_pg_ste_bwd_f32(const float *g, const uint64_t *mask, float *gx, int64_t rows, int64_t rowlen,
                        int64_t group, const double *scale, void *stream) {
  PGView v;
  int rc;
  if (!pg_enter(rows, rowlen, group, true, g && mask && gx && scale, mask, &v, &rc)) return rc;
  const bool vec = (rowlen % 4 == 0) && aligned16(g) && aligned16(gx);
  with_pg_form(vec, v, [&](auto V, auto U) {
    hipLaunchKernelGGL((k_pg_ste_bwd<decltype(V)::value, decltype(U)::value>), pg_grid(v, decltype(U)::value),
                       dim3(kBlock), 0, (hipStream_t)stream, g, mask, gx, v, scale);
  });
  return launch_rc();
}

int vsiq_pg_lsq_bwd_f32(const float *g, const float *x, float *gx, int64_t rows, int64_t rowlen, int64_t group,
                        const double *scale, const double *zp, int zp_learn, int qmin, int qmax, double gscale,
                        double *grad_scale_out, double *grad_zp_out, void *stream) {
  PGView v;
  int rc;
  if (!pg_enter(rows, rowlen, group, qmin <= qmax && zp_learn >= 0 && zp_learn <= 1,
                g && x && gx && scale && zp && grad_scale_out, nullptr, &v, &rc))   // no mask
    return rc;
  const PGFixed a{scale, zp, zp_learn, (float)qmin, (float)qmax};
  const bool vec = (rowlen % 4 == 0) && aligned16(g) && aligned16(x) && aligned16(gx);
  with_pg_form(vec, v, [&](auto V, auto U) {
    launch_pg_lsq<decltype(V)::value, decltype(U)::value>(g, x, gx, v, a, gscale, grad_scale_out, grad_zp_out,
                                                          (hipStream_t)stream);
  });
  return launch_rc();
}

}  // extern "C"
