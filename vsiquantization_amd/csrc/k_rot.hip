// k_rot.hip — Hadamard-rotated group-wise weight quantization: the group transform alone
// (vsiq_pg_hadamard_f32) and, in one launch each, transform -> observe + qparams + fake quant
// -> transform (vsiq_pg_rot_observe_fq_f32), the same with given [rows, ngr] qparams
// (vsiq_pg_rot_fq_fwd_f32) and transform -> STE backward -> transform (vsiq_pg_rot_ste_bwd_f32).
// include/vsiq.h states hadamard_G and what each entry equals bit for bit.
//
// Lane mapping: k_pg.hip's (k_pg_wave.cuh).  A wave owns one 256-element chunk of a row, a lane
// 4 consecutive elements, a group of G = 32 / 64 / 128 / 256 elements is GL = G / 4 = 8 / 16 /
// 32 / 64 adjacent lanes.  rowlen % G == 0 here, so a group lies wholly inside the row or is
// wholly padding: padding lanes hold copies of the row's last elements, transform them among
// themselves and store nothing.
//
// The transform stays in registers; no LDS is allocated and no step reads a lane of another
// group.  Stage h of the definition pairs elements i and i + h:
//
//   h = 1, 2        the lane's own four values: 8 adds.
//   h = 4, 8, 32    lane ^ 1, ^ 2, ^ 8.  The partner arrives as the DPP operand of the add
//                   itself (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_ror:8), so the
//                   exchange costs no instruction.  The lane with the stage's bit set needs
//                   partner - own: it flips the sign bit of its own value first (one v_xor with
//                   a per-lane constant) and adds.  partner + (-own) and partner - own are the
//                   same IEEE operation; fp32 addition commutes.  2 VALU per element.
//   h = 16          lane ^ 4.  gfx950 has no DPP control for it (row_half_mirror is ^ 7, the row
//                   shifts cross the 8-lane group), so the partner comes through ds_swizzle in
//                   bit mode (and 0x1f, xor 4): the LDS crossbar without an LDS allocation,
//                   issued beside the VALU.  1 DS + 2 VALU per element.
//   h = 64, 128     lane ^ 16, ^ 32.  v_permlane16_swap / v_permlane32_swap exchange the odd
//                   rows (upper half) of one register with the even rows (lower half) of
//                   another.  Fed two of the lane's elements (a, b), one swap leaves A = (a of
//                   the lower lanes, b of the lower lanes) and B = (a of the upper, b of the
//                   upper) side by side: A + B and A - B are then both elements' sums in one
//                   register and both differences in the other, each with own + partner in the
//                   lower and partner - own in the upper lane's operand order, and a second
//                   swap returns them to their lanes.  2 VALU per element, no sign flip, no DS;
//                   ds_bpermute would cost an address register and a DS round trip instead.
//   * c_G           4 multiplies; then a NaN becomes the canonical quiet NaN (2 compares and a
//                   wave-uniform branch; include/vsiq.h says why).
//
// GL is a template parameter: the stages a group does not have are not compiled, and the
// fused kernels' two transforms are straight-line code around the quantizer.
//
// One store policy, as k_pg.hip: the vector path (16-byte aligned tensors; rowlen % 4 == 0
// always holds here) streams with nontemporal loads and stores through pg_load /
// pg_store_row, the scalar path (unaligned pointers) uses plain ones.  This file does not
// read the store-policy tuning knob.
#include "k_pg_wave.cuh"
#include "k_rot.cuh"   // rot_hadamard, rot_sign and the stage helpers (shared with k_mx_rot.hip)

namespace vsiq {

// ----------------------------------------------------------------------------
// the transform alone (y == x allowed: every lane loads its elements before any store of its
// wave's task, and no task reads another's)
// ----------------------------------------------------------------------------
template <bool VEC, int U, int GL>
__global__ __launch_bounds__(kBlock) void k_rot_hadamard(const float *x, float *y, PGView v) {
  PGTask k[U];
  f4 w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = pg_task<U>(v, u);
    w[u] = pg_load<VEC>(x, k[u], v);
  }
  const RotSign g = rot_sign();
#pragma unroll
  for (int u = 0; u < U; ++u) w[u] = rot_hadamard<GL>(w[u], g);
#pragma unroll
  for (int u = 0; u < U; ++u) pg_store_row<VEC>(k[u], v, y, w[u]);
}

// ----------------------------------------------------------------------------
// the fused forwards.  yr / codes / mask are nullable at run time (wave-uniform tests): the
// quantizer always forms the code bytes and the mask words, which cost a handful of scalar
// instructions beside two transforms, and the kernels do not multiply by eight output arms.
// ----------------------------------------------------------------------------
struct RotObs {
  float *run_min, *run_max;
  double *scale_out, *zp_out;
  int sym;
  float lo, hi;
  double qden, eps;
};

struct RotFixed {
  const double *scale, *zp;
  int zp_round;
  float lo, hi;
};

struct RotOutPtrs {
  float *y, *yr;
  uint8_t *codes;
  uint64_t *mask;
};

// one task's stores: y = the second transform's result, yr / codes / mask from the quantizer
template <bool VEC>
__device__ __forceinline__ void rot_store(const PGTask &k, const PGView &v, const RotOutPtrs &p, const f4 &o,
                                          const PGOut &q) {
  pg_store_row<VEC>(k, v, p.y, o);
  if (p.yr) pg_store_row<VEC>(k, v, p.yr, q.o);
  if (!k.live) return;
  if (p.codes && k.i < k.ng) {
    uint8_t *cr = p.codes + k.row * v.rowlen;
    if (VEC) reinterpret_cast<uint32_t *>(cr)[k.i] = q.c;
    else
      for (int j = 0; j < 4; ++j) cr[4 * k.i + j] = (uint8_t)(q.c >> (8 * j));   // rowlen % 4 == 0
  }
  if (p.mask && threadIdx.x % kWave < 4)
    p.mask[k.row * mask_words_per_row(v.rowlen) + 4 * (int64_t)k.chunk + threadIdx.x % kWave] = q.mw;
}

template <bool VEC, int U, int GL, bool QUANT>
__global__ __launch_bounds__(kBlock) void k_rot_observe_fq(const float *__restrict__ x, RotOutPtrs out, PGView v,
                                                           RotObs a) {
  PGTask k[U];
  f4 w[U];
  float rmn[U], rmx[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = pg_task<U>(v, u);
    w[u] = pg_load<VEC>(x, k[u], v);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    rmn[u] = a.run_min[k[u].qi];
    rmx[u] = a.run_max[k[u].qi];
  }
  const RotSign g = rot_sign();
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t seg = lane & ~(uint32_t)(GL - 1);
  const uint64_t segmask = ~0ull >> (64 - GL);
  PGOut q[U];
  f4 o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const f4 r = rot_hadamard<GL>(w[u], g);
    const PGRange m = pg_range<false>(r, v, seg, segmask);
    float lo = rmn[u], hi = rmx[u];
    if (!m.nan) {   // k_pg_observe_fq's update on the rotated group
      if (m.mn < lo) lo = m.mn;
      if (m.mx > hi) hi = m.mx;
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
      q[u] = pg_quantize<VEC, true, true>(r, p, k[u], v);
      o[u] = rot_hadamard<GL>(q[u].o, g);
    }
  }
  if (QUANT) {
#pragma unroll
    for (int u = 0; u < U; ++u) rot_store<VEC>(k[u], v, out, o[u], q[u]);
  }
}

template <bool VEC, int U, int GL>
__global__ __launch_bounds__(kBlock) void k_rot_fq_fwd(const float *__restrict__ x, RotOutPtrs out, PGView v,
                                                       RotFixed a) {
  PGTask k[U];
  f4 w[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = pg_task<U>(v, u);
    w[u] = pg_load<VEC>(x, k[u], v);
  }
  const RotSign g = rot_sign();
  PGOut q[U];
  f4 o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const QPSrc s{nullptr, a.scale + k[u].qi, a.zp + k[u].qi, 0.0, 0.0, a.lo, a.hi, a.zp_round, 0};
    const QP p = load_qp(s);
    q[u] = pg_quantize<VEC, true, true>(rot_hadamard<GL>(w[u], g), p, k[u], v);
    o[u] = rot_hadamard<GL>(q[u].o, g);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) rot_store<VEC>(k[u], v, out, o[u], q[u]);
}

// ----------------------------------------------------------------------------
// backward: gx = hadamard(ste(hadamard(g))), ste being k_pg_ste_bwd's element arithmetic
// ----------------------------------------------------------------------------
template <bool VEC, int U, int GL>
__global__ __launch_bounds__(kBlock) void k_rot_ste_bwd(const float *__restrict__ gy,
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
    w[u] = pg_load<VEC>(gy, k[u], v);
    const uint64_t *mr = mask + k[u].row * mask_words_per_row(v.rowlen) + 4 * (int64_t)k[u].chunk;   // wave-uniform
#pragma unroll
    for (int j = 0; j < 4; ++j) m[u][j] = mr[j];
    sc[u] = scale[k[u].qi];
  }
  const RotSign g = rot_sign();
  const uint32_t lane = threadIdx.x % kWave;
  f4 o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const f4 r = rot_hadamard<GL>(w[u], g);
    const SteDiv d = make_stediv((float)sc[u]);
    const bool m0 = (m[u][0] >> lane) & 1u, m1 = (m[u][1] >> lane) & 1u, m2 = (m[u][2] >> lane) & 1u,
               m3 = (m[u][3] >> lane) & 1u;
    f4 e;
    e.x = m0 ? ste_quot(r.x, d) : 0.0f;
    e.y = m1 ? ste_quot(r.y, d) : 0.0f;
    e.z = m2 ? ste_quot(r.z, d) : 0.0f;
    e.w = m3 ? ste_quot(r.w, d) : 0.0f;
    if (!(d.fast & ste_ok(r.x) & ste_ok(r.y) & ste_ok(r.z) & ste_ok(r.w))) {
      e.x = ste_ieee(r.x, m0, d);   // rare
      e.y = ste_ieee(r.y, m1, d);
      e.z = ste_ieee(r.z, m2, d);
      e.w = ste_ieee(r.w, m3, d);
    }
    // the transform exchanges lanes: back to a converged wave before it
    o[u] = rot_hadamard<GL>(e, g);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) pg_store_row<VEC>(k[u], v, gx, o[u]);
}

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
// what every entry of this file opens with: pg_enter plus rowlen % group == 0
static bool rot_enter(int64_t rows, int64_t rowlen, int64_t group, bool args_ok, bool ptrs_ok, const void *mask,
                      PGView *v, int *rc) {
  const bool div = pg_group_ok(group) && rowlen > 0 && rowlen % group == 0;
  return pg_enter(rows, rowlen, group, args_ok && div, ptrs_ok, mask, v, rc);
}

// f(VEC, U, GL) over the launch forms of with_pg_form and the four group widths
template <class F>
static void with_rot_form(bool vec, const PGView &v, F &&f) {
  with_pg_form(vec, v, [&](auto V, auto U) {
    with_int<8, 16, 32, 64>((int)v.gl, [&](auto GL) { f(V, U, GL); });
  });
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_pg_hadamard_f32(const float *x, float *y, int64_t rows, int64_t rowlen, int64_t group, void *stream) {
  PGView v;
  int rc;
  if (!rot_enter(rows, rowlen, group, true, x && y, nullptr, &v, &rc)) return rc;
  with_rot_form(aligned16(x) && aligned16(y), v, [&](auto V, auto U, auto GL) {
    hipLaunchKernelGGL((k_rot_hadamard<decltype(V)::value, decltype(U)::value, decltype(GL)::value>),
                       pg_grid(v, decltype(U)::value), dim3(kBlock), 0, (hipStream_t)stream, x, y, v);
  });
  return launch_rc();
}

int vsiq_pg_rot_observe_fq_f32(const float *x, float *y, float *yr, void *codes, uint64_t *mask, int64_t rows,
                               int64_t rowlen, int64_t group, float *run_min, float *run_max, double *scale_out,
                               double *zp_out, int symmetric, int qmin, int qmax, double qden, double eps,
                               void *stream) {
  PGView v;
  int rc;
  if (!rot_enter(rows, rowlen, group, qmin <= qmax,
                 x && run_min && run_max && scale_out && zp_out && (y || (!yr && !codes && !mask)), mask, &v, &rc))
    return rc;
  const RotObs a{run_min, run_max, scale_out, zp_out, symmetric, (float)qmin, (float)qmax, qden, eps};
  const RotOutPtrs out{y, yr, (uint8_t *)codes, mask};
  const bool vec = aligned16(x) && (!y || aligned16(y)) && (!yr || aligned16(yr)) && (!codes || aligned4(codes));
  with_rot_form(vec, v, [&](auto V, auto U, auto GL) {
    constexpr bool VE = decltype(V)::value;
    constexpr int UU = decltype(U)::value, G = decltype(GL)::value;
    const dim3 grid = pg_grid(v, UU), block(kBlock);
    if (y) hipLaunchKernelGGL((k_rot_observe_fq<VE, UU, G, true>), grid, block, 0, (hipStream_t)stream, x, out, v, a);
    else hipLaunchKernelGGL((k_rot_observe_fq<VE, UU, G, false>), grid, block, 0, (hipStream_t)stream, x, out, v, a);
  });
  return launch_rc();
}

int vsiq_pg_rot_fq_fwd_f32(const float *x, float *y, float *yr, void *codes, uint64_t *mask, int64_t rows,
                           int64_t rowlen, int64_t group, const double *scale, const double *zp, int zp_round,
                           int qmin, int qmax, void *stream) {
  PGView v;
  int rc;
  if (!rot_enter(rows, rowlen, group, qmin <= qmax, x && y && scale && zp, mask, &v, &rc)) return rc;
  const RotFixed a{scale, zp, zp_round, (float)qmin, (float)qmax};
  const RotOutPtrs out{y, yr, (uint8_t *)codes, mask};
  const bool vec = aligned16(x) && aligned16(y) && (!yr || aligned16(yr)) && (!codes || aligned4(codes));
  with_rot_form(vec, v, [&](auto V, auto U, auto GL) {
    hipLaunchKernelGGL((k_rot_fq_fwd<decltype(V)::value, decltype(U)::value, decltype(GL)::value>),
                       pg_grid(v, decltype(U)::value), dim3(kBlock), 0, (hipStream_t)stream, x, out, v, a);
  });
  return launch_rc();
}

int vsiq_pg_rot_ste_bwd_f32(const float *g, const uint64_t *mask, float *gx, int64_t rows, int64_t rowlen,
                            int64_t group, const double *scale, void *stream) {
  PGView v;
  int rc;
  if (!rot_enter(rows, rowlen, group, true, g && mask && gx && scale, mask, &v, &rc)) return rc;
  with_rot_form(aligned16(g) && aligned16(gx), v, [&](auto V, auto U, auto GL) {
    hipLaunchKernelGGL((k_rot_ste_bwd<decltype(V)::value, decltype(U)::value, decltype(GL)::value>),
                       pg_grid(v, decltype(U)::value), dim3(kBlock), 0, (hipStream_t)stream, g, mask, gx, v, scale);
  });
  return launch_rc();
}

}  // extern "C"
