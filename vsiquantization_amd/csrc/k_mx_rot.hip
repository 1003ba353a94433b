// k_mx_rot.hip — Hadamard-rotated MX fake quantization: y = hadamard_32(MX(hadamard_32(x))) per
// scale block of 32 (vsiq_mx_rot_fq_fwd_f32, vsiq_mx_rot_fq_fwd_cols_f32) and its straight-through
// backward gx = hadamard_32(mask ? hadamard_32(g) : +0) (vsiq_mx_rot_ste_bwd_f32, _cols_f32), one
// launch and one read of the input each.  fp32 in and out; no workspace, LDS allocation, atomics
// or state between launches.  hadamard_32 is k_rot.cuh's transform at 8 lanes per group (row
// form) or the same stages over a register index (column form); MX is k_mx.cuh's element code
// unchanged.  include/vsiq.h states the definition and the composition of existing entries each
// call equals bit for bit.
//
// Block length = transform length, so a block's whole life -- transform, maximum, rounding,
// transform -- stays with the lanes (row form) or the registers (column form) that loaded it.
//
// Row form, x [rows, rowlen], rowlen % 32 == 0.  k_mx.hip's k_mx_rows32 mapping: the lanes follow
// the FLAT tensor, a wave owns 256-element chunk c, lane l elements 256c + 4l .. + 3, a block is
// 8 adjacent lanes, and the wave's four ballots are the per-tensor mask view's four words of the
// chunk.  Per chunk, all in registers:
//   rot_hadamard<8>      h = 1, 2 in the lane; h = 4, 8 as quad_perm DPP operands of the adds;
//                        h = 16 (lane ^ 4) through ds_swizzle; * c_32; NaN canonical
//   pg_reduce at 8       the block maximum of |r| bit patterns: three DPP steps
//   mx_scale, mx_quad    scale byte, the four elements, their codes and mask bits
//   rot_hadamard<8>      again, on the quantized values
// U chunks per wave, every load in flight before the first transform (U = 4 where the grid still
// fills the device, as k_mx_rows32).  n % 32 == 0, so lanes past the tensor's end sit in 8-lane
// groups of their own: they hold copies of the last group, transform among themselves and store
// nothing.  Pointers that are not 16-byte aligned take the same kernel with per-element loads
// and stores (VEC false, one chunk per wave): there is no LDS-staged form, a Hadamard block has
// no short form.
//
// Column form, x [outer, channels, inner], channels % 32 == 0, blocks along `channels` at stride
// `inner`.  k_mx.hip's k_mx_cols mapping: lanes along inner, a wave 256 consecutive inner
// positions of one (outer, channel block), every lane its four blocks' 32 channels as 32 x float4
// in registers.  The transform's five stages pair registers c and c + h: 5 x 64 adds and
// subtracts per lane and transform, no cross-lane step at all.  The second transform needs all 32
// quantized quads, so yr, the codes and each channel's mask ballots leave as the elements are
// quantized (in place, over the rotated values), before it.
//
// Backward, both mappings: load g, transform, keep where the mask bit is set and +0 elsewhere
// ((mask ? r * 1 : 0) / 1 is exactly that, the STE kernel with scale 1), transform, store.  The
// row form reads its chunk's four mask words with wave-uniform loads, the column form one mask
// row's four words per channel, as the forward wrote them.
//
// The vector paths stream with nontemporal loads and stores, the per-element paths use plain
// ones, as k_mx.hip and k_rot.hip; this file does not read the store-policy tuning knob.
#include "k_mx_wave.cuh"   // the element code (k_mx.cuh), mx_quad, mx_mask_word, MxCols
#include "k_pg_wave.cuh"   // pg_reduce
#include "k_rot.cuh"       // rot_hadamard, rot_sign

namespace vsiq {

constexpr int kMxrU = 4;   // row kernels: chunks per wave where the grid still fills the device

struct MxrOut {
  float *y, *yr;             // yr, codes, scales, mask: nullable (wave-uniform tests)
  uint8_t *codes, *scales;
  uint64_t *mask;
};

// ----------------------------------------------------------------------------
// rows: a block is 8 adjacent lanes
// ----------------------------------------------------------------------------
// chunk u of this wave (unclamped) and its lane's group of 4 in the flat tensor, clamped for the load
struct MxrChunk {
  uint32_t t;
  int64_t i, ic;
};

template <int U>
__device__ __forceinline__ MxrChunk mxr_chunk(int u, uint32_t chunks, int64_t ng) {
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  MxrChunk k;
  k.t = blockIdx.x * (uint32_t)(kWaves * U) + (uint32_t)u * kWaves + wave;   // < 2^31 + 4U
  k.i = (int64_t)k.t * kWave + lane;
  const int64_t c = (int64_t)(k.t < chunks ? k.t : chunks - 1) * kWave + lane;   // a chunk past the last repeats it,
  k.ic = c < ng ? c : ng - 1;                                                     // a lane past the end the last group
  return k;
}

template <bool VEC, int U, bool CODES>
__global__ __launch_bounds__(kBlock) void k_mxr_rows(const float *__restrict__ x, MxrOut out, int64_t n,
                                                     uint32_t chunks, MxFmt f) {
  const uint32_t lane = threadIdx.x % kWave;
  const int64_t ng = n / 4;   // a multiple of 8
  MxrChunk k[U];
  f4 v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = mxr_chunk<U>(u, chunks, ng);
    v[u] = load_group<VEC, VEC>(x, k[u].ic, n);
  }
  const RotSign g = rot_sign();
  MxQuad q[U];
  f4 o[U];
  uint64_t mw[U];
  uint32_t sc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const f4 r = rot_hadamard<8>(v[u], g);
    const MxMaxBits mx;
    // padding lanes are whole 8-lane groups (ng % 8 == 0): no block sees their copies
    const uint32_t am = pg_reduce(mx(mx(mx_abs_bits(r.x), mx_abs_bits(r.y)), mx(mx_abs_bits(r.z), mx_abs_bits(r.w))),
                                  8u, mx);
    const MxScale s = mx_scale(am, f);
    sc[u] = s.code;
    q[u] = mx_quad<CODES>(r, s, s, s, s, f);
    mw[u] = out.mask ? mx_mask_word(q[u].m, k[u].t < chunks && k[u].i < ng ? 4 : 0) : 0;
    // the transform exchanges lanes: mx_elem's block-uniform branch has rejoined before it
    o[u] = rot_hadamard<8>(q[u].y, g);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (k[u].t >= chunks) continue;   // wave-uniform
    const int64_t i = k[u].i;
    if (i < ng) {
      store_group<VEC, VEC>(out.y, i, n, o[u]);
      if (out.yr) store_group<VEC, VEC>(out.yr, i, n, q[u].y);
      if (CODES) {
        if (VEC) reinterpret_cast<uint32_t *>(out.codes)[i] = q[u].c;
        else
          for (int j = 0; j < 4; ++j) out.codes[4 * i + j] = (uint8_t)(q[u].c >> (8 * j));
      }
      if (out.scales && lane % 8 == 0) out.scales[i / 8] = (uint8_t)sc[u];   // block (r, b) at r * rowlen / 32 + b
    }
    if (out.mask && lane < 4) out.mask[4 * (int64_t)k[u].t + lane] = mw[u];
  }
}

template <bool VEC, int U>
__global__ __launch_bounds__(kBlock) void k_mxr_rows_bwd(const float *__restrict__ gy,
                                                         const uint64_t *__restrict__ mask, float *__restrict__ gx,
                                                         int64_t n, uint32_t chunks) {
  const uint32_t lane = threadIdx.x % kWave;
  const int64_t ng = n / 4;
  MxrChunk k[U];
  f4 v[U];
  uint64_t m[U][4];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    k[u] = mxr_chunk<U>(u, chunks, ng);
    v[u] = load_group<VEC, VEC>(gy, k[u].ic, n);
    const uint64_t *mr = mask + 4 * (int64_t)(k[u].t < chunks ? k[u].t : chunks - 1);   // wave-uniform
#pragma unroll
    for (int j = 0; j < 4; ++j) m[u][j] = mr[j];
  }
  const RotSign g = rot_sign();
  f4 o[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const f4 r = rot_hadamard<8>(v[u], g);
    f4 e;
    e.x = (m[u][0] >> lane) & 1u ? r.x : 0.0f;
    e.y = (m[u][1] >> lane) & 1u ? r.y : 0.0f;
    e.z = (m[u][2] >> lane) & 1u ? r.z : 0.0f;
    e.w = (m[u][3] >> lane) & 1u ? r.w : 0.0f;
    o[u] = rot_hadamard<8>(e, g);
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (k[u].t < chunks && k[u].i < ng) store_group<VEC, VEC>(gx, k[u].i, n, o[u]);
}

// ----------------------------------------------------------------------------
// columns: lanes along inner, a lane's four blocks are the four components of its 32 registers
// ----------------------------------------------------------------------------
// hadamard_32 over the register index, on four blocks at once
__device__ __forceinline__ void mxr_hadamard_regs(f4 (&v)[32]) {
#pragma unroll
  for (int h = 1; h < 32; h *= 2) {
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      if (c & h) continue;
      const f4 a = v[c], b = v[c + h];
      v[c].x = a.x + b.x; v[c].y = a.y + b.y; v[c].z = a.z + b.z; v[c].w = a.w + b.w;
      v[c + h].x = a.x - b.x; v[c + h].y = a.y - b.y; v[c + h].z = a.z - b.z; v[c + h].w = a.w - b.w;
    }
  }
  constexpr float cg = RotC<8>::c;
  bool nan = false;
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    v[c].x *= cg; v[c].y *= cg; v[c].z *= cg; v[c].w *= cg;
    nan |= __builtin_isunordered(v[c].x, v[c].y) | __builtin_isunordered(v[c].z, v[c].w);
  }
  if (__ballot(nan)) {   // rot_hadamard's rule: a NaN result is the canonical quiet NaN
    const float qnan = __uint_as_float(0x7FC00000u);
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      v[c].x = v[c].x != v[c].x ? qnan : v[c].x;
      v[c].y = v[c].y != v[c].y ? qnan : v[c].y;
      v[c].z = v[c].z != v[c].z ? qnan : v[c].z;
      v[c].w = v[c].w != v[c].w ? qnan : v[c].w;
    }
  }
}

// where a wave works: (outer o, channel block b, inner chunk q) of task t, clamped into the grid
struct MxrColTask {
  int64_t row0, i, ng;   // first (outer, channel) row, this lane's group of 4 in the row, groups per row
  uint32_t q, ob;        // chunk of inner, o * cb + b
  int nv;                // elements of the lane's group that exist (0: a dead task or a lane past the row)
  bool live;
};

template <bool VEC>
__device__ __forceinline__ MxrColTask mxr_col_task(const MxCols &a) {
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const uint32_t t = blockIdx.x * (uint32_t)kWaves + wave;
  MxrColTask k;
  k.live = t < a.tasks;   // wave-uniform
  const uint32_t tc = k.live ? t : a.tasks - 1;
  k.q = tc % a.cpr;
  k.ob = tc / a.cpr;
  k.row0 = (int64_t)(k.ob / a.cb) * a.channels + 32 * (int64_t)(k.ob % a.cb);
  k.ng = cdiv(a.inner, 4);
  k.i = (int64_t)k.q * kWave + lane;
  k.nv = k.live ? (VEC ? (k.i < k.ng ? 4 : 0) : valid_in_group(k.i, a.inner)) : 0;
  return k;
}

template <bool VEC>
__device__ __forceinline__ void mxr_col_load(const float *__restrict__ x, const MxrColTask &k, const MxCols &a,
                                             f4 (&v)[32]) {
#pragma unroll
  for (int c = 0; c < 32; ++c)   // a lane past the row loads its last group: blocks of its own, never stored
    v[c] = load_group_c<VEC, VEC>(x + (k.row0 + c) * a.inner, k.i, k.ng, a.inner);
}

template <bool VEC, bool CODES>
__global__ __launch_bounds__(kBlock) void k_mxr_cols(const float *__restrict__ x, MxrOut out, MxCols a, MxFmt f) {
  const uint32_t lane = threadIdx.x % kWave;
  const MxrColTask k = mxr_col_task<VEC>(a);
  f4 v[32];
  mxr_col_load<VEC>(x, k, a, v);
  mxr_hadamard_regs(v);
  uint32_t am[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    am[0] = std::max(am[0], mx_abs_bits(v[c].x));
    am[1] = std::max(am[1], mx_abs_bits(v[c].y));
    am[2] = std::max(am[2], mx_abs_bits(v[c].z));
    am[3] = std::max(am[3], mx_abs_bits(v[c].w));
  }
  const MxScale s0 = mx_scale(am[0], f), s1 = mx_scale(am[1], f), s2 = mx_scale(am[2], f), s3 = mx_scale(am[3], f);
  if (out.scales && k.nv) {   // [outer][cb][inner]
    uint8_t *sp = out.scales + (int64_t)k.ob * a.inner + 4 * k.i;
    const uint32_t pk = s0.code | (s1.code << 8) | (s2.code << 16) | (s3.code << 24);
    if (VEC) *reinterpret_cast<uint32_t *>(sp) = pk;
    else
      for (int j = 0; j < k.nv; ++j) sp[j] = (uint8_t)(pk >> (8 * j));
  }
  const int64_t wpr = mask_words_per_row(a.inner);
#pragma unroll
  for (int c = 0; c < 32; ++c) {   // the rotated domain's outputs leave here; v keeps the quantized values
    const MxQuad r = mx_quad<CODES>(v[c], s0, s1, s2, s3, f);
    v[c] = r.y;
    const int64_t row = k.row0 + c;
    if (out.mask) {   // kernel-uniform
      const uint64_t mw = mx_mask_word(r.m, k.nv);
      if (k.live && lane < 4) out.mask[row * wpr + 4 * (int64_t)k.q + lane] = mw;
    }
    if (k.nv) {
      if (out.yr) store_group<VEC, VEC>(out.yr + row * a.inner, k.i, a.inner, r.y);
      if (CODES) {
        uint8_t *cr = out.codes + row * a.inner;
        if (VEC) reinterpret_cast<uint32_t *>(cr)[k.i] = r.c;
        else
          for (int j = 0; j < k.nv; ++j) cr[4 * k.i + j] = (uint8_t)(r.c >> (8 * j));
      }
    }
  }
  mxr_hadamard_regs(v);
  if (k.nv) {
#pragma unroll
    for (int c = 0; c < 32; ++c) store_group<VEC, VEC>(out.y + (k.row0 + c) * a.inner, k.i, a.inner, v[c]);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_mxr_cols_bwd(const float *__restrict__ gy,
                                                         const uint64_t *__restrict__ mask, float *__restrict__ gx,
                                                         MxCols a) {
  const uint32_t lane = threadIdx.x % kWave;
  const MxrColTask k = mxr_col_task<VEC>(a);
  f4 v[32];
  mxr_col_load<VEC>(gy, k, a, v);
  mxr_hadamard_regs(v);
  const uint64_t *mr = mask + k.row0 * mask_words_per_row(a.inner) + 4 * (int64_t)k.q;   // wave-uniform
  const int64_t wpr = mask_words_per_row(a.inner);
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    const uint64_t m0 = mr[c * wpr], m1 = mr[c * wpr + 1], m2 = mr[c * wpr + 2], m3 = mr[c * wpr + 3];
    v[c].x = (m0 >> lane) & 1u ? v[c].x : 0.0f;
    v[c].y = (m1 >> lane) & 1u ? v[c].y : 0.0f;
    v[c].z = (m2 >> lane) & 1u ? v[c].z : 0.0f;
    v[c].w = (m3 >> lane) & 1u ? v[c].w : 0.0f;
  }
  mxr_hadamard_regs(v);
  if (k.nv) {
#pragma unroll
    for (int c = 0; c < 32; ++c) store_group<VEC, VEC>(gx + (k.row0 + c) * a.inner, k.i, a.inner, v[c]);
  }
}

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
// what the row entries open with: argument errors, then the mask's alignment; *chunks on success
static int mxr_enter_rows(int64_t rows, int64_t rowlen, bool ok, const void *mask, int64_t *n, int64_t *chunks) {
  if (rows <= 0 || rowlen <= 0 || rowlen % 32 != 0 || !ok || rows > 0x7fffffffffffffffLL / rowlen) return VSIQ_E_ARG;
  *n = rows * rowlen;
  *chunks = cdiv(*n, 256);
  if (*chunks > 0x7fffffffLL) return VSIQ_E_ARG;
  return aligned8(mask) ? 0 : VSIQ_E_ALIGN;
}

static int mxr_enter_cols(int64_t outer, int64_t channels, int64_t inner, bool ok, const void *mask, MxCols *a) {
  if (outer <= 0 || channels <= 0 || inner <= 0 || channels % 32 != 0 || !ok) return VSIQ_E_ARG;
  if (channels > 0x7fffffffffffffffLL / outer || outer * channels > 0x7fffffffffffffffLL / inner) return VSIQ_E_ARG;
  const int64_t cb = channels / 32, cpr = cdiv(inner, 256);
  if (outer > 0x7fffffffLL || cb > 0x7fffffffLL / outer || cpr > 0x7fffffffLL / (outer * cb)) return VSIQ_E_ARG;
  *a = MxCols{channels, inner, (uint32_t)cb, (uint32_t)cpr, (uint32_t)(outer * cb * cpr)};
  return aligned8(mask) ? 0 : VSIQ_E_ALIGN;
}

// f(VEC, U) over the row kernels' three launch forms: per-element, vector with 1 chunk per wave,
// vector with kMxrU
template <class F>
static void with_mxr_form(bool vec, int64_t chunks, F &&f) {
  if (!vec) f(BoolC<false>{}, IntC<1>{});
  else if (chunks >= (int64_t)kWaves * kMxrU * 4 * device_cus()) f(BoolC<true>{}, IntC<kMxrU>{});
  else f(BoolC<true>{}, IntC<1>{});
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_mx_rot_fq_fwd_f32(const float *x, float *y, float *yr, uint8_t *codes, uint8_t *scales, uint64_t *mask,
                           int64_t rows, int64_t rowlen, int fmt, void *stream) {
  int64_t n, chunks;
  if (const int rc = mxr_enter_rows(rows, rowlen, mx_fmt_ok(fmt) && x && y, mask, &n, &chunks)) return rc;
  const MxFmt f = mx_fmt(fmt);
  const MxrOut out{y, yr, codes, scales, mask};
  const bool vec = aligned16(x) && aligned16(y) && (!yr || aligned16(yr)) && (!codes || aligned4(codes));
  with_mxr_form(vec, chunks, [&](auto V, auto U) {
    with_bool(codes != nullptr, [&](auto C) {
      constexpr int UU = decltype(U)::value;
      hipLaunchKernelGGL((k_mxr_rows<decltype(V)::value, UU, decltype(C)::value>),
                         dim3((unsigned)cdiv(chunks, kWaves * UU)), dim3(kBlock), 0, (hipStream_t)stream, x, out, n,
                         (uint32_t)chunks, f);
    });
  });
  return launch_rc();
}

int vsiq_mx_rot_fq_fwd_cols_f32(const float *x, float *y, float *yr, uint8_t *codes, uint8_t *scales, uint64_t *mask,
                                int64_t outer, int64_t channels, int64_t inner, int fmt, void *stream) {
  MxCols a;
  if (const int rc = mxr_enter_cols(outer, channels, inner, mx_fmt_ok(fmt) && x && y, mask, &a)) return rc;
  const MxFmt f = mx_fmt(fmt);
  const MxrOut out{y, yr, codes, scales, mask};
  const bool vec = inner % 4 == 0 && aligned16(x) && aligned16(y) && (!yr || aligned16(yr)) &&
                   (!codes || aligned4(codes)) && (!scales || aligned4(scales));
  with_bool2(vec, codes != nullptr, [&](auto V, auto C) {
    hipLaunchKernelGGL((k_mxr_cols<decltype(V)::value, decltype(C)::value>), dim3((unsigned)cdiv(a.tasks, kWaves)),
                       dim3(kBlock), 0, (hipStream_t)stream, x, out, a, f);
  });
  return launch_rc();
}

int vsiq_mx_rot_ste_bwd_f32(const float *g, const uint64_t *mask, float *gx, int64_t rows, int64_t rowlen,
                            void *stream) {
  int64_t n, chunks;
  if (const int rc = mxr_enter_rows(rows, rowlen, g && mask && gx, mask, &n, &chunks)) return rc;
  with_mxr_form(aligned16(g) && aligned16(gx), chunks, [&](auto V, auto U) {
    constexpr int UU = decltype(U)::value;
    hipLaunchKernelGGL((k_mxr_rows_bwd<decltype(V)::value, UU>), dim3((unsigned)cdiv(chunks, kWaves * UU)),
                       dim3(kBlock), 0, (hipStream_t)stream, g, mask, gx, n, (uint32_t)chunks);
  });
  return launch_rc();
}

int vsiq_mx_rot_ste_bwd_cols_f32(const float *g, const uint64_t *mask, float *gx, int64_t outer, int64_t channels,
                                 int64_t inner, void *stream) {
  MxCols a;
  if (const int rc = mxr_enter_cols(outer, channels, inner, g && mask && gx, mask, &a)) return rc;
  with_bool(inner % 4 == 0 && aligned16(g) && aligned16(gx), [&](auto V) {
    hipLaunchKernelGGL((k_mxr_cols_bwd<decltype(V)::value>), dim3((unsigned)cdiv(a.tasks, kWaves)), dim3(kBlock), 0,
                       (hipStream_t)stream, g, mask, gx, a);
  });
  return launch_rc();
}

}  // extern "C"
