// k_mx.hip — MX block-scaled fake quantization (MXFP4 / MXFP6 / MXFP8) on the device: the row
// form (vsiq_mx_fq_fwd_f32) and the column form (vsiq_mx_fq_fwd_cols_f32) of the host loops in
// k_host.hip, on k_mx.cuh's element code unchanged.  fp32 in and out; one launch and one read
// of x per call; no workspace, counter, atomics or state between launches.  include/vsiq.h
// states the arithmetic and both mask views.
//
// Row form, x [rows, rowlen], blocks of 32 along each row.  The lanes follow the FLAT tensor, not
// its rows: lane l of the wave on 256-element chunk c owns elements 256c + 4l .. 256c + 4l + 3 of
// the n = rows * rowlen elements, the mapping of the 1-bit mask's per-tensor view (one row of n),
// so the wave's four ballots ARE the chunk's four mask words, every word up to the tensor's last
// chunk is written whole by exactly one wave, and short rows fill a wave between them (a
// [64, 27] conv weight is 7 waves, not 64).
//   k_mx_rows32   rowlen % 32 == 0, 16-byte aligned: every block is 8 adjacent lanes of one
//                 wave (rows start on block boundaries, chunks too).  The block maximum -- of
//                 |v| bit patterns, as on the host, so NaN / Inf blocks need no test of their
//                 own -- is three DPP steps (k_pg_wave.cuh pg_reduce at 8 lanes): no LDS, no
//                 barrier.  U chunks per wave, all loads in flight before the first reduction.
//   k_mx_rows_any any other row length or alignment.  Blocks then start anywhere in a wave
//                 and cross waves and workgroups, so a workgroup stages the |v| patterns of its
//                 1024 elements in LDS with up to 32 elements either side (the only elements
//                 read by two workgroups: the blocks its edges cut), and every lane takes its
//                 block's maximum from there.  VEC (rowlen % 4 == 0, aligned): 16-byte loads
//                 and stores, a lane's 4 elements share a block; else per-element accesses and
//                 a block lookup per element.
//
// Column form, x [outer, channels, inner], blocks of 32 along `channels` at stride `inner`.
// Lanes run along `inner`: a wave takes 256 consecutive inner positions (4 per lane) of one
// (outer, channel block) and each lane walks its <= 32 channels, holding them in registers
// (32 x 4 fp32) between the maximum and the rounding: one global read, no LDS, no cross-lane
// step.  Every lane owns 4 blocks (one per inner position).  Its mask view is (outer * channels,
// inner): for channel row r the wave's ballots are the four words of chunk q of that row, so
// again every word is written whole by one wave.
//
// The vector paths stream with nontemporal loads and stores, the per-element paths use plain
// ones, as k_pg.hip; this file does not read the tuning knob.
#include "k_mx_wave.cuh"   // the element code (k_mx.cuh), mx_quad, mx_mask_word, MxCols
#include "k_pg_wave.cuh"   // pg_reduce

namespace vsiq {

constexpr int kMxSpan = 4 * kBlock;   // elements of a k_mx_rows_any workgroup
constexpr int kMxU = 4;               // k_mx_rows32: chunks per wave where the grid still fills the device

// ----------------------------------------------------------------------------
// rows, rowlen % 32 == 0: a block is 8 adjacent lanes
// ----------------------------------------------------------------------------
template <int U, bool CODES, bool MASK>
__global__ __launch_bounds__(kBlock) void k_mx_rows32(const float *__restrict__ x, float *__restrict__ y,
                                                      uint8_t *__restrict__ codes, uint8_t *__restrict__ scales,
                                                      uint64_t *__restrict__ mask, int64_t n, uint32_t chunks,
                                                      MxFmt f) {
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const int64_t ng = n / 4;   // a multiple of 8
  uint32_t t[U];
  f4 v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {   // a chunk past the last repeats it, a lane past the end its last group
    t[u] = blockIdx.x * (uint32_t)(kWaves * U) + (uint32_t)u * kWaves + wave;   // < 2^31 + 4U
    const int64_t i = (int64_t)(t[u] < chunks ? t[u] : chunks - 1) * kWave + lane;
    v[u] = ld4<true>(x + 4 * (i < ng ? i : ng - 1));
  }
  MxQuad q[U];
  uint64_t mw[U];
  uint32_t sc[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t a0 = mx_abs_bits(v[u].x), a1 = mx_abs_bits(v[u].y), a2 = mx_abs_bits(v[u].z),
                   a3 = mx_abs_bits(v[u].w);
    const MxMaxBits mx;
    // lanes past the end sit in 8-lane groups of their own (ng % 8 == 0): no block sees their copies
    const uint32_t am = pg_reduce(mx(mx(a0, a1), mx(a2, a3)), 8u, mx);
    const MxScale s = mx_scale(am, f);
    sc[u] = s.code;
    q[u] = mx_quad<CODES>(v[u], s, s, s, s, f);
    const int64_t i = (int64_t)t[u] * kWave + lane;
    mw[u] = MASK ? mx_mask_word(q[u].m, t[u] < chunks && i < ng ? 4 : 0) : 0;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (t[u] >= chunks) continue;   // wave-uniform
    const int64_t i = (int64_t)t[u] * kWave + lane;
    if (i < ng) {
      st4<true>(y + 4 * i, q[u].y);
      if (CODES) reinterpret_cast<uint32_t *>(codes)[i] = q[u].c;
      if (scales && lane % 8 == 0) scales[i / 8] = (uint8_t)sc[u];   // block (r, k) at r * rowlen / 32 + k = e / 32
    }
    if (MASK && lane < 4) mask[4 * (int64_t)t[u] + lane] = mw[u];
  }
}

// ----------------------------------------------------------------------------
// rows, any row length and alignment: block maxima from the workgroup's span in LDS
// ----------------------------------------------------------------------------
template <bool VEC, bool CODES, bool MASK>
__global__ __launch_bounds__(kBlock) void k_mx_rows_any(const float *__restrict__ x, float *__restrict__ y,
                                                        uint8_t *__restrict__ codes, uint8_t *__restrict__ scales,
                                                        uint64_t *__restrict__ mask, int64_t n, int64_t rowlen,
                                                        MxFmt f) {
  __shared__ uint32_t sm[32 + kMxSpan + 32];   // |v| patterns of elements wb - 32 .. wb + kMxSpan + 31
  const int64_t wb = (int64_t)blockIdx.x * kMxSpan, ng = cdiv(n, 4), nb = mx_row_blocks(rowlen);
  const int64_t i = wb / 4 + threadIdx.x;
  const f4 v = load_group_c<VEC, VEC>(x, i, ng, n);   // the flat tensor as one row of n
  const float xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) sm[32 + 4 * threadIdx.x + j] = mx_abs_bits(xv[j]);
  if (threadIdx.x < 64) {   // the halo either side (clamped into the tensor; a slot outside it is never read)
    const int64_t e = threadIdx.x < 32 ? wb - 32 + threadIdx.x : wb + kMxSpan + (threadIdx.x - 32);
    sm[threadIdx.x < 32 ? threadIdx.x : kMxSpan + threadIdx.x] = mx_abs_bits(x[e < 0 ? 0 : e < n ? e : n - 1]);
  }
  __syncthreads();
  const int64_t e0 = 4 * i, ec = e0 < n ? e0 : n - 1;
  int64_t row = ec / rowlen, col = ec - row * rowlen, have = -1;
  MxScale s = mx_scale(0u, f);
  MxQuad q;
  float yv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  q.c = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t e = e0 + j;
    q.m[j] = false;
    if (e < n) {
      const int64_t c0 = col & ~(int64_t)31, bs = e - (col - c0);   // the block's first element: >= wb - 31
      if (bs != have) {   // VEC: once per lane
        const int64_t be = std::min(bs + 32, e - col + rowlen);     // <= wb + kMxSpan + 32, <= n
        uint32_t am = 0u;
        for (int64_t k = bs; k < be; ++k) am = std::max(am, sm[k - wb + 32]);
        s = mx_scale(am, f);
        have = bs;
        if (scales && col == c0) scales[row * nb + (col >> 5)] = (uint8_t)s.code;   // its first element's lane
      }
      const MxElem o = mx_elem<CODES>(xv[j], s, f);
      yv[j] = o.y;
      q.c |= o.code << (8 * j);
      q.m[j] = o.m;
      if (++col == rowlen) {
        col = 0;
        ++row;
      }
    }
  }
  q.y.x = yv[0]; q.y.y = yv[1]; q.y.z = yv[2]; q.y.w = yv[3];
  const int nv = valid_in_group(i, n);
  const uint64_t mw = MASK ? mx_mask_word(q.m, nv) : 0;
  if (i < ng) {
    store_group<VEC, VEC>(y, i, n, q.y);
    if (CODES) {
      if (VEC) reinterpret_cast<uint32_t *>(codes)[i] = q.c;
      else
        for (int j = 0; j < nv; ++j) codes[e0 + j] = (uint8_t)(q.c >> (8 * j));
    }
  }
  const int64_t chunk = wb / 256 + threadIdx.x / kWave;
  if (MASK && threadIdx.x % kWave < 4 && chunk < cdiv(n, 256)) mask[4 * chunk + threadIdx.x % kWave] = mw;
}

// ----------------------------------------------------------------------------
// columns: lanes along inner, every lane its 4 blocks' <= 32 channels in registers
// ----------------------------------------------------------------------------
template <bool VEC, bool CODES, bool MASK>
__global__ __launch_bounds__(kBlock) void k_mx_cols(const float *__restrict__ x, float *__restrict__ y,
                                                    uint8_t *__restrict__ codes, uint8_t *__restrict__ scales,
                                                    uint64_t *__restrict__ mask, MxCols a, MxFmt f) {
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const uint32_t t = blockIdx.x * (uint32_t)kWaves + wave;
  const bool live = t < a.tasks;   // wave-uniform
  const uint32_t tc = live ? t : a.tasks - 1;
  const uint32_t q = tc % a.cpr, ok = tc / a.cpr, k = ok % a.cb, o = ok / a.cb;
  const int64_t left = a.channels - 32 * (int64_t)k;
  const int cnt = left < 32 ? (int)left : 32;
  const int64_t ng = cdiv(a.inner, 4), i = (int64_t)q * kWave + lane;
  const int64_t row0 = (int64_t)o * a.channels + 32 * (int64_t)k;
  const int nv = live ? (VEC ? (i < ng ? 4 : 0) : valid_in_group(i, a.inner)) : 0;
  f4 v[32];
#pragma unroll
  for (int c = 0; c < 32; ++c)   // a channel past the block repeats its last one, a lane past the row its last group
    v[c] = load_group_c<VEC, VEC>(x + (row0 + (c < cnt ? c : cnt - 1)) * a.inner, i, ng, a.inner);
  uint32_t am[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    am[0] = std::max(am[0], mx_abs_bits(v[c].x));
    am[1] = std::max(am[1], mx_abs_bits(v[c].y));
    am[2] = std::max(am[2], mx_abs_bits(v[c].z));
    am[3] = std::max(am[3], mx_abs_bits(v[c].w));
  }
  const MxScale s0 = mx_scale(am[0], f), s1 = mx_scale(am[1], f), s2 = mx_scale(am[2], f), s3 = mx_scale(am[3], f);
  if (scales && nv) {   // [outer][cb][inner]
    uint8_t *sp = scales + ((int64_t)o * a.cb + k) * a.inner + 4 * i;
    const uint32_t pk = s0.code | (s1.code << 8) | (s2.code << 16) | (s3.code << 24);
    if (VEC) *reinterpret_cast<uint32_t *>(sp) = pk;
    else
      for (int j = 0; j < nv; ++j) sp[j] = (uint8_t)(pk >> (8 * j));
  }
  const int64_t wpr = mask_words_per_row(a.inner);
#pragma unroll
  for (int c = 0; c < 32; ++c) {
    if (c >= cnt) continue;   // wave-uniform
    const MxQuad r = mx_quad<CODES>(v[c], s0, s1, s2, s3, f);
    const uint64_t mw = MASK ? mx_mask_word(r.m, nv) : 0;
    const int64_t row = row0 + c;
    if (nv) {
      store_group<VEC, VEC>(y + row * a.inner, i, a.inner, r.y);
      if (CODES) {
        uint8_t *cr = codes + row * a.inner;
        if (VEC) reinterpret_cast<uint32_t *>(cr)[i] = r.c;
        else
          for (int j = 0; j < nv; ++j) cr[4 * i + j] = (uint8_t)(r.c >> (8 * j));
      }
    }
    if (MASK && live && lane < 4) mask[row * wpr + 4 * (int64_t)q + lane] = mw;
  }
}

// host: the checks both entries share, in the host entries' order, then the mask's alignment
static int mx_enter(bool sizes_ok, int fmt, const void *x, const void *y, const void *mask) {
  if (!sizes_ok || !mx_fmt_ok(fmt) || !x || !y) return VSIQ_E_ARG;
  return aligned8(mask) ? 0 : VSIQ_E_ALIGN;
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_mx_fq_fwd_f32(const float *x, float *y, uint8_t *codes, uint8_t *scales, uint64_t *mask, int64_t rows,
                       int64_t rowlen, int fmt, void *stream) {
  if (const int rc = mx_enter(rows > 0 && rowlen > 0, fmt, x, y, mask)) return rc;
  if (rows > 0x7fffffffffffffffLL / rowlen) return VSIQ_E_ARG;
  const int64_t n = rows * rowlen, chunks = cdiv(n, 256);
  if (chunks > 0x7fffffffLL) return VSIQ_E_ARG;
  const MxFmt f = mx_fmt(fmt);
  const hipStream_t st = (hipStream_t)stream;
  const bool al = aligned16(x) && aligned16(y) && (!codes || aligned4(codes));
  with_bool2(codes != nullptr, mask != nullptr, [&](auto C, auto M) {
    constexpr bool kC = decltype(C)::value, kM = decltype(M)::value;
    if (al && rowlen % 32 == 0) {
      if (chunks >= (int64_t)kWaves * kMxU * 4 * device_cus())
        hipLaunchKernelGGL((k_mx_rows32<kMxU, kC, kM>), dim3((unsigned)cdiv(chunks, kWaves * kMxU)), dim3(kBlock), 0,
                           st, x, y, codes, scales, mask, n, (uint32_t)chunks, f);
      else
        hipLaunchKernelGGL((k_mx_rows32<1, kC, kM>), dim3((unsigned)cdiv(chunks, kWaves)), dim3(kBlock), 0, st, x, y,
                           codes, scales, mask, n, (uint32_t)chunks, f);
    } else {
      with_bool(al && rowlen % 4 == 0, [&](auto V) {
        hipLaunchKernelGGL((k_mx_rows_any<decltype(V)::value, kC, kM>), dim3((unsigned)cdiv(n, kMxSpan)), dim3(kBlock),
                           0, st, x, y, codes, scales, mask, n, rowlen, f);
      });
    }
  });
  return launch_rc();
}

int vsiq_mx_fq_fwd_cols_f32(const float *x, float *y, uint8_t *codes, uint8_t *scales, uint64_t *mask, int64_t outer,
                            int64_t channels, int64_t inner, int fmt, void *stream) {
  if (const int rc = mx_enter(outer > 0 && channels > 0 && inner > 0, fmt, x, y, mask)) return rc;
  if (channels > 0x7fffffffffffffffLL / outer || outer * channels > 0x7fffffffffffffffLL / inner) return VSIQ_E_ARG;
  const int64_t cb = cdiv(channels, 32), cpr = cdiv(inner, 256);
  if (outer > 0x7fffffffLL || cb > 0x7fffffffLL / outer || cpr > 0x7fffffffLL / (outer * cb)) return VSIQ_E_ARG;
  const MxCols a{channels, inner, (uint32_t)cb, (uint32_t)cpr, (uint32_t)(outer * cb * cpr)};
  const MxFmt f = mx_fmt(fmt);
  const bool vec = inner % 4 == 0 && aligned16(x) && aligned16(y) && (!codes || aligned4(codes)) &&
                   (!scales || aligned4(scales));
  with_bool2(codes != nullptr, mask != nullptr, [&](auto C, auto M) {
    with_bool(vec, [&](auto V) {
      hipLaunchKernelGGL((k_mx_cols<decltype(V)::value, decltype(C)::value, decltype(M)::value>),
                         dim3((unsigned)cdiv(a.tasks, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, x, y, codes,
                         scales, mask, a, f);
    });
  });
  return launch_rc();
}

}  // extern "C"
