// k_gptq.hip — GPTQ for group-wise weights (vsiq_pg_gptq_f32): error-compensated rounding of a
// [rows, rowlen] weight, one input column at a time, with the upper Cholesky factor U of the
// damped inverse Hessian.  include/vsiq.h states the arithmetic; every v[j] receives its updates
// as single fmaf's in ascending i, so the blocking below returns the bits of the unblocked loop.
//
// rowlen / 128 (rounded up) steps, each a BLOCK launch on the columns [b, b + 128) and, when
// columns remain, a TRAILING launch on the columns >= b + 128.  y is the working copy of v (the
// first two launches read w instead), the [rows, 128] strip `work` carries a block's errors e to
// its trailing launch.  Stream order is the only order between launches; no atomics, no waits.
//
// BLOCK kernel: one lane per row, one wave per workgroup, 64 rows per workgroup.  Nothing
// crosses lanes; a lane's arithmetic is the definition's loop on its row.
//   LDS   U's 128 x 128 diagonal block, row-major (64 KB), read as wave-wide broadcast 16-byte
//         reads; the tile's rows TRANSPOSED, s_v[column][lane] with the lane stride padded to 65
//         words, so a lane's walk along its row and the coalesced global accesses along a row
//         (lanes over columns) are both free of bank conflicts; the same for the errors (s_e)
//         and the packed code bytes (s_c).  137 KB of gfx950's 160 KB in all.
//   regs  the block runs as four sub-blocks of 32 columns in a rolled loop: a sub-block's 32
//         current values and its 32 errors live in registers with static indices (the 32 x 32
//         triangle is fully unrolled: 496 fmaf's and 32 quantizer calls), then the sub-block's
//         errors are pushed onto the block's remaining columns in LDS, 4 columns at a time (32
//         broadcast reads of U and 128 fmaf's per 4 columns).  Holding all 128 columns in
//         registers would unroll 8128 fmaf's and 128 quantizers into about 100 KB of straight-line
//         code that every wave runs exactly once, more than the instruction cache holds; the
//         rolled loop is 1/4 of the triangle plus a short loop, with the same LDS reads per fmaf
//         (one 16-byte broadcast read per 4).
//   A group's qparams are computed when its first column comes up, from the group's current
//   values in s_v: every update they will ever get has been applied by then.
//
// TRAILING kernel: grid of (64-row tiles) x (256-column tiles), lanes along the columns.  A lane
// keeps its column of the 128-row strip U[b .. b + 128, j] in 128 registers and reuses it over
// the tile's rows, four rows at a time (four independent fmaf chains); a row's 128 errors are
// wave-uniform and arrive as scalar loads from `work`, so the fmaf's take them from SGPRs.  (The
// compiler hoists the four rows' 512 scalar loads together and parks the overflow in VGPR lanes,
// v_writelane / v_readlane, not in scratch: DESIGN §8.)
//
// This file does not read the store-policy tuning knob: all loads and stores are plain ones.
#include "dispatch.cuh"
#include "k_gptq.cuh"
#include "k_pg.cuh"

namespace vsiq {

constexpr int kGptqRows = kWave;           // rows per block-kernel workgroup: one per lane
constexpr int kGptqLd = kGptqRows + 1;     // lane stride of the transposed tiles, in words
constexpr int kGptqSub = 32;               // columns held in registers at a time
constexpr int kGptqTrailRows = 64;         // rows per trailing-kernel workgroup
constexpr int kGptqTrailR = 4;             // rows in flight per lane

struct GptqArgs {
  int64_t rows, rowlen, ngr;
  int64_t b;     // the block's first column
  int bw;        // its width: min(128, rowlen - b), a multiple of the group
  int sym;
  float lo, hi;
  double qden, eps;
};

// the forwards' element function: the no-check fast path where it is proven equal, else IEEE
__device__ __forceinline__ Elem gptq_elem(float x, const QP &p) {
  return (p.fast & fq_x_ok(x)) ? fq_elem_fast(x, p) : fq_elem<true>(x, p);
}

template <int G, bool FIRST>
__global__ __launch_bounds__(kGptqRows) void k_gptq_block(const float *__restrict__ w, float *__restrict__ y,
                                                          const float *__restrict__ U, uint8_t *__restrict__ codes,
                                                          double *__restrict__ scale, double *__restrict__ zp,
                                                          float *__restrict__ work, GptqArgs a) {
  __shared__ f4 s_u[kGptqBlock * (kGptqBlock / 4)];
  __shared__ float s_v[kGptqBlock * kGptqLd];
  __shared__ float s_e[kGptqBlock * kGptqLd];
  __shared__ uint32_t s_c[(kGptqBlock / 4) * kGptqLd];
  const int lane = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * kGptqRows;
  const int nrow = (int)(a.rows - r0 < kGptqRows ? a.rows - r0 : kGptqRows);   // >= 1
  const float *src = FIRST ? w : y;

  // U's diagonal block: 16-byte loads, 32 per row of the block (b, bw and rowlen are multiples of 32)
  for (int t = lane; t < a.bw * (kGptqBlock / 4); t += kGptqRows) {
    const int i = t / (kGptqBlock / 4), c4 = t % (kGptqBlock / 4);
    if (4 * c4 < a.bw) s_u[t] = *reinterpret_cast<const f4 *>(U + (a.b + i) * a.rowlen + a.b + 4 * c4);
  }
  // the tile's rows, lanes along the row; rows past the tensor's end replicate its last row
  for (int rr = 0; rr < kGptqRows; ++rr) {
    const float *row = src + (r0 + (rr < nrow ? rr : nrow - 1)) * a.rowlen + a.b;
    for (int c = lane; c < a.bw; c += kGptqRows) s_v[c * kGptqLd + rr] = row[c];
  }
  __syncthreads();

  const int64_t qrow = (r0 + (lane < nrow ? lane : nrow - 1)) * a.ngr + a.b / G;
  QP p = make_qp(1.0f, 0.0f, a.lo, a.hi, 0);
  for (int c0 = 0; c0 < a.bw; c0 += kGptqSub) {
    if (c0 % G == 0) {   // a group starts: its qparams from its current values
      GptqRange g;
      for (int j = 0; j < G; ++j) gptq_range_add(g, s_v[(c0 + j) * kGptqLd + lane]);
      double s, z;
      gptq_group_qparams(g, a.sym, a.qden, a.eps, &s, &z);
      if (lane < nrow) {
        scale[qrow + c0 / G] = s;
        zp[qrow + c0 / G] = z;
      }
      p = make_qp((float)s, (float)z, a.lo, a.hi, 0);
    }
    float v[kGptqSub], e[kGptqSub];
    uint32_t cw[kGptqSub / 4];
#pragma unroll
    for (int k = 0; k < kGptqSub; ++k) v[k] = s_v[(c0 + k) * kGptqLd + lane];
#pragma unroll
    for (int k = 0; k < kGptqSub / 4; ++k) cw[k] = 0;
    const f4 *ud = s_u + c0 * (kGptqBlock / 4) + c0 / 4;   // U[c0 + i, c0 + 4 c ..] at ud[i * 32 + c]
#pragma unroll
    for (int i = 0; i < kGptqSub; ++i) {
      const Elem q = gptq_elem(v[i], p);
      const f4 ui = ud[i * (kGptqBlock / 4) + i / 4];
      const float d = i % 4 == 0 ? ui.x : i % 4 == 1 ? ui.y : i % 4 == 2 ? ui.z : ui.w;
      e[i] = (v[i] - q.y) / d;   // IEEE: this file is built with the correctly rounded division
      s_v[(c0 + i) * kGptqLd + lane] = q.y;
      s_e[(c0 + i) * kGptqLd + lane] = e[i];
      cw[i / 4] |= q.code << (8 * (i % 4));
      const float ne = -e[i];
#pragma unroll
      for (int c = i / 4; c < kGptqSub / 4; ++c) {
        const f4 u = c == i / 4 ? ui : ud[i * (kGptqBlock / 4) + c];
        if (4 * c + 0 > i) v[4 * c + 0] = __builtin_fmaf(ne, u.x, v[4 * c + 0]);
        if (4 * c + 1 > i) v[4 * c + 1] = __builtin_fmaf(ne, u.y, v[4 * c + 1]);
        if (4 * c + 2 > i) v[4 * c + 2] = __builtin_fmaf(ne, u.z, v[4 * c + 2]);
        if (4 * c + 3 > i) v[4 * c + 3] = __builtin_fmaf(ne, u.w, v[4 * c + 3]);
      }
    }
#pragma unroll
    for (int k = 0; k < kGptqSub / 4; ++k) s_c[(c0 / 4 + k) * kGptqLd + lane] = cw[k];
    // the sub-block's 32 errors onto the block's remaining columns, ascending i per column
    for (int j = c0 + kGptqSub; j < a.bw; j += 4) {
      float x0 = s_v[(j + 0) * kGptqLd + lane], x1 = s_v[(j + 1) * kGptqLd + lane];
      float x2 = s_v[(j + 2) * kGptqLd + lane], x3 = s_v[(j + 3) * kGptqLd + lane];
      const f4 *uj = s_u + c0 * (kGptqBlock / 4) + j / 4;
#pragma unroll
      for (int i = 0; i < kGptqSub; ++i) {
        const f4 u = uj[i * (kGptqBlock / 4)];
        const float ne = -e[i];
        x0 = __builtin_fmaf(ne, u.x, x0);
        x1 = __builtin_fmaf(ne, u.y, x1);
        x2 = __builtin_fmaf(ne, u.z, x2);
        x3 = __builtin_fmaf(ne, u.w, x3);
      }
      s_v[(j + 0) * kGptqLd + lane] = x0;
      s_v[(j + 1) * kGptqLd + lane] = x1;
      s_v[(j + 2) * kGptqLd + lane] = x2;
      s_v[(j + 3) * kGptqLd + lane] = x3;
    }
  }
  __syncthreads();

  // out through the transposed tiles: lanes along the row again
  for (int rr = 0; rr < nrow; ++rr) {
    float *yr = y + (r0 + rr) * a.rowlen + a.b;
    float *er = work + (r0 + rr) * kGptqBlock;
    for (int c = lane; c < a.bw; c += kGptqRows) {
      yr[c] = s_v[c * kGptqLd + rr];
      er[c] = s_e[c * kGptqLd + rr];
    }
    if (codes && 4 * lane < a.bw)
      reinterpret_cast<uint32_t *>(codes + (r0 + rr) * a.rowlen + a.b)[lane] = s_c[lane * kGptqLd + rr];
  }
}

// v[r, j] = fmaf(-e[r, i], U[b + i, j], v[r, j]) for i = 0 .. 127 in order, all j >= b + 128
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void k_gptq_trail(const float *__restrict__ w, float *__restrict__ y,
                                                       const float *__restrict__ U,
                                                       const float *__restrict__ work, int64_t rows,
                                                       int64_t rowlen, int64_t b) {
  const int64_t j0 = b + kGptqBlock + (int64_t)blockIdx.y * kBlock + threadIdx.x;
  const bool live = j0 < rowlen;
  const int64_t j = live ? j0 : rowlen - 1;   // a lane past the row's end computes its last column and stores nothing
  const float *src = FIRST ? w : y;
  float u[kGptqBlock];
#pragma unroll
  for (int i = 0; i < kGptqBlock; ++i) u[i] = U[(b + i) * rowlen + j];
  const int64_t r0 = (int64_t)blockIdx.x * kGptqTrailRows;
  const int64_t r1 = rows - r0 < kGptqTrailRows ? rows : r0 + kGptqTrailRows;
  for (int64_t r = r0; r < r1; r += kGptqTrailR) {
    float v[kGptqTrailR];
    const float *e[kGptqTrailR];
#pragma unroll
    for (int k = 0; k < kGptqTrailR; ++k) {
      const int64_t rr = r + k < r1 ? r + k : r1 - 1;   // past the tile: its last row again, not stored
      v[k] = src[rr * rowlen + j];
      e[k] = work + rr * kGptqBlock;
    }
#pragma unroll
    for (int i = 0; i < kGptqBlock; ++i) {
#pragma unroll
      for (int k = 0; k < kGptqTrailR; ++k) v[k] = __builtin_fmaf(-e[k][i], u[i], v[k]);
    }
#pragma unroll
    for (int k = 0; k < kGptqTrailR; ++k)
      if (live && r + k < r1) y[(r + k) * rowlen + j0] = v[k];
  }
}

template <int G, bool FIRST>
static void launch_gptq_block(const float *w, float *y, const float *U, uint8_t *codes, double *scale, double *zp,
                              float *work, const GptqArgs &a, hipStream_t st) {
  hipLaunchKernelGGL((k_gptq_block<G, FIRST>), dim3((unsigned)cdiv(a.rows, kGptqRows)), dim3(kGptqRows), 0, st, w, y,
                     U, codes, scale, zp, work, a);
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int64_t vsiq_pg_gptq_work_bytes(int64_t rows, int64_t rowlen) {
  if (rows <= 0 || rowlen <= 0 || rows > 0x7fffffffLL) return 0;
  return rows * kGptqBlock * (int64_t)sizeof(float);
}

int vsiq_pg_gptq_f32(const float *w, const float *U, float *y, void *codes, double *scale_out, double *zp_out,
                     void *work, int64_t rows, int64_t rowlen, int64_t group, int symmetric, int qmin, int qmax,
                     double qden, double eps, void *stream) {
  if (!gptq_sizes_ok(rows, rowlen, group) || qmin > qmax || !w || !U || !y || !scale_out || !zp_out || !work)
    return VSIQ_E_ARG;
  if (!aligned16(w) || !aligned16(U) || !aligned16(y) || !aligned16(work) || !aligned4(codes)) return VSIQ_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  GptqArgs a{rows, rowlen, rowlen / group, 0, 0, symmetric, (float)qmin, (float)qmax, qden, eps};
  for (int64_t b = 0; b < rowlen; b += kGptqBlock) {
    // y == w (in place): every launch then reads and writes the one working copy
    const bool first = b == 0 && w != y;
    a.b = b;
    a.bw = (int)std::min<int64_t>(kGptqBlock, rowlen - b);
    with_int<32, 64, 128>((int)group, [&](auto G) {
      if (first) launch_gptq_block<decltype(G)::value, true>(w, y, U, (uint8_t *)codes, scale_out, zp_out, (float *)work, a, st);
      else launch_gptq_block<decltype(G)::value, false>(w, y, U, (uint8_t *)codes, scale_out, zp_out, (float *)work, a, st);
    });
    const int64_t rest = rowlen - (b + kGptqBlock);
    if (rest <= 0) break;
    const dim3 grid((unsigned)cdiv(rows, kGptqTrailRows), (unsigned)cdiv(rest, kBlock));
    if (first) hipLaunchKernelGGL((k_gptq_trail<true>), grid, dim3(kBlock), 0, st, w, y, U, (const float *)work, rows, rowlen, b);
    else hipLaunchKernelGGL((k_gptq_trail<false>), grid, dim3(kBlock), 0, st, w, y, U, (const float *)work, rows, rowlen, b);
  }
  return launch_rc();
}

}  // extern "C"
