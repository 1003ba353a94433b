// k_pg_mse.hip — the per-group MSE observer (PerGroupMSEObserver, observers/per_group_mse.py):
// group (r, j) of the group-wise view (k_pg.cuh) is the per-channel search of k_pc_mse.hip on
// a row holding that group's elements alone -- its own min / max / NaN flag, `count` candidate
// ranges, every candidate's summed squared error, the strict-< pick, the running update of
// (run_min, run_max)[r, j], the f64 qparams and optionally the fake-quantized group -- in ONE
// launch and one read of the tensor, with no workspace, no counter and no workgroup barrier.
//
// Lane mapping: k_pg.hip's (k_pg_wave.cuh).  A wave owns one 256-element chunk of one row, a
// group is gl = G/4 = 8 / 16 / 32 / 64 adjacent lanes of it, and the four ballots of the fake
// quant are the chunk's mask words; lanes past the row end hold (clamped) copies of the row's
// last elements, add +0 to every error sum and store nothing.
//
// What is this kernel's own: up to 8 groups share a wave and each has its own candidates, so a
// candidate's parameters cannot sit in SGPRs for the whole wave (k_mse_step.cuh's mse_step).
//   * Candidates are built once per group, not once per lane: lane m of a group builds
//     candidates m, m + gl, ... of a pass of kPgMsePass and publishes (s, 1/s, z, flags) as one
//     16-byte entry of the group's slice of a wave-private LDS table (8 groups x 64 entries per
//     wave, 32.5 KB per workgroup; slices kPgMseStride entries apart so that the 8 groups'
//     broadcast reads fall into different banks).  Only the wave itself reads its slice: the
//     ordering is the wave's own (LDS executes a wave's accesses in order), no s_barrier.
//   * Candidates are scored kPgMseBatch = 8 at a time.  Every lane keeps 8 f64 partial sums
//     (its 4 elements against the batch's 8 candidates), and a transpose-reduce butterfly folds
//     them: at step i a lane swaps half of its partials with lane ^ (1 << i) and adds the half
//     it keeps (4 + 2 + 1 exchange-adds for 8 candidates instead of 8 x 3), after which lane l
//     holds candidate rev3(l & 7) summed over its 8 lanes.  Groups wider than 8 lanes then add
//     the lanes l ^ 8, l ^ 16, l ^ 32 -- inside the group only.  The owner keeps a running
//     (least error, smallest index); the pick is a min-with-index over the group's lanes.
//   * The fast element path (fq_elem_fast) is taken on a wave-uniform condition per pass --
//     every element of the wave fq_x_ok and every valid candidate of the pass fast -- else
//     the IEEE one (fq_elem<true>): the same y bit for bit, and no divergence per group.
// The order of a group's f64 sums is a function of (rowlen, group, count) only: lane sums of 4
// terms in element order, the butterfly, the octet adds.  No floating-point atomics.
//
// One store policy, k_pg.hip's: the vector path streams with nontemporal loads and stores, the
// scalar path (rowlen % 4 != 0 or unaligned pointers) uses plain per-element accesses.  This
// file does not read the tuning knob.
#include "k_mse_step.cuh"
#include "k_pg_wave.cuh"

namespace vsiq {

constexpr int kPgMseBatch = 8;     // candidates per butterfly
constexpr int kPgMsePass = 64;     // candidates published per pass (count <= 128: at most two passes)
constexpr int kPgMseGroups = 8;    // groups of one wave at G = 32
constexpr int kPgMseStride = kPgMsePass + 1;   // entries between two groups' slices (bank skew)

struct PgMseArgs {
  int count;
  float *run_min, *run_max;
  double *scale_out, *zp_out;
  double *clip_out;    // [rows, ngr, 2]
  double *err_out;     // [rows, ngr, count] (nullable)
  int32_t *pick_out;   // [rows, ngr]
  int sym;
  float lo, hi;
  double qden, eps;
};

struct MinU {
  static __device__ uint32_t identity() { return 0xffffffffu; }
  __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; }
};

// the wave's own LDS writes before its own LDS reads (and the reverse): the compiler keeps the
// order, the LDS queue is drained; no other wave touches the slice
__device__ __forceinline__ void pgm_lds_order() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// v of lane ^ 4 / lane ^ 16 (ds_swizzle bit mode: and 0x1f, or 0, xor X) and of lane ^ 32
template <int XOR>
__device__ __forceinline__ double pgm_swizzle(double v) {
  constexpr int kPattern = (XOR << 10) | 0x1f;
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)u, kPattern);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)(uint32_t)(u >> 32), kPattern);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ double pgm_xor32(double v) {
  const int addr = (int)(((threadIdx.x % kWave) ^ 32u) << 2);
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)u);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(u >> 32));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// the candidate of a batch that lane l ends up owning
__device__ __forceinline__ uint32_t pgm_own(uint32_t lane) {
  return ((lane & 1u) << 2) | (lane & 2u) | ((lane >> 2) & 1u);
}

// Transpose-reduce over the 8 lanes l & ~7 .. l | 7: p[c] is this lane's sum for candidate c of
// the batch; returns candidate pgm_own(l) summed over the 8 lanes.  Whole wave active.
__device__ __forceinline__ double pgm_fold8(const double (&p)[kPgMseBatch]) {
  const uint32_t lane = threadIdx.x % kWave;
  const bool b0 = (lane & 1u) != 0u, b1 = (lane & 2u) != 0u, b2 = (lane & 4u) != 0u;
  double q[4], r[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double keep = b0 ? p[4 + j] : p[j], send = b0 ? p[j] : p[4 + j];
    q[j] = keep + dpp<0xB1>(send, 0.0);   // quad_perm [1,0,3,2]: lane ^ 1
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double keep = b1 ? q[2 + j] : q[j], send = b1 ? q[j] : q[2 + j];
    r[j] = keep + dpp<0x4E>(send, 0.0);   // quad_perm [2,3,0,1]: lane ^ 2
  }
  const double keep = b2 ? r[1] : r[0], send = b2 ? r[0] : r[1];
  return keep + pgm_swizzle<4>(send);
}

// the same candidate's sums of the group's other octets (lanes l ^ 8, ^ 16, ^ 32: never a lane
// of another group), to every one of them
__device__ __forceinline__ double pgm_octets(double v, uint32_t gl) {
  if (gl >= 16) v = v + dpp<0x128>(v, 0.0);   // row_ror:8: lane ^ 8
  if (gl >= 32) v = v + pgm_swizzle<16>(v);
  if (gl == 64) v = v + pgm_xor32(v);
  return v;
}

// one batch: this lane's elements against the 8 published candidates sc[0..7] of its group
template <bool IEEE>
__device__ __forceinline__ double pgm_batch(const f4 *sc, const f4 (&ev)[1], uint32_t vm, float qlo, float qhi) {
  double p[kPgMseBatch];
#pragma unroll
  for (int j = 0; j < kPgMseBatch; ++j) {
    const f4 c = sc[j];
    QP q;
    q.s = c.x;
    q.z = c.z;
    q.lo = qlo;
    q.hi = qhi;
    q.discrete = 0;
    q.d.b = c.x;
    q.d.r = c.y;
    q.d.fast = q.fast = IEEE ? 0u : 1u;
    p[j] = mse_part<IEEE, true, 1>(ev, q, vm);
  }
  return pgm_fold8(p);
}

template <bool VEC, bool QUANT, bool CODES, bool MASK>
__global__ __launch_bounds__(kBlock) void k_pg_mse(const float *__restrict__ x, float *__restrict__ y,
                                                   uint8_t *__restrict__ codes, uint64_t *__restrict__ mask,
                                                   PGView v, MseRatios R, PgMseArgs a) {
  __shared__ f4 s_c[kWaves][kPgMseGroups * kPgMseStride];
  const PGTask k = pg_task<1>(v, 0);
  const f4 e = pg_load<VEC>(x, k, v);
  float st[2] = {a.run_min[k.qi], a.run_max[k.qi]};
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  const uint32_t seg = lane & ~(v.gl - 1), m = lane - seg;
  const uint64_t segmask = v.gl == 64 ? ~0ull : ((1ull << v.gl) - 1ull);
  const bool writer = k.live && k.qvalid;

  // the group's own min / max / NaN flag, as k_pc_mse.hip reduces a row (an all-NaN group: inf, -inf)
  const PGRange r = pg_range<true>(e, v, seg, segmask);
  const float mn = r.mn, mx = r.mx;
  const bool nan = r.nan, fb = mse_fallback(mn, mx, nan, a.count);   // the group's own

  int pick = 0;
  if (__ballot(!fb) != 0) {   // wave-uniform: some group of the wave searches
    // elements past the row end (a clamped lane, the tail of a partial 4-element group) add +0
    const int nv = k.i < k.ng ? (VEC ? 4 : valid_in_group(k.i, v.rowlen)) : 0;
    const uint32_t vm = (1u << nv) - 1u;
    const f4 ev[1] = {e};
    const uint32_t xok = fq_x_ok(e.x) & fq_x_ok(e.y) & fq_x_ok(e.z) & fq_x_ok(e.w);
    const bool xfast = __ballot(!xok) == 0;
    const uint32_t own = pgm_own(lane);
    f4 *sc = s_c[wave] + (lane / v.gl) * kPgMseStride;   // the group's slice
    double best = __builtin_inf();
    for (int c0 = 0; c0 < a.count; c0 += kPgMsePass) {
      const int np = a.count - c0 < kPgMsePass ? a.count - c0 : kPgMsePass;
      // publish: every entry of the pass is written; one past the count, of an invalid
      // candidate or of a group that fell back is invalid with harmless parameters
      uint32_t slow = 0u;
      for (uint32_t c = m; c < (uint32_t)kPgMsePass; c += v.gl) {   // kPgMsePass / gl trips in every lane
        f4 o;
        o.x = 1.0f; o.y = 1.0f; o.z = 0.0f; o.w = u2f(0u);
        if (!fb && (int)c < np) {
          const MseCand cd = mse_candidate(mn, mx, R.r[c0 + (int)c], a.sym, a.qden, a.eps);
          if (cd.valid) {
            const QP p = make_qp(cd.s, cd.z, a.lo, a.hi, 0);
            o.x = p.s; o.y = p.d.r; o.z = p.z;
            o.w = u2f(kMseValid | (p.fast ? kMseFast : 0u));
            slow |= p.fast ? 0u : 1u;
          }
        }
        sc[c] = o;
      }
      pgm_lds_order();
      const bool fast = xfast && __ballot(slow != 0u) == 0;   // wave-uniform
      for (int b = 0; b < np; b += kPgMseBatch) {
        double E = fast ? pgm_batch<false>(sc + b, ev, vm, a.lo, a.hi) : pgm_batch<true>(sc + b, ev, vm, a.lo, a.hi);
        E = pgm_octets(E, v.gl);
        const int kk = c0 + b + (int)own;
        if (!(f2u(sc[b + own].w) & kMseValid)) E = __builtin_inf();   // its error is +inf whatever the group holds
        if (a.err_out && writer && !fb && m < (uint32_t)kPgMseBatch && kk < a.count)
          a.err_out[k.qi * a.count + kk] = E;
        if (E < best) {   // this lane's candidates come in rising order: mse_pick's scan
          best = E;
          pick = kk;
        }
      }
      pgm_lds_order();
    }
    // min with index over the group's lanes, ties to the smaller k (all +inf: 0)
    const double least = pg_reduce(best, v.gl, MinD());
    pick = (int)pg_reduce(best == least ? (uint32_t)pick : 0xffffffffu, v.gl, MinU());
  }
  if (a.err_out && writer && fb)
    for (int kk = (int)m; kk < a.count; kk += (int)v.gl) a.err_out[k.qi * a.count + kk] = __builtin_inf();

  // the end of the group, as pc_mse_finish ends a row: computed by every lane, stored by the first
  float lo = mn, hi = mx;
  if (!fb) mse_range(mn, mx, R.r[pick], &lo, &hi);
  double qp[VSIQ_QP_LEN], clip[2];
  hist_finish(lo, hi, nan, st, qp, clip, a.sym, a.qden, a.eps);
  if (writer && lane == seg) {
    a.run_min[k.qi] = st[0];
    a.run_max[k.qi] = st[1];
    a.scale_out[k.qi] = qp[VSIQ_QP_SCALE];
    a.zp_out[k.qi] = qp[VSIQ_QP_ZP];
    a.clip_out[2 * k.qi] = clip[0];
    a.clip_out[2 * k.qi + 1] = clip[1];
    a.pick_out[k.qi] = pick;
  }
  if (QUANT) {
    const QP p = make_qp((float)qp[VSIQ_QP_SCALE], (float)qp[VSIQ_QP_ZP], a.lo, a.hi, 0);
    const PGOut go = pg_quantize<VEC, CODES, MASK>(e, p, k, v);
    pg_store<VEC, CODES, MASK>(k, v, y, codes, mask, go);
  }
}

template <bool VEC>
static void launch_pg_mse(const float *x, float *y, uint8_t *c, uint64_t *m, const PGView &v, const MseRatios &R,
                          const PgMseArgs &a, hipStream_t st) {
  const dim3 grid = pg_grid(v, 1), block(kBlock);
  if (!y) hipLaunchKernelGGL((k_pg_mse<VEC, false, false, false>), grid, block, 0, st, x, y, c, m, v, R, a);
  else if (c && m) hipLaunchKernelGGL((k_pg_mse<VEC, true, true, true>), grid, block, 0, st, x, y, c, m, v, R, a);
  else if (c) hipLaunchKernelGGL((k_pg_mse<VEC, true, true, false>), grid, block, 0, st, x, y, c, m, v, R, a);
  else if (m) hipLaunchKernelGGL((k_pg_mse<VEC, true, false, true>), grid, block, 0, st, x, y, c, m, v, R, a);
  else hipLaunchKernelGGL((k_pg_mse<VEC, true, false, false>), grid, block, 0, st, x, y, c, m, v, R, a);
}

}  // namespace vsiq

using namespace vsiq;

extern "C" {

int vsiq_pg_observe_mse_f32(const float *x, float *y, void *codes, uint64_t *mask, int64_t rows, int64_t rowlen,
                            int64_t group, const double *ratios, int count, float *run_min, float *run_max,
                            double *scale_out, double *zp_out, double *clip_out, double *err_out, int32_t *pick_out,
                            int symmetric, int qmin, int qmax, double qden, double eps, void *stream) {
  PGView v;
  int rc;
  if (!pg_enter(rows, rowlen, group, qmin < qmax && mse_ratios_ok(ratios, count),
                x && run_min && run_max && scale_out && zp_out && clip_out && pick_out && (y || (!codes && !mask)),
                mask, &v, &rc))
    return rc;
  MseRatios R{};
  for (int k = 0; k < count; ++k) R.r[k] = ratios[k];
  const PgMseArgs a{count,    run_min,   run_max,     scale_out,   zp_out, clip_out, err_out,
                    pick_out, symmetric, (float)qmin, (float)qmax, qden,   eps};
  const bool vec = (rowlen % 4 == 0) && aligned16(x) && (!y || aligned16(y)) && (!codes || aligned4(codes));
  with_bool(vec, [&](auto V) {
    launch_pg_mse<decltype(V)::value>(x, y, (uint8_t *)codes, mask, v, R, a, (hipStream_t)stream);
  });
  return launch_rc();
}

}  // extern "C"
