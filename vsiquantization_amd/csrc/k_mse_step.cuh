// k_mse_step.cuh -- the MSE search's wave step, shared by the per-tensor pass
// (k_observe_mse.hip) and the per-channel kernel (k_pc_mse.hip): U groups of 4 per lane held
// in registers scored against every candidate in turn.  Device only; the arithmetic of one
// term is k_observe_mse.cuh's.
#pragma once
#include "k_observe_mse.cuh"

namespace vsiq {

// candidate flags (wave-uniform, read with the candidate's parameters)
constexpr uint32_t kMseValid = 1u, kMseFast = 2u;

__device__ __forceinline__ float lane_f32(float v, int lane) {
  return u2f((uint32_t)__builtin_amdgcn_readlane((int)f2u(v), lane));
}

// One lane's sum of the error terms of its U groups for one candidate.  IEEE: fq_elem's
// division; else fq_elem_fast (the candidate passed fq_fast_qp and every element of the
// wave's step fq_x_ok: the same y bit for bit).  TAIL: bit 4k + j of `vm` says element j
// of group k exists.
template <bool IEEE, bool TAIL, int U>
__device__ __forceinline__ double mse_part(const f4 (&v)[U], const QP &p, uint32_t vm) {
  double a = 0.0;
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const float x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float y = IEEE ? fq_elem<true>(x[j], p).y : fq_elem_fast(x[j], p).y;
      const double t = mse_term(y, x[j]);
      a += (TAIL && !((vm >> (4 * k + j)) & 1u)) ? 0.0 : t;
    }
  }
  return a;
}

// Lane l of every wave holds the parameters of candidates l and l + 64 (ps / pr / pz /
// pf: scale, its reciprocal, zero point, flags) and the wave's error sums of those two
// (acc).  One step: the wave's U groups per lane against every candidate in turn, the
// candidate's parameters read into SGPRs, the lanes' partial sums reduced on DPP and
// added by the lane that owns the candidate.
template <bool TAIL, int U>
__device__ __forceinline__ void mse_step(const f4 (&v)[U], uint32_t vm, int count, const float (&ps)[2],
                                         const float (&pr)[2], const float (&pz)[2], const uint32_t (&pf)[2],
                                         float qlo, float qhi, double (&acc)[2]) {
  uint32_t ok = 1u;
#pragma unroll
  for (int k = 0; k < U; ++k) ok &= fq_x_ok(v[k].x) & fq_x_ok(v[k].y) & fq_x_ok(v[k].z) & fq_x_ok(v[k].w);
  const bool xfast = __ballot(!ok) == 0;
  const int lane = threadIdx.x % kWave;
#pragma unroll 1
  for (int h = 0; h < 2; ++h) {   // (one copy of the loop body: selects, not two unrolled halves)
    const float hs = h ? ps[1] : ps[0], hr = h ? pr[1] : pr[0], hz = h ? pz[1] : pz[0];
    const uint32_t hf = h ? pf[1] : pf[0];
    const int kn = count - h * kWave < kWave ? count - h * kWave : kWave;
    double own = 0.0;   // this step's sum of the candidate this lane owns
    for (int kk = 0; kk < kn; ++kk) {
      const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)hf, kk);
      if (!(f & kMseValid)) continue;   // its error is +inf whatever the tensor holds
      QP p;
      p.s = lane_f32(hs, kk);
      p.z = lane_f32(hz, kk);
      p.lo = qlo;
      p.hi = qhi;
      p.discrete = 0;
      p.d.b = p.s;
      p.d.r = lane_f32(hr, kk);
      p.d.fast = p.fast = (f & kMseFast) ? 1u : 0u;
      double part;
      if (xfast && p.fast) part = mse_part<false, TAIL, U>(v, p, vm);   // wave-uniform branch
      else part = mse_part<true, TAIL, U>(v, p, vm);
      const double red = wave_reduce(part, AddD());
      own = lane == kk ? red : own;
    }
    acc[0] += h ? 0.0 : own;
    acc[1] += h ? own : 0.0;
  }
}

}  // namespace vsiq
