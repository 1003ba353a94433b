"""PerChannelMSEObserver's per-call cost at four weight shapes, K = 64 candidates, 4-bit
symmetric grid:

  * pcmse     fakequant.per_channel_observe_mse, observe-only and with the fake-quantized y,
  * K3        fakequant.per_channel_observe_fq on the same tensor (the memory-bound floor),
  * mse       the per-tensor observe_mse (K2 + the search pass) on the same rows * rowlen
              elements: the same element-candidate count,
  * eager     the torch loop it replaces, timed on ONE row and multiplied by rows,

timed by HIP events around R repetitions after warm-up, the variants alternated.  DESIGN.md
§5.1 holds the numbers.  usage: python tools/exp/pc_mse_bench.py [reps]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vsiquantization_amd.fakequant import (mse_ratios, observe_mse, per_channel_observe_fq,  # noqa: E402
                                           per_channel_observe_mse)

SHAPES = ((1024, 9216), (256, 1152), (64, 27), (128, 9))
K, BITS = 64, 4
QMIN, QMAX = -8, 7


def eager_row(v, ratios):
    """The loop a toolkit writes in eager torch for one row (symmetric grid)."""
    m = v.abs().max()
    best, pick = None, 0
    for k, r in enumerate(ratios):
        s = m * r / (QMAX + 1e-8)
        y = torch.clamp(torch.round(v / s), QMIN, QMAX) * s
        e = (y.double() - v.double()).square().sum()
        if best is None:
            best = e
        else:
            better = e < best
            best = torch.where(better, e, best)
            pick = torch.where(better, k, pick)
    return best, pick


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    ratios = mse_ratios(K)
    print(f"{'shape':>12s} {'pcmse us':>9s} {'pcmse+y us':>10s} {'K3 us':>8s} {'mse us':>9s} {'eager us':>10s} "
          f"{'pcmse/mse':>9s} {'Gec/s':>7s}")
    for rows, rowlen in SHAPES:
        x = torch.randn(rows, rowlen, device=dev, generator=gen)
        flat = x.reshape(-1)
        state = torch.zeros(2, rows, dtype=torch.float32, device=dev)
        s1 = torch.zeros(2, dtype=torch.float32, device=dev)
        kw = dict(symmetric=True, qmin=QMIN, qmax=QMAX, num_bits=BITS, run_min=state[0], run_max=state[1])

        def pc_obs():
            per_channel_observe_mse(x, ratios=ratios, quantize=False, **kw)

        def pc_fq():
            per_channel_observe_mse(x, ratios=ratios, **kw)

        def k3():
            per_channel_observe_fq(x, symmetric=True, qmin=QMIN, qmax=QMAX, obs_bits=BITS, run_min=state[0],
                                   run_max=state[1])

        def mse():
            observe_mse(flat, symmetric=True, num_bits=BITS, run_minmax=s1, ratios=ratios, qmin=QMIN, qmax=QMAX)

        def eager():
            eager_row(x[0], ratios)

        fns = ((pc_obs, reps), (pc_fq, reps), (k3, reps * 5), (mse, reps), (eager, max(2, reps // 5)))
        for f, _ in fns:
            for _ in range(2):
                f()
        total, count = [0.0] * len(fns), [0] * len(fns)
        rounds = 2   # alternate the variants: drift of a shared machine hits all alike
        for _ in range(rounds):
            for i, (f, r) in enumerate(fns):
                e0, e1 = bench.HipEvent(), bench.HipEvent()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(max(1, r // rounds)):
                    f()
                e1.record()
                torch.cuda.synchronize()
                total[i] += e0.elapsed_time(e1) * 1e3
                count[i] += max(1, r // rounds)
        t_obs, t_fq, t_k3, t_mse, t_eager = (t / c for t, c in zip(total, count))
        t_eager *= rows   # one row timed, every row is such a loop
        ecs = rows * rowlen * K / (t_obs * 1e-6)
        print(f"{rows:6d}x{rowlen:<5d} {t_obs:9.1f} {t_fq:10.1f} {t_k3:8.1f} {t_mse:9.1f} {t_eager:10.1f} "
              f"{t_obs / t_mse:9.2f} {ecs / 1e9:7.1f}", flush=True)


if __name__ == "__main__":
    main()
