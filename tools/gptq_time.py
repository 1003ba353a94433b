"""Time per_group_gptq (csrc/k_gptq.hip) against an eager-torch GPTQ loop on the same GPU and U.

    python tools/gptq_time.py [--rows 1024] [--rowlen 9216] [--reps 5] [--skip-eager]

HIP events around the whole call, one warm-up, the median of ``reps`` runs, for w4 g32 / g64 / g128.
The eager loop is the standard blocked implementation (128-column blocks, a per-column quantize and
rank-1 update inside a block, one matmul for the columns to its right), with the group's min/max
qparams taken at the group's first column.  For the kernels' shares, run it alone under a kernel
trace (``--skip-eager --reps 1``)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vsiquantization_amd as V  # noqa: E402


def eager_gptq(w, U, G, qmax):
    W = w.clone()
    Q = torch.empty_like(W)
    n = W.shape[1]
    for b in range(0, n, 128):
        e_ = min(b + 128, n)
        W1, Q1, E1, U1 = W[:, b:e_].clone(), Q[:, b:e_], torch.empty_like(W[:, b:e_]), U[b:e_, b:e_]
        for i in range(e_ - b):
            if (b + i) % G == 0:
                s = W1[:, i:i + G].abs().amax(1) / qmax
            q = torch.clamp(torch.round(W1[:, i] / s), -qmax - 1, qmax) * s
            Q1[:, i] = q
            err = (W1[:, i] - q) / U1[i, i]
            W1[:, i:] -= err[:, None] * U1[i, i:][None, :]
            E1[:, i] = err
        W[:, e_:] -= E1 @ U[b:e_, e_:]
    return Q


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--rowlen", type=int, default=9216)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-eager", action="store_true")
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(a.rows, a.rowlen, generator=g) * 0.05).cuda()
    X = (torch.randn(2 * a.rowlen, a.rowlen, generator=g) * (1 + torch.rand(a.rowlen, generator=g))).cuda()
    U = V.gptq_factor(torch.zeros(a.rowlen, a.rowlen, device="cuda").addmm_(X.t(), X, beta=0, alpha=1 / X.shape[0]))
    del X
    for G in (32, 64, 128):
        rec = {"rows": a.rows, "rowlen": a.rowlen, "group": G, "reps": a.reps}
        rec["hip_ms"] = timed(lambda: V.per_group_gptq(w, U, group_size=G, symmetric=True, qmin=-8, qmax=7,
                                                       obs_bits=4), a.reps)
        if not a.skip_eager:
            rec["eager_ms"] = timed(lambda: eager_gptq(w, U, G, 7), max(1, a.reps // 2))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
