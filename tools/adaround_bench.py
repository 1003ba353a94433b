"""Time AdaRound's two launches against the eager-torch composition of the same formulas.

    python tools/adaround_bench.py [--reps 200] [--out FILE]

For each shape ([1024, 9216] and [64, 27], per-channel 4-bit): the soft forward with R and
the backward (lambda != 0), each as a batch of `reps` back-to-back calls between two HIP
events (mean per call, median of 5 batches, after a warm-up batch), alternating with the
eager composition timed the same way in the same process.  The eager side is plain torch
ops on the same tensors (fp32; the regulariser's pow in f64 as the kernels do it), its
backward through autograd.  Algorithmic bytes: 12 B/elem forward (w, V in, y out), 16
B/elem backward (g, w, V in, grad_V out); the fraction is of 8 TB/s.  Prints one JSON
line per shape.  The [64, 27] times are host-bound call times (6.9 KB of data)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vsiquantization_amd.fakequant import adaround_backward, adaround_forward  # noqa: E402

PEAK = 8e12
LAM, BETA = 0.01, 3.7


def eager_forward(w, V, s, z, lo, hi, beta):
    sig = torch.sigmoid(V)
    h = torch.clamp(sig * 1.2 - 0.1, 0, 1)
    r = torch.floor(w / s + z) + h
    y = (torch.clamp(r, lo, hi) - z) * s
    u = torch.abs(2 * h.double() - 1)
    return y, torch.sum(1 - torch.pow(u, beta))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def bench(rows, rowlen, reps, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn((rows, rowlen), device=dev, generator=gen) * 0.05
    V = torch.empty((rows, rowlen), device=dev).uniform_(-4, 4, generator=gen)
    g = torch.randn((rows, rowlen), device=dev, generator=gen)
    s64 = (w.abs().amax(1) / 7).double()
    z64 = torch.zeros(rows, dtype=torch.float64, device=dev)
    s, z = s64.float().reshape(-1, 1), z64.float().reshape(-1, 1)
    Vp = V.clone().requires_grad_(True)

    def k_fwd():
        return adaround_forward(w, V, s64, z64, -8, 7, axis=0, beta=BETA)

    def k_bwd():
        return adaround_backward(g, w, V, s64, z64, -8, 7, axis=0, lam=LAM, beta=BETA)

    def e_fwd():
        with torch.no_grad():
            return eager_forward(w, V, s, z, -8, 7, BETA)

    def e_step():   # forward + backward through autograd (the backward alone cannot be run)
        y, reg = eager_forward(w, Vp, s, z, -8, 7, BETA)
        Vp.grad = None
        (torch.sum(y * g) + LAM * reg).backward()

    # the same numbers first: y and grad_V of the two sides agree to fp32 rounding
    ye, _ = e_fwd()
    yk, _ = k_fwd()
    e_step()
    gk = k_bwd()
    res = {"shape": [rows, rowlen], "reps": reps,
           "max_abs_dy": float((ye - yk).abs().max()), "max_abs_dgrad": float((Vp.grad - gk).abs().max())}
    n = rows * rowlen
    t = {}
    for _ in range(2):   # alternate the two sides; keep the second pass
        t["kernel_fwd_us"] = timed(k_fwd, reps)
        t["eager_fwd_us"] = timed(e_fwd, reps)
        t["kernel_bwd_us"] = timed(k_bwd, reps)
        t["eager_fwd_bwd_us"] = timed(e_step, reps)
    for k, (med, lo_, hi_) in t.items():
        res[k] = round(med, 2)
        res[k + "_range"] = [round(lo_, 2), round(hi_, 2)]
    res["fwd_fraction_of_8TBs"] = round(12 * n / (t["kernel_fwd_us"][0] * 1e-6) / PEAK, 4)
    res["bwd_fraction_of_8TBs"] = round(16 * n / (t["kernel_bwd_us"][0] * 1e-6) / PEAK, 4)
    res["fwd_speedup_vs_eager"] = round(t["eager_fwd_us"][0] / t["kernel_fwd_us"][0], 2)
    res["step_speedup_vs_eager"] = round(t["eager_fwd_bwd_us"][0] / (t["kernel_fwd_us"][0] + t["kernel_bwd_us"][0]), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [json.dumps(bench(r, c, a.reps, dev)) for r, c in ((1024, 9216), (64, 27))]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
