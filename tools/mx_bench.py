"""Time the MX fake-quant kernels (csrc/k_mx.hip) against an eager-torch MX composition and
against the group-wise forward at g32 on the same weight.

    python tools/mx_bench.py [--reps 100] [--out FILE]

Shapes: a [1024, 9216] weight (row form, blocks along the rows) and a [256, 64, 56, 56]
activation (column form, blocks along the channels).  For fp4_e2m1 and fp8_e4m3: the forward
alone (y) and with codes + scales + mask, each as a batch of `reps` back-to-back calls between
two HIP events (mean per call, median of 5 batches, after a warm-up batch), alternating with
  (a) the eager composition on the GPU: amax per block, floor(log2), exp2, clamp, the grid
      rounding by an add and subtract of a power of two, rescale (same y for finite inputs);
  (b) the weight only: per_group_fake_quant at group 32 with given qparams (k_pg.hip), the
      in-project yardstick for a block kernel at this shape.
Algorithmic bytes: 8 B/elem for y alone (x in, y out); 9 B + 1/32 B (scales) + 1/8 B (mask)
with all outputs; the fraction is of 8 TB/s.  Prints one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vsiquantization_amd import fakequant as FQ  # noqa: E402

PEAK = 8e12
# name -> (emax, emin, mantissa bits, max normal)
FORMATS = {"fp4_e2m1": (2, 0, 1, 6.0), "fp8_e4m3": (8, -6, 3, 448.0)}


def eager_mx(x, fmt, dim):
    """MX fake quant of finite x in plain torch ops, blocks of 32 along ``dim`` (its size a multiple of 32)."""
    emax, emin, mbits, maxn = FORMATS[fmt]
    shape = x.shape
    xb = x.unflatten(dim, (shape[dim] // 32, 32))
    amax = xb.abs().amax(dim + 1, keepdim=True)
    e = torch.clamp(torch.floor(torch.log2(amax)) - emax, min=-127.0)
    a = xb.abs() * torch.exp2(-e)
    step = torch.exp2(torch.clamp(torch.floor(torch.log2(a)), min=float(emin)) - mbits)
    q = torch.clamp(torch.round(a / step) * step, max=maxn)
    return (torch.copysign(q, xb) * torch.exp2(e)).reshape(shape)


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


def bench(shape, axis, reps, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(shape, device=dev, generator=gen) * 0.05
    n = x.numel()
    res = {"shape": list(shape), "axis": axis, "reps": reps}
    sides = {}
    for fmt in FORMATS:
        sides[f"kernel_{fmt}_y_us"] = lambda fmt=fmt: FQ._mx_forward(x, fmt, axis, False, False)
        sides[f"kernel_{fmt}_all_us"] = lambda fmt=fmt: FQ._mx_forward(x, fmt, axis, True, True)
        sides[f"eager_{fmt}_us"] = lambda fmt=fmt: eager_mx(x, fmt, axis % x.dim())
        ye, yk = sides[f"eager_{fmt}_us"](), sides[f"kernel_{fmt}_y_us"]()[0]
        res[f"max_abs_dy_{fmt}"] = float((ye - yk).abs().max())   # the same numbers first
    if axis == -1:
        ngr = shape[1] // 32
        scale = (x.view(shape[0], ngr, 32).abs().amax(2) / 7).double()
        zp = torch.zeros_like(scale)
        sides["pg_g32_y_us"] = lambda: FQ.per_group_fake_quant(x, scale, zp, -8, 7, group_size=32)
        sides["pg_g32_all_us"] = lambda: FQ.per_group_fake_quant(x, scale, zp, -8, 7, group_size=32, want_mask=True,
                                                                 want_codes=True)
    t = {}
    for _ in range(2):   # alternate the sides; keep the second pass
        for k, fn in sides.items():
            t[k] = timed(fn, reps)
    for k, (med, lo, hi) in t.items():
        res[k] = round(med, 2)
        res[k + "_range"] = [round(lo, 2), round(hi, 2)]
    for fmt in FORMATS:
        res[f"{fmt}_y_fraction_of_8TBs"] = round(8 * n / (t[f"kernel_{fmt}_y_us"][0] * 1e-6) / PEAK, 4)
        res[f"{fmt}_all_fraction_of_8TBs"] = round((9 + 1 / 32 + 1 / 8) * n / (t[f"kernel_{fmt}_all_us"][0] * 1e-6) / PEAK, 4)
        res[f"{fmt}_speedup_vs_eager"] = round(t[f"eager_{fmt}_us"][0] / t[f"kernel_{fmt}_y_us"][0], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [json.dumps(bench(s, ax, a.reps, dev)) for s, ax in (((1024, 9216), -1), ((256, 64, 56, 56), 1))]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
