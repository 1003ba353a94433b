#!/usr/bin/env python
"""Time the bf16 / fp16 kernels against the fp32 kernel and against the only alternative a
half tensor had before them: widen to fp32, run the fp32 kernel, narrow the result.

Shape: C3's activation, 512 x 3 x 224 x 224 (77,070,336 elements), fused ReLU.  Ops: the
K5 forward, the STE backward (1-bit mask) and the K4 learnable backward.  For each op and
each of bf16 / fp16, in one process and interleaved launch by launch:

  typed   the 16-bit kernel (8-byte accesses)
  f32     the fp32 kernel on an fp32 copy of the same values
  widen   x.float() [, g.float()] -> fp32 kernel -> .to(T)

Every launch is timed with a pair of HIP events; the median of --launches (>= 20) launches
is reported, after a warm-up that lasts until the store-gate tuner has settled
(vsiq_gate_tuning_pending() == 0).  `bytes` are the bytes the algorithm must move (reads +
writes of the tensors and the mask), `frac` is bytes / time over 8 TB/s.  Prints a table
and one JSON line; exits 1 when a typed kernel is not faster than its widen sequence.
Needs the GPU (no fallback).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vsiquantization_amd import _hip as H              # noqa: E402
from vsiquantization_amd import fakequant as FQ        # noqa: E402

PEAK = 8.0e12   # B/s, MI355X HBM3E
SHAPE = (512, 3, 224, 224)
SCALE, QMIN, QMAX = 0.02, -128, 127


def timed(fn, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    return a, b


def measure(variants, launches, warm_max):
    """variants: name -> callable.  Interleaved; returns name -> median microseconds."""
    st = torch.cuda.current_stream()
    for i in range(warm_max):
        for fn in variants.values():
            fn()
        if i >= 3 and H.gate_tuning_pending() == 0:
            break
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(launches):
        for k, fn in variants.items():
            ev[k].append(timed(fn, st))
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warm-max", type=int, default=200)
    ap.add_argument("--elements", type=int, default=0, help="override the C3 element count (rehearsals)")
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("half_rate.py needs the GPU")
    dev = "cuda"
    n = args.elements or (SHAPE[0] * SHAPE[1] * SHAPE[2] * SHAPE[3])
    torch.manual_seed(0)
    c32 = torch.randn(n, device=dev)
    g32 = torch.randn(n, device=dev)
    mask_bytes = int(H.lib().vsiq_mask_words(1, n)) * 8
    rows, ok = [], True
    for dtype in (torch.bfloat16, torch.float16):
        c, g = c32.to(dtype), g32.to(dtype)
        cf, gf = c.float(), g.float()      # the same values, so both kernels do the same work
        _, mask, _ = FQ.fake_quant(c, SCALE, 0, QMIN, QMAX, want_mask=True, act="relu")
        e = c.element_size()
        ops = {
            "k5_fwd": (2 * n, 0,
                       lambda x=c: FQ.fake_quant(x, SCALE, 0, QMIN, QMAX, act="relu"),
                       lambda x=cf: FQ.fake_quant(x, SCALE, 0, QMIN, QMAX, act="relu"),
                       lambda x=c, t=dtype: FQ.fake_quant(x.float(), SCALE, 0, QMIN, QMAX, act="relu")[0].to(t)),
            "ste_bwd": (3 * n, mask_bytes,
                        lambda: FQ.ste_backward(g, mask, SCALE, pre=c, act="relu"),
                        lambda: FQ.ste_backward(gf, mask, SCALE, pre=cf, act="relu"),
                        lambda t=dtype: FQ.ste_backward(g.float(), mask, SCALE, pre=c.float(), act="relu").to(t)),
            "k4_bwd": (3 * n, 0,
                       lambda: FQ.lsq_backward(g, c, SCALE, 0, QMIN, QMAX, 1e-3, 0, act="relu"),
                       lambda: FQ.lsq_backward(gf, cf, SCALE, 0, QMIN, QMAX, 1e-3, 0, act="relu"),
                       lambda t=dtype: FQ.lsq_backward(g.float(), c.float(), SCALE, 0, QMIN, QMAX, 1e-3, 0,
                                                       act="relu")[0].to(t)),
        }
        for op, (elems, extra, typed, f32, widen) in ops.items():
            us = measure({"typed": typed, "f32": f32, "widen": widen}, args.launches, args.warm_max)
            bt, bf = elems * e + extra, elems * 4 + extra
            rows.append(dict(op=op, dtype=str(dtype).replace("torch.", ""), n=n, typed_us=round(us["typed"], 1),
                             f32_us=round(us["f32"], 1), widen_us=round(us["widen"], 1), typed_bytes=bt, f32_bytes=bf,
                             typed_frac=round(bt / (us["typed"] * 1e-6) / PEAK, 3),
                             f32_frac=round(bf / (us["f32"] * 1e-6) / PEAK, 3),
                             typed_over_f32=round(us["typed"] / us["f32"], 3),
                             typed_over_widen=round(us["typed"] / us["widen"], 3)))
            ok = ok and us["typed"] < us["widen"]
        del c, g, cf, gf, mask
    print(f"{'op':8} {'dtype':9} {'typed us':>9} {'frac':>6} {'f32 us':>8} {'frac':>6} {'widen us':>9} "
          f"{'t/f32':>6} {'t/widen':>8}")
    for r in rows:
        print(f"{r['op']:8} {r['dtype']:9} {r['typed_us']:9.1f} {r['typed_frac']:6.3f} {r['f32_us']:8.1f} "
              f"{r['f32_frac']:6.3f} {r['widen_us']:9.1f} {r['typed_over_f32']:6.3f} {r['typed_over_widen']:8.3f}")
    print(json.dumps({"tool": "half_rate", "device": torch.cuda.get_device_name(0), "launches": args.launches,
                      "peak_bytes_per_s": PEAK, "typed_faster_than_widen": ok, "rows": rows}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
