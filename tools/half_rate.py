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

--k4d: the records-only learnable backward (K4d, vsiq_act_lsq_bwd_part_t) instead, at the
C4 activation sizes (YOLOv8n backbone at 320 x 320, batch 256: 3.3M, 6.6M, 13M and 26M
elements), fused ReLU, 4-bit symmetric.  Per dtype and size, interleaved as above:

  k4d     the typed records-only launch (no fold)
  k4      the typed per-call K4 on the same tensors (what a half tensor took before K4d)
  f32     the fp32 records-only launch on an fp32 copy of the same values

and one whole-backward row per dtype over the backbone's 27 activation sizes: 27 typed
records-only launches + ONE vsiq_lsq_fold_multi against 27 typed per-call K4 launches, each
sequence between one pair of events behind a device-side blocker (so the launches are queued
when the first one starts and the time is the device's, not the host's).  No exit status
from the comparison: the numbers are the result.
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


def yolov8n_backbone_sizes(batch=256, img=320, width=(3, 16, 32, 64, 128, 256), depth=(1, 2, 2)):
    """Elements of the 27 activation-quantizer inputs of the YOLOv8n backbone (bench.py's C4
    layer list: batch x cout x hout x hout), in forward order."""
    sizes, h = [], img

    def conv(cout, k, s):
        nonlocal h
        h = (h + 2 * ((k - 1) // 2) - k) // s + 1
        sizes.append(batch * cout * h * h)

    def csp(cout, n):
        conv(cout, 1, 1)
        for _ in range(2 * n):
            conv(cout // 2, 3, 1)
        conv(cout, 1, 1)

    conv(width[1], 3, 2)
    for w, d in zip(width[2:], depth + depth[:1]):
        conv(w, 3, 2)
        csp(w, d)
    conv(width[5] // 2, 1, 1)
    conv(width[5], 1, 1)   # SPP
    return sizes


K4D_SIZES = (128 * 10 * 10 * 256, 64 * 20 * 20 * 256, 32 * 40 * 40 * 256, 16 * 80 * 80 * 256)
K4D_SCALE, K4D_QMIN, K4D_QMAX = 0.3, -8, 7


def k4d_main(args):
    from vsiquantization_amd.quantizers import deferred as D
    dev = "cuda"
    lib = H.lib()
    torch.manual_seed(0)
    nrec = lambda n: int(lib.vsiq_lsq_part_records(H.c_i64(n)))                      # noqa: E731
    part = lambda g, c, rec: D.lsq_backward_part(g, c, K4D_SCALE, 0, K4D_QMIN, K4D_QMAX, False, "relu", rec)  # noqa: E731
    k4 = lambda g, c: FQ.lsq_backward(g, c, K4D_SCALE, 0, K4D_QMIN, K4D_QMAX, 1e-3, 0, act="relu")            # noqa: E731
    sizes = [max(4, int(n * args.shrink) // 4 * 4) for n in K4D_SIZES]
    rows = []
    for dtype in (torch.bfloat16, torch.float16):
        for n in sizes:
            c = torch.randn(n, device=dev).to(dtype)
            g = torch.randn(n, device=dev).to(dtype)
            cf, gf = c.float(), g.float()
            rec = torch.empty(2 * nrec(n), dtype=torch.float64, device=dev)
            us = measure({"k4d": lambda: part(g, c, rec), "k4": lambda: k4(g, c), "f32": lambda: part(gf, cf, rec)},
                         args.launches, args.warm_max)
            bt, bf = 3 * n * c.element_size(), 3 * n * 4
            rows.append(dict(op="k4d_bwd", dtype=str(dtype).replace("torch.", ""), n=n, k4d_us=round(us["k4d"], 2),
                             k4_us=round(us["k4"], 2), f32_k4d_us=round(us["f32"], 2), typed_bytes=bt, f32_bytes=bf,
                             k4d_frac=round(bt / (us["k4d"] * 1e-6) / PEAK, 3),
                             k4d_over_k4=round(us["k4d"] / us["k4"], 3),
                             k4d_over_f32=round(us["k4d"] / us["f32"], 3)))
            del c, g, cf, gf, rec
    # the whole backward of the backbone's 27 activation quantizers
    layer_n = [max(4, int(n * args.shrink) // 4 * 4) for n in yolov8n_backbone_sizes()]
    blocker = torch.empty(int((1 << 29) * min(1.0, args.shrink * 64)), device=dev)   # 2 GiB: ~1 ms of copy
    blocker2 = torch.empty_like(blocker)
    st = torch.cuda.current_stream()
    whole = []
    for dtype in (torch.bfloat16, torch.float16):
        cs = [torch.randn(n, device=dev).to(dtype) for n in layer_n]
        gs = [torch.randn(n, device=dev).to(dtype) for n in layer_n]
        entries = []
        for n in layer_n:
            e = D._Fold()
            e.nrec = nrec(n)
            e.records = torch.empty(2 * e.nrec, dtype=torch.float64, device=dev)
            e.zd, e.zh, e.gscale, e.qmin, e.qmax, e.learn_zp = None, 0.0, 1e-3, K4D_QMIN, K4D_QMAX, False
            e.out = torch.empty(2, dtype=torch.float64, device=dev)
            entries.append(e)

        def deferred():
            for g, c, e in zip(reversed(gs), reversed(cs), reversed(entries)):
                part(g, c, e.records)
            D.fold(entries)

        def per_call():
            for g, c in zip(reversed(gs), reversed(cs)):
                k4(g, c)

        for i in range(args.warm_max):
            deferred()
            per_call()
            if i >= 3 and H.gate_tuning_pending() == 0:
                break
        torch.cuda.synchronize()
        ev = {"deferred": [], "per_call": []}
        for _ in range(args.launches):
            for k, fn in (("deferred", deferred), ("per_call", per_call)):
                blocker2.copy_(blocker)
                ev[k].append(timed(fn, st))
            torch.cuda.synchronize()
        us = {k: statistics.median(a.elapsed_time(b) * 1e3 for a, b in v) for k, v in ev.items()}
        whole.append(dict(op="k4d_backward_27", dtype=str(dtype).replace("torch.", ""), layers=len(layer_n),
                          elements=sum(layer_n), deferred_us=round(us["deferred"], 1),
                          per_call_us=round(us["per_call"], 1),
                          deferred_over_per_call=round(us["deferred"] / us["per_call"], 3)))
        del cs, gs, entries
    print(f"{'op':8} {'dtype':9} {'n':>10} {'k4d us':>8} {'frac':>6} {'k4 us':>8} {'f32 k4d':>8} {'k4d/k4':>7} "
          f"{'k4d/f32':>8}")
    for r in rows:
        print(f"{r['op']:8} {r['dtype']:9} {r['n']:10d} {r['k4d_us']:8.2f} {r['k4d_frac']:6.3f} {r['k4_us']:8.2f} "
              f"{r['f32_k4d_us']:8.2f} {r['k4d_over_k4']:7.3f} {r['k4d_over_f32']:8.3f}")
    print(f"{'op':16} {'dtype':9} {'elements':>10} {'27 k4d + fold us':>17} {'27 k4 us':>9} {'ratio':>6}")
    for r in whole:
        print(f"{r['op']:16} {r['dtype']:9} {r['elements']:10d} {r['deferred_us']:17.1f} {r['per_call_us']:9.1f} "
              f"{r['deferred_over_per_call']:6.3f}")
    print(json.dumps({"tool": "half_rate --k4d", "device": torch.cuda.get_device_name(0), "launches": args.launches,
                      "peak_bytes_per_s": PEAK, "rows": rows, "whole_backward": whole}))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warm-max", type=int, default=200)
    ap.add_argument("--elements", type=int, default=0, help="override the C3 element count (rehearsals)")
    ap.add_argument("--k4d", action="store_true", help="time the records-only learnable backward at the C4 sizes")
    ap.add_argument("--shrink", type=float, default=1.0, help="--k4d: scale every element count (rehearsals)")
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("half_rate.py needs the GPU")
    if args.k4d:
        return k4d_main(args)
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
