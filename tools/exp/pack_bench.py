"""The export kernels' per-call cost at the north-star weight (1024 x 9216) and a first-layer
weight (64 x 27), per channel, for 2 / 4 / 8-bit fields:

  * pack      fakequant.quantize_pack (one launch: codes, fields, fp32 qparams),
  * codes+sh  what the package offered before: per_channel_fake_quant(want_codes=True), then
              eager-torch shifts and ors of the int8 / uint8 codes into the same layout,
  * unpack    fakequant.unpack_dequant into fp32 and bf16,
  * eager     the eager-torch inverse (shifts, mask, + qmin, - zp, * s) into the same dtype,
  * K3-fixed  per_channel_fake_quant alone (the existing per-channel forward: 8 B/elem),

timed by HIP events around R repetitions after warm-up, the variants alternated; each line
also gives the fraction of 8 TB/s the kernel's algorithmic bytes (pack 4 + bits/8, unpack
bits/8 + sizeof(y) per element) amount to.  DESIGN.md §5.1 holds the numbers.
usage: python tools/exp/pack_bench.py [reps]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vsiquantization_amd.fakequant import per_channel_fake_quant, quantize_pack, unpack_dequant  # noqa: E402

SHAPES = ((1024, 9216), (64, 27))
PEAK = 8e12


def eager_pack(codes, qmin, bits, row_bytes):
    """int8 / uint8 codes [rows, rowlen] -> the packed layout with eager torch ops."""
    rows, rowlen = codes.shape
    per = 8 // bits
    f = (codes.to(torch.int16) - qmin).to(torch.uint8)
    pad = row_bytes * per - rowlen
    if pad:
        f = torch.nn.functional.pad(f, (0, pad))
    f = f.reshape(rows, row_bytes, per)
    out = f[:, :, 0].clone()
    for k in range(1, per):
        out |= f[:, :, k] << (k * bits)
    return out


def eager_unpack(data, qparams, rowlen, qmin, bits, dtype):
    per = 8 // bits
    shifts = torch.arange(per, device=data.device, dtype=torch.uint8) * bits
    f = (data.unsqueeze(-1) >> shifts) & ((1 << bits) - 1)
    q = f.reshape(data.shape[0], -1)[:, :rowlen].to(torch.float32) + qmin
    return ((q - qparams[:, 1:2]) * qparams[:, 0:1]).to(dtype)


def timed(fns, reps, rounds=2):
    for f in fns:
        for _ in range(3):
            f()
    total = [0.0] * len(fns)
    n = max(1, reps // rounds)
    for _ in range(rounds):   # alternate the variants: drift of a shared machine hits all alike
        for i, f in enumerate(fns):
            e0, e1 = bench.HipEvent(), bench.HipEvent()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                f()
            e1.record()
            torch.cuda.synchronize()
            total[i] += e0.elapsed_time(e1) * 1e3
    return [t / (n * rounds) for t in total]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    print(f"{'shape':>12s} {'bits':>4s} {'pack us':>8s} {'frac':>5s} {'codes+sh us':>11s} {'K3-fixed us':>11s} {'frac':>5s} "
          f"{'unpack32 us':>11s} {'frac':>5s} {'eager32 us':>10s} {'unpack16 us':>11s} {'frac':>5s} {'eager16 us':>10s}")
    for rows, rowlen in SHAPES:
        n = rows * rowlen
        x = torch.randn(rows, rowlen, device=dev, generator=gen)
        for bits in (2, 4, 8):
            qmin, qmax = -(2 ** (bits - 1)), 2 ** (bits - 1) - 1
            s = (x.abs().amax(dim=1) / qmax).to(torch.float64)
            z = torch.zeros(rows, dtype=torch.float64, device=dev)
            p = quantize_pack(x, s, z, qmin, qmax, bits=bits, axis=0)
            rb = p.data.shape[1]
            codes = per_channel_fake_quant(x, s, z, qmin, qmax, want_codes=True)[2]
            assert torch.equal(eager_pack(codes, qmin, bits, rb), p.data)
            assert torch.equal(eager_unpack(p.data, p.qparams, rowlen, qmin, bits, torch.float32), unpack_dequant(p))
            fns = (lambda: quantize_pack(x, s, z, qmin, qmax, bits=bits, axis=0),
                   lambda: eager_pack(per_channel_fake_quant(x, s, z, qmin, qmax, want_codes=True)[2], qmin, bits, rb),
                   lambda: per_channel_fake_quant(x, s, z, qmin, qmax),
                   lambda: unpack_dequant(p),
                   lambda: eager_unpack(p.data, p.qparams, rowlen, qmin, bits, torch.float32),
                   lambda: unpack_dequant(p, torch.bfloat16),
                   lambda: eager_unpack(p.data, p.qparams, rowlen, qmin, bits, torch.bfloat16))
            t = timed(fns, reps)
            frac = lambda b, us: n * b / (us * 1e-6) / PEAK   # noqa: E731
            print(f"{rows:6d}x{rowlen:<5d} {bits:4d} {t[0]:8.1f} {frac(4 + bits / 8, t[0]):5.2f} {t[1]:11.1f} "
                  f"{t[2]:11.1f} {frac(8, t[2]):5.2f} {t[3]:11.1f} {frac(bits / 8 + 4, t[3]):5.2f} {t[4]:10.1f} "
                  f"{t[5]:11.1f} {frac(bits / 8 + 2, t[5]):5.2f} {t[6]:10.1f}", flush=True)


if __name__ == "__main__":
    main()
