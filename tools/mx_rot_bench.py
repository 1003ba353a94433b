"""Time Hadamard-rotated MX fake quantization (csrc/k_mx_rot.hip) against the route a user had
before it -- hadamard_transform -> mx_fake_quant -> hadamard_transform, three launches of this
same commit -- and against plain mx_fake_quant.

    python tools/mx_rot_bench.py [--reps 100] [--out FILE]

Shapes: a [1024, 9216] weight (row form) and a [64, 64, 80, 80] activation with blocks along
axis 1 (column form).  hadamard_transform works on rows only, so the activation's composition
carries the two transposing copies it needs (NCHW -> NHWC and back), forward and backward.
fp4_e2m1; forward (y + mask, what training saves) and backward (from the saved mask), each as a
batch of `reps` back-to-back calls between two HIP events (mean per call, median of 5 batches
after a warm-up call), the sides alternated and the second pass kept (tools/mx_bench.py's
timing).  Algorithmic bytes of a fused call: 8 B/elem; the fraction is of 8 TB/s.  Prints one
JSON line per shape."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mx_bench import PEAK, timed  # noqa: E402
from vsiquantization_amd import fakequant as FQ  # noqa: E402

FMT = "fp4_e2m1"


def bench(shape, axis, reps, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(shape, device=dev, generator=gen) * 0.05
    g = torch.randn(shape, device=dev, generator=gen)
    cols = axis == 1
    to_rows = (lambda t: t.permute(0, 2, 3, 1).contiguous()) if cols else (lambda t: t)
    back = (lambda t: t.permute(0, 3, 1, 2).contiguous()) if cols else (lambda t: t)
    mask = FQ._mx_rot_forward(x, FMT, axis, False, True)[4]
    mask3 = FQ._mx_forward(FQ.hadamard_transform(to_rows(x), 32), FMT, -1, False, True)[3]

    def composed_fwd():
        yr, _, _, m = FQ._mx_forward(FQ.hadamard_transform(to_rows(x), 32), FMT, -1, False, True)
        return back(FQ.hadamard_transform(yr, 32)), m

    def composed_bwd():
        return back(FQ.hadamard_transform(FQ.ste_backward(FQ.hadamard_transform(to_rows(g), 32), mask3, 1.0, 0), 32))

    sides = {
        "fused_fwd_us": lambda: FQ._mx_rot_forward(x, FMT, axis, False, True),
        "composed_fwd_us": composed_fwd,
        "mx_fwd_us": lambda: FQ._mx_forward(x, FMT, axis, False, True),
        "fused_bwd_us": lambda: FQ.mx_rot_ste_backward(g, mask, axis),
        "composed_bwd_us": composed_bwd,
    }
    assert torch.equal(sides["fused_fwd_us"]()[0].view(torch.int32), composed_fwd()[0].view(torch.int32))
    assert torch.equal(sides["fused_bwd_us"]().view(torch.int32), composed_bwd().view(torch.int32))
    t = {}
    for _ in range(2):   # alternate the sides; keep the second pass
        for k, fn in sides.items():
            t[k] = timed(fn, reps)
    res = {"shape": list(shape), "axis": axis, "fmt": FMT, "reps": reps}
    for k, (med, lo, hi) in t.items():
        res[k] = round(med, 2)
        res[k + "_range"] = [round(lo, 2), round(hi, 2)]
    for way in ("fwd", "bwd"):
        res[f"fused_{way}_fraction_of_8TBs"] = round(8 * x.numel() / (t[f"fused_{way}_us"][0] * 1e-6) / PEAK, 4)
        res[f"{way}_speedup_vs_composed"] = round(t[f"composed_{way}_us"][0] / t[f"fused_{way}_us"][0], 2)
    res["fused_fwd_over_mx_fwd"] = round(t["fused_fwd_us"][0] / t["mx_fwd_us"][0], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps(bench(s, ax, a.reps, "cuda:0")) for s, ax in (((1024, 9216), -1), ((64, 64, 80, 80), 1))]
    for ln in lines:
        print(ln, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
