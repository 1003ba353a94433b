"""Time group-wise quantization (csrc/k_pg.hip) against the only route there was before it.

    python tools/bench_per_group.py [--reps 200] [--rounds 7] [--out FILE]

For each shape ([1024, 9216] and [256, 1152]) and group size (32, 128):

  new   per_group_observe_fq(x, group_size=G, want_mask=True)           and pg_ste_backward
  old   per_channel_observe_fq(x.view(-1, G), want_mask=True)  (K3)     and pc_ste_backward

Each measurement is a batch of `reps` back-to-back calls between two HIP events (mean per call),
after a warm-up batch; the two routes alternate for `rounds` rounds and the median, minimum and
maximum over the rounds are reported in microseconds, so the spread of each route is next to
the difference between them.  All output and state buffers are allocated by the calls
themselves, as a user's are.  Algorithmic bytes of the new route: forward 8 B / element (x in, y
out) + 1 bit / element of mask + 24 B / group of qparams and state; backward 8 B / element + the
mask + 8 B / group; reported over the median time as a fraction of 8 TB/s.  The mask bytes of
both routes are printed: the reshaped route pads every G-element row to 256 mask bits.
One JSON line per (shape, G).  Reads nothing outside the repository."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vsiquantization_amd import _hip as H  # noqa: E402
from vsiquantization_amd.fakequant import (pc_ste_backward, per_channel_observe_fq, per_group_observe_fq,  # noqa: E402
                                           pg_ste_backward)

PEAK = 8e12
SHAPES = ((1024, 9216), (256, 1152))
GROUPS = (32, 128)


def batch_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(fns, reps, rounds):
    """{name: (median, min, max)} of `rounds` batches of every fn, the fns taking turns."""
    for fn in fns.values():   # warm-up batch each
        batch_us(fn, reps)
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(batch_us(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def bench(rows, rowlen, G, reps, rounds, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((rows, rowlen), device=dev, generator=gen) * 0.05
    g = torch.randn((rows, rowlen), device=dev, generator=gen)
    xv, gv = x.view(-1, G), g.view(-1, G)
    kw = dict(symmetric=True, qmin=-8, qmax=7, want_mask=True)
    new = per_group_observe_fq(x, group_size=G, **kw)
    old = per_channel_observe_fq(xv, **kw)
    assert torch.equal(new["y"].view(-1, G), old["y"]) and torch.equal(new["scale"].view(-1), old["scale"])
    assert torch.equal(pg_ste_backward(g, new["mask"], new["scale"], G).view(-1, G),
                       pc_ste_backward(gv, old["mask"], old["scale"]))
    t = alternate({
        "new_fwd": lambda: per_group_observe_fq(x, group_size=G, **kw),
        "old_fwd": lambda: per_channel_observe_fq(xv, **kw),
        "new_bwd": lambda: pg_ste_backward(g, new["mask"], new["scale"], G),
        "old_bwd": lambda: pc_ste_backward(gv, old["mask"], old["scale"]),
    }, reps, rounds)
    n, groups = rows * rowlen, rows * (rowlen // G)
    mask_new = 8 * int(H.lib().vsiq_mask_words(rows, rowlen))
    mask_old = 8 * int(H.lib().vsiq_mask_words(rows * (rowlen // G), G))
    res = {"shape": [rows, rowlen], "G": G, "reps": reps, "rounds": rounds,
           "mask_bytes_new": mask_new, "mask_bytes_old": mask_old}
    for k, (med, lo, hi) in t.items():
        res[k + "_us"] = round(med, 2)
        res[k + "_range"] = [round(lo, 2), round(hi, 2)]
    res["new_fwd_fraction_of_8TBs"] = round((8 * n + mask_new + 24 * groups) / (t["new_fwd"][0] * 1e-6) / PEAK, 4)
    res["new_bwd_fraction_of_8TBs"] = round((8 * n + mask_new + 8 * groups) / (t["new_bwd"][0] * 1e-6) / PEAK, 4)
    res["fwd_old_over_new"] = round(t["old_fwd"][0] / t["new_fwd"][0], 2)
    res["bwd_old_over_new"] = round(t["old_bwd"][0] / t["new_bwd"][0], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for rows, rowlen in SHAPES:
        for G in GROUPS:
            lines.append(json.dumps(bench(rows, rowlen, G, a.reps, a.rounds, "cuda:0")))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
