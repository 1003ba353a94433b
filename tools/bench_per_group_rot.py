"""Time Hadamard-rotated group-wise quantization (csrc/k_rot.hip) against the route a user had
before it and against the unrotated kernel that moves the same bytes.

    python tools/bench_per_group_rot.py [--reps 200] [--rounds 7] [--out FILE]

For each shape ([1024, 9216] and [256, 1152]) and group size (32, 128), forward and backward:

  rot    per_group_rot_observe_fq(x, group_size=G, want_mask=True)  and pg_rot_ste_backward
  old    (x.view(-1, G) @ H_G) -> per_group_observe_fq / pg_ste_backward -> (. @ H_G): two dense fp32
         torch.matmul with the orthonormal Hadamard matrix around the group-wise kernel
  plain  per_group_observe_fq / pg_ste_backward alone: the floor for a kernel moving these bytes;
         rot / plain is the cost of the two transforms

Timing as tools/bench_per_group.py: batches of `reps` back-to-back calls between two HIP events after
a warm-up batch, the routes taking turns for `rounds` rounds; median, minimum and maximum over the
rounds in microseconds.  Algorithmic bytes of the rotated forward: 8 B / element + 1 bit / element of
mask + 24 B / group; backward 8 B / element + the mask + 8 B / group; over the median time as a
fraction of 8 TB/s.  The matmul route's results differ from the kernel's in the last bits (its sums
run in another order), so only closeness is asserted for it.  One JSON line per (shape, G)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_per_group import GROUPS, PEAK, SHAPES, alternate  # noqa: E402
from vsiquantization_amd import _hip as H  # noqa: E402
from vsiquantization_amd.fakequant import (hadamard_transform, per_group_observe_fq, per_group_rot_observe_fq,  # noqa: E402
                                           pg_rot_ste_backward, pg_ste_backward)


def bench(rows, rowlen, G, reps, rounds, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((rows, rowlen), device=dev, generator=gen) * 0.05
    g = torch.randn((rows, rowlen), device=dev, generator=gen)
    Hm = hadamard_transform(torch.eye(G, device=dev), G)
    kw = dict(group_size=G, symmetric=True, qmin=-8, qmax=7, want_mask=True)

    def old_fwd():
        r = per_group_observe_fq((x.view(-1, G) @ Hm).view(rows, rowlen), **kw)
        return (r["y"].view(-1, G) @ Hm).view(rows, rowlen), r

    rot = per_group_rot_observe_fq(x, **kw)
    plain = per_group_observe_fq(x, **kw)
    y_old, r_old = old_fwd()
    assert float((y_old - rot["y"]).abs().mean()) < 0.01 * float(rot["scale"].mean())   # a few flipped roundings

    def old_bwd():
        gr = pg_ste_backward((g.view(-1, G) @ Hm).view(rows, rowlen), r_old["mask"], r_old["scale"], G)
        return (gr.view(-1, G) @ Hm).view(rows, rowlen)

    t = alternate({
        "rot_fwd": lambda: per_group_rot_observe_fq(x, **kw),
        "old_fwd": old_fwd,
        "plain_fwd": lambda: per_group_observe_fq(x, **kw),
        "rot_bwd": lambda: pg_rot_ste_backward(g, rot["mask"], rot["scale"], G),
        "old_bwd": old_bwd,
        "plain_bwd": lambda: pg_ste_backward(g, plain["mask"], plain["scale"], G),
    }, reps, rounds)
    n, groups = rows * rowlen, rows * (rowlen // G)
    mask = 8 * int(H.lib().vsiq_mask_words(rows, rowlen))
    res = {"shape": [rows, rowlen], "G": G, "reps": reps, "rounds": rounds}
    for k, (med, lo, hi) in t.items():
        res[k + "_us"] = round(med, 2)
        res[k + "_range"] = [round(lo, 2), round(hi, 2)]
    res["rot_fwd_fraction_of_8TBs"] = round((8 * n + mask + 24 * groups) / (t["rot_fwd"][0] * 1e-6) / PEAK, 4)
    res["rot_bwd_fraction_of_8TBs"] = round((8 * n + mask + 8 * groups) / (t["rot_bwd"][0] * 1e-6) / PEAK, 4)
    for d in ("fwd", "bwd"):
        res[d + "_old_over_rot"] = round(t["old_" + d][0] / t["rot_" + d][0], 2)
        res[d + "_rot_over_plain"] = round(t["rot_" + d][0] / t["plain_" + d][0], 2)
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
