"""Time the per-group MSE search (csrc/k_pg_mse.hip) against the only route there was before it
and against the floor it sits on.

    python tools/bench_per_group_mse.py [--reps 50] [--rounds 7] [--out FILE]

For each shape ([1024, 9216] and [256, 1152]) and group size (32, 128), 64 candidates, 4-bit
symmetric, no error table requested, three routes take turns:

  new     per_group_observe_mse(x, group_size=G)                 one launch of k_pg_mse.hip
  old     per_channel_observe_mse(x.view(-1, G))                 k_pc_mse.hip, one wave per G-element "row"
  floor   per_group_observe_fq(x, group_size=G)                  plain min / max: what the search costs on top

Each measurement is a batch of `reps` back-to-back calls between two HIP events (mean per call),
after a warm-up batch; the routes alternate for `rounds` rounds and the median, minimum and
maximum over the rounds are reported in microseconds.  "new_faster_than_old" is true only where
the new route's maximum over the rounds is below the old route's minimum; the ratio of medians
is printed either way.  All output and state buffers are allocated by the calls themselves, as
a user's are (the old route always allocates and writes its [rows, 64] error table: it has no
way not to).  One JSON line per (shape, G).  Reads nothing outside the repository."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_per_group import alternate  # noqa: E402
from vsiquantization_amd.fakequant import (mse_ratios, per_channel_observe_mse, per_group_observe_fq,  # noqa: E402
                                           per_group_observe_mse)

SHAPES = ((1024, 9216), (256, 1152))
GROUPS = (32, 128)


def bench(rows, rowlen, G, reps, rounds, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((rows, rowlen), device=dev, generator=gen) * 0.05
    xv = x.view(-1, G)
    ratios = mse_ratios(64)
    kw = dict(symmetric=True, qmin=-8, qmax=7, num_bits=4, ratios=ratios)
    new = per_group_observe_mse(x, group_size=G, **kw)
    old = per_channel_observe_mse(xv, **kw)
    assert torch.equal(new["y"].view(-1, G), old["y"]) and torch.equal(new["scale"].view(-1), old["scale"])
    assert torch.equal(new["pick"].view(-1), old["pick"]) and bool(new["pick"].any())
    t = alternate({
        "new": lambda: per_group_observe_mse(x, group_size=G, **kw),
        "old": lambda: per_channel_observe_mse(xv, **kw),
        "floor": lambda: per_group_observe_fq(x, group_size=G, symmetric=True, qmin=-8, qmax=7, obs_bits=4),
    }, reps, rounds)
    res = {"shape": [rows, rowlen], "G": G, "candidates": len(ratios), "reps": reps, "rounds": rounds}
    for k, (med, lo, hi) in t.items():
        res[k + "_us"] = round(med, 2)
        res[k + "_range"] = [round(lo, 2), round(hi, 2)]
    res["old_over_new"] = round(t["old"][0] / t["new"][0], 2)
    res["new_over_floor"] = round(t["new"][0] / t["floor"][0], 2)
    res["new_faster_than_old"] = bool(t["new"][2] < t["old"][1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
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
