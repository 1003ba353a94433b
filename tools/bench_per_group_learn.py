"""Time the learnable group-wise route (csrc/k_pg.hip k_pg_lsq_bwd) against the only route there
was before it.

    python tools/bench_per_group_learn.py [--reps 200] [--rounds 7] [--out FILE]

For each shape ([1024, 9216] and [256, 1152]) and group size (32, 128), symmetric int4 with a
learned scale (zp_learn 0) and asymmetric uint4 with a learned zero point too (zp_learn 1):

  new   per_group_fake_quant(x, s, z, zp_round)  then  pg_lsq_backward(g, x, s, z)      one launch each
  old   per_channel_fake_quant(x.view(-1, G), ...)  then  pc_lsq_backward(...)  (K6: workspace + counters)

"step" is the forward followed by the backward, "bwd" the backward alone, and "ste" the group-wise
STE backward (pg_ste_backward) for comparison.  Each measurement is a batch of `reps` back-to-back
calls between two HIP events (mean per call), after a warm-up batch; the routes alternate for
`rounds` rounds and the median, minimum and maximum over the rounds are reported in microseconds,
so the spread of each route is next to the difference between them.  All output buffers are
allocated by the calls themselves, as a user's are.  Algorithmic bytes: the learnable backward
12 B / element (g and x in, gx out) + 32 B / group (scale and zp in, both gradients out); the STE
backward 8 B / element + 1 bit / element of mask + 8 B / group; each reported over the median time
as a fraction of 8 TB/s.  One JSON line per (shape, G, zp_learn).  Reads nothing outside the
repository."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vsiquantization_amd import _hip as H  # noqa: E402
from vsiquantization_amd.fakequant import (pc_lsq_backward, per_channel_fake_quant, per_group_fake_quant,  # noqa: E402
                                           per_group_observe_fq, pg_lsq_backward, pg_ste_backward)

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


def bench(rows, rowlen, G, learn_zp, reps, rounds, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((rows, rowlen), device=dev, generator=gen) * 0.05
    g = torch.randn((rows, rowlen), device=dev, generator=gen)
    xv, gv = x.view(-1, G), g.view(-1, G)
    sym = not learn_zp
    qmin, qmax = (-8, 7) if sym else (0, 15)
    obs = per_group_observe_fq(x, group_size=G, symmetric=sym, qmin=qmin, qmax=qmax, obs_bits=4, want_mask=True)
    s = obs["scale"] * 0.8                      # a learned scale below the observed one: the clamp cuts
    z = obs["zp"] + (0.3 if learn_zp else 0.0)
    sv, zv = s.view(-1), z.view(-1)
    gscale = (qmax * G) ** -0.5

    def new_step():
        per_group_fake_quant(x, s, z, qmin, qmax, group_size=G, zp_round=learn_zp)
        return pg_lsq_backward(g, x, s, z, qmin, qmax, gscale, learn_zp, G)

    def old_step():
        per_channel_fake_quant(xv, sv, zv, qmin, qmax, zp_round=learn_zp)
        return pc_lsq_backward(gv, xv, sv, zv, qmin, qmax, gscale, learn_zp)

    a, b = new_step(), old_step()
    assert torch.equal(a[0].view(-1, G), b[0])
    assert torch.allclose(a[1].view(-1), b[1], rtol=1e-6, atol=1e-9) and torch.allclose(a[2].view(-1), b[2],
                                                                                           rtol=1e-6, atol=1e-9)
    t = alternate({
        "new_step": new_step,
        "old_step": old_step,
        "new_bwd": lambda: pg_lsq_backward(g, x, s, z, qmin, qmax, gscale, learn_zp, G),
        "old_bwd": lambda: pc_lsq_backward(gv, xv, sv, zv, qmin, qmax, gscale, learn_zp),
        "ste_bwd": lambda: pg_ste_backward(g, obs["mask"], s, G),
    }, reps, rounds)
    n, groups = rows * rowlen, rows * (rowlen // G)
    mask = 8 * int(H.lib().vsiq_mask_words(rows, rowlen))
    res = {"shape": [rows, rowlen], "G": G, "zp_learn": int(learn_zp), "reps": reps, "rounds": rounds}
    for k, (med, lo, hi) in t.items():
        res[k + "_us"] = round(med, 2)
        res[k + "_range"] = [round(lo, 2), round(hi, 2)]
    res["new_bwd_fraction_of_8TBs"] = round((12 * n + 32 * groups) / (t["new_bwd"][0] * 1e-6) / PEAK, 4)
    res["ste_bwd_fraction_of_8TBs"] = round((8 * n + mask + 8 * groups) / (t["ste_bwd"][0] * 1e-6) / PEAK, 4)
    res["step_old_over_new"] = round(t["old_step"][0] / t["new_step"][0], 2)
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
            for learn_zp in (False, True):
                lines.append(json.dumps(bench(rows, rowlen, G, learn_zp, a.reps, a.rounds, "cuda:0")))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
