"""PercentileObserver's per-call cost on the C5 layer sizes (1.6M, 6.6M, 26M, 52M elements)
against the MinMaxObserver call it extends:

  * K2         fakequant.observe_tensor (one read, the running update),
  * percentile fakequant.observe_percentile (K2, then the histogram pass),
  * hist       the histogram launch alone (vsiq_act_observe_hist_f32 on a given record),

on randn, post-ReLU (about half the elements in bin 0) and outlier-stretched data (ten
planted +-1e4 values: nearly every element in a few bins).  Call time by HIP events around R
repetitions through the public API (host launch cost included: two launches against one),
the variants alternated; the histogram pass's algorithmic bytes are 4 B per element.
DESIGN.md §5.1 holds the numbers.  usage: python tools/exp/percentile_bench.py [reps]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vsiquantization_amd import _hip as H  # noqa: E402
from vsiquantization_amd.fakequant import observe_percentile, observe_tensor, qden  # noqa: E402

SIZES = (1_638_400, 6_553_600, 26_214_400, 52_428_800)
TAIL, BINS = 1e-4, 2048   # the observer's defaults: percentile 99.99, 2048 bins


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    dev = torch.device("cuda:0")
    lib = H.lib()
    gen = torch.Generator(device=dev).manual_seed(7)
    print(f"{'elements':>10s} {'data':>9s} {'K2 us':>8s} {'pct us':>8s} {'ratio':>6s} {'hist us':>8s} "
          f"{'hist GB/s':>10s} {'of 8 TB/s':>9s}")
    for n in SIZES:
        base = torch.randn(n, device=dev, generator=gen) * 3
        stretched = base.clone()
        stretched[torch.randperm(n, device=dev, generator=gen)[:10]] = 1e4
        stretched[torch.randperm(n, device=dev, generator=gen)[:10]] = -1e4
        for name, x in (("randn", base), ("post-relu", torch.relu(base)), ("outliers", stretched)):
            state = torch.zeros(2, dtype=torch.float32, device=dev)
            qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=dev)
            clip = torch.empty(2, dtype=torch.float64, device=dev)
            _, st = observe_tensor(x, symmetric=True, want_qp=False)
            w = H.workspace(dev, n)
            hist = w.histogram()
            stream = H.stream_of(dev)

            def k2():
                observe_tensor(x, symmetric=True, run_minmax=state)

            def pct():
                observe_percentile(x, symmetric=True, run_minmax=state, tail=TAIL, bins=BINS)

            def hist_only():
                rc = lib.vsiq_act_observe_hist_f32(H.ptr(x), H.c_i64(n), 0, H.ptr(st), BINS, TAIL, H.ptr(hist),
                                                   H.c_i64(hist.numel()), H.ptr(w.counter), H.ptr(state), H.ptr(qp),
                                                   H.ptr(clip), 1, qden(True, 8, 1e-8), 1e-8, stream)
                assert rc == 0

            fns = (k2, pct, hist_only)
            for f in fns:
                for _ in range(5):
                    f()
            total = [0.0, 0.0, 0.0]
            rounds = 4   # alternate the variants: drift of the shared machine hits all alike
            for _ in range(rounds):
                for i, f in enumerate(fns):
                    e0, e1 = bench.HipEvent(), bench.HipEvent()
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(reps // rounds):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    total[i] += e0.elapsed_time(e1) * 1e3
            t_k2, t_pct, t_hist = (t / (reps // rounds * rounds) for t in total)
            gbs = 4 * n / t_hist / 1e3
            print(f"{n:10d} {name:>9s} {t_k2:8.1f} {t_pct:8.1f} {t_pct / t_k2:6.2f} {t_hist:8.1f} {gbs:10.1f} "
                  f"{gbs / 8000:9.3f}", flush=True)
            assert int(hist.ne(0).sum()) == 0 and int(w.counter.ne(0).sum()) == 0


if __name__ == "__main__":
    main()
