"""MSEObserver's per-call cost at 3.3M and 52M elements, K = 64 candidates, 4-bit symmetric
grid, with no activation and with ReLU fused:

  * K2     fakequant.observe_tensor (one read, the running update),
  * mse    the search launch alone (vsiq_act_observe_mse_f32 on a given record),
  * eager  the torch loop it replaces, on the GPU: per candidate divide, add, round, clamp,
           dequantize and an f64 squared-error sum (K passes with their temporaries),

timed by HIP events around R repetitions, the variants alternated.  The search is VALU-bound:
beside the times the script prints the element-candidates per second and the fraction of the
VALU issue rate that is (VALU_PER_EC instructions per element-candidate, counted in the
kernel's hot loop for gfx950, against 256 CUs x 4 SIMDs x 16 lanes x the shader clock).
DESIGN.md §5.1 holds the numbers.  usage: python tools/exp/mse_bench.py [reps]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vsiquantization_amd import _hip as H  # noqa: E402
from vsiquantization_amd.fakequant import mse_ratios, observe_tensor, qden  # noqa: E402

SIZES = (3_276_800, 52_428_800)
K, BITS = 64, 4
QMIN, QMAX = -8, 7
VALU_PER_EC = 17.8            # 571 VALU instructions per 32 element-candidates (hot loop, fast path)
LANE_RATE = 256 * 4 * 16 * 2.4e9   # lane-instructions per second at 2.4 GHz


def eager_search(v, ratios):
    """The loop a toolkit writes in eager torch (range from the tensor, symmetric grid)."""
    m = v.abs().max()
    best, pick = None, 0
    for k, r in enumerate(ratios):
        s = m * r / (QMAX + 1e-8)
        y = torch.clamp(torch.round(v / s), QMIN, QMAX) * s
        e = (y.double() - v.double()).square().sum()
        if best is None:
            best = e
        else:
            better = e < best
            best = torch.where(better, e, best)
            pick = torch.where(better, k, pick)
    return best, pick


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    dev = torch.device("cuda:0")
    lib = H.lib()
    gen = torch.Generator(device=dev).manual_seed(7)
    ratios = mse_ratios(K)
    table = (H.c_d * K)(*ratios)
    print(f"{'elements':>10s} {'act':>5s} {'K2 us':>8s} {'mse us':>9s} {'x K2':>6s} {'eager us':>10s} {'eager/mse':>9s} "
          f"{'Gec/s':>8s} {'VALU frac':>9s} {'pick':>4s}")
    for n in SIZES:
        x = torch.randn(n, device=dev, generator=gen) * 3
        for act, code in ((None, H.ACT_NONE), ("relu", H.ACT_RELU)):
            state = torch.zeros(2, dtype=torch.float32, device=dev)
            qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=dev)
            clip = torch.empty(2, dtype=torch.float64, device=dev)
            err = torch.empty(K, dtype=torch.float64, device=dev)
            pick = torch.empty(1, dtype=torch.int32, device=dev)
            _, st = observe_tensor(x, symmetric=True, num_bits=BITS, want_qp=False, act=act)
            w = H.workspace(dev, n)
            w.reserve_doubles(int(lib.vsiq_observe_mse_ws_doubles(H.c_i64(n), K)))
            stream = H.stream_of(dev)
            v = torch.relu(x) if act else x

            def k2():
                observe_tensor(x, symmetric=True, num_bits=BITS, run_minmax=state, act=act)

            def mse():
                rc = lib.vsiq_act_observe_mse_f32(H.ptr(x), H.c_i64(n), code, H.ptr(st), table, K, QMIN, QMAX,
                                                  H.ptr(w.ws), H.c_i64(w.ws_len), H.ptr(w.counter), H.ptr(state),
                                                  H.ptr(qp), H.ptr(clip), H.ptr(err), H.ptr(pick), 1,
                                                  qden(True, BITS, 1e-8), 1e-8, stream)
                assert rc == 0

            def eager():
                eager_search(v, ratios)

            fns = ((k2, reps * 5), (mse, reps), (eager, max(2, reps // 10)))
            for f, _ in fns:
                for _ in range(2):
                    f()
            total, count = [0.0, 0.0, 0.0], [0, 0, 0]
            rounds = 2   # alternate the variants: drift of the shared machine hits all alike
            for _ in range(rounds):
                for i, (f, r) in enumerate(fns):
                    e0, e1 = bench.HipEvent(), bench.HipEvent()
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(max(1, r // rounds)):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    total[i] += e0.elapsed_time(e1) * 1e3
                    count[i] += max(1, r // rounds)
            t_k2, t_mse, t_eager = (t / c for t, c in zip(total, count))
            ecs = n * K / (t_mse * 1e-6)
            print(f"{n:10d} {str(act):>5s} {t_k2:8.1f} {t_mse:9.1f} {t_mse / t_k2:6.1f} {t_eager:10.1f} "
                  f"{t_eager / t_mse:9.1f} {ecs / 1e9:8.1f} {ecs * VALU_PER_EC / LANE_RATE:9.3f} {int(pick):4d}",
                  flush=True)
            assert int(w.counter.ne(0).sum()) == 0


if __name__ == "__main__":
    main()
