"""AdaRound on the GPU: k_adaround_fwd / k_adaround_bwd against the host loops (bit for
bit) and the numpy oracle of tests/adaround_common.py, at the seams of the (rows, chunks)
grid (2048 elements of one row per workgroup) and of the regulariser's fold (1, <= 128,
<= 2048 and more workgroups), then the edge inputs, the autograd Function, the module,
the export round trip, the layer driver and HIP-graph capture."""
import numpy as np
import pytest
import torch

from tests import adaround_common as A
from tests.test_adaround_cpu import (check_edges, check_end_to_end, check_function_gradient,
                                     check_init_and_round_trip)
from vsiquantization_amd.fakequant import adaround_backward, adaround_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("tag,rows,rowlen,per_row", A.all_cases())
def test_device_against_host(tag, rows, rowlen, per_row):
    """y (soft and hard) and grad_V with lambda = 0 bit for bit, every grid."""
    for k, (bits, sym) in enumerate(A.GRIDS):
        w, Vv, g, sc, zp, lo, hi = A.make_case(rows, rowlen, bits, sym, per_row, seed=31 * k + rowlen)
        for hard in (False, True):
            yd, _ = A.run(w, Vv, sc, zp, lo, hi, per_row, DEV, hard=hard)
            yh, _ = A.run(w, Vv, sc, zp, lo, hi, per_row, hard=hard)
            assert A.bits_equal(yd, yh), (tag, bits, sym, hard)
        gd = A.run_bwd(g, w, Vv, sc, zp, lo, hi, per_row, DEV, lam=0.0, beta=2.0)
        gh = A.run_bwd(g, w, Vv, sc, zp, lo, hi, per_row, lam=0.0, beta=2.0)
        assert A.bits_equal(gd, gh), (tag, bits, sym)


def test_unaligned_views():
    """Tensors whose storage is not 16-byte aligned take the per-element path: same bits."""
    w, Vv, g, sc, zp, lo, hi = A.make_case(8, 64, 4, False, True, seed=3)
    pad = lambda a: torch.cat([torch.zeros(1), torch.from_numpy(a).reshape(-1)]).to(DEV)[1:].reshape(a.shape)  # noqa: E731
    s, z = torch.from_numpy(sc), torch.from_numpy(zp)
    yd, _ = adaround_forward(pad(w), pad(Vv), s, z, lo, hi, axis=0)
    assert yd.data_ptr() % 16 == 0 and pad(w).data_ptr() % 16 == 4
    assert A.bits_equal(yd, A.run(w, Vv, sc, zp, lo, hi, True)[0])
    gd = adaround_backward(pad(g), pad(w), pad(Vv), s, z, lo, hi, axis=0, lam=0.0)
    assert A.bits_equal(gd, A.run_bwd(g, w, Vv, sc, zp, lo, hi, True, lam=0.0, beta=2.0))


@pytest.mark.parametrize("beta", A.BETAS)
def test_regulariser(beta):
    """grad_V with lambda != 0 within 1 fp32 ulp of the oracle (device and libm f64 pow may
    differ in the last f64 bit); R within 1e-9 relative (the project's bar for f64 sums)."""
    cases = [(1, n, False) for n in A.N_FLAT] + [(r, c, True) for r, c in A.SHAPES_PC + A.SHAPES_FOLD]
    for rows, rowlen, per_row in cases:
        w, Vv, g, sc, zp, lo, hi = A.make_case(rows, rowlen, 4, False, per_row, seed=rowlen + 1)
        h = A.lib_h(Vv)
        yd, R = A.run(w, Vv, sc, zp, lo, hi, per_row, DEV, beta=beta)
        Ro = A.oracle_reg(h, beta)
        print(rows, rowlen, beta, "R", float(R), Ro)
        assert abs(float(R) - Ro) <= 1e-9 * abs(Ro)
        assert A.bits_equal(yd, A.run(w, Vv, sc, zp, lo, hi, per_row)[0])   # y is the same with R asked
        _, R2 = A.run(w, Vv, sc, zp, lo, hi, per_row, DEV, beta=beta, want_y=False)
        _, R3 = A.run(w, Vv, sc, zp, lo, hi, per_row, DEV, beta=beta)
        assert float(R2) == float(R) == float(R3)   # fixed summation order; the counter was left at 0
        gd = A.run_bwd(g, w, Vv, sc, zp, lo, hi, per_row, DEV, lam=0.01, beta=beta).cpu().numpy()
        go = A.oracle_grad(g, w, Vv, sc, zp, lo, hi, 0.01, beta, h=h)
        d = A.ulp_distance(gd, go).max()
        print("max ulp", d)
        assert d <= 1


def test_edges():
    check_edges(DEV)


def test_function_gradient():
    check_function_gradient(DEV)


def test_init_and_round_trip():
    check_init_and_round_trip(DEV)


def test_end_to_end():
    check_end_to_end(DEV)


def test_graph_capture():
    """One forward (with R) and one backward captured on [64, 27], replayed twice: the
    outputs equal the eager ones bit for bit."""
    w, Vv, g, sc, zp, lo, hi = A.make_case(64, 27, 4, False, True, seed=9)
    wd, vd, gd_ = (torch.from_numpy(a).to(DEV) for a in (w, Vv, g))
    s, z = torch.from_numpy(sc).to(DEV), torch.from_numpy(zp).to(DEV)
    ye, Re = adaround_forward(wd, vd, s, z, lo, hi, axis=0, beta=3.7)
    ge = adaround_backward(gd_, wd, vd, s, z, lo, hi, axis=0, lam=0.01, beta=3.7)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up on the capture stream, as torch.cuda.graph asks
        adaround_forward(wd, vd, s, z, lo, hi, axis=0, beta=3.7)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yc, Rc = adaround_forward(wd, vd, s, z, lo, hi, axis=0, beta=3.7)
        gc = adaround_backward(gd_, wd, vd, s, z, lo, hi, axis=0, lam=0.01, beta=3.7)
    for _ in range(2):
        yc.zero_(); gc.zero_(); Rc.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert A.bits_equal(yc, ye) and A.bits_equal(gc, ge) and float(Rc) == float(Re)


def test_errors():
    w = torch.zeros(4, 8, device=DEV)
    for bad in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match=str(bad)):
            adaround_forward(w.to(bad), w, 0.1, 0, -8, 7)
        with pytest.raises(TypeError, match=str(bad)):
            adaround_backward(w, w, w.to(bad), 0.1, 0, -8, 7)
    with pytest.raises(ValueError, match="like w"):
        adaround_forward(w, torch.zeros(4, 9, device=DEV), 0.1, 0, -8, 7)
    with pytest.raises(ValueError, match="is on cpu, w on cuda"):
        adaround_forward(w, torch.zeros(4, 8), 0.1, 0, -8, 7)
    with pytest.raises(RuntimeError, match="per-channel scale has 3 entries, the tensor has 4 channels"):
        adaround_forward(w, w, torch.ones(3), None, -8, 7, axis=0)
    layer, x = A.build_layer(0, DEV)
    layer.weight_quantizer.scale = 1
    import vsiquantization_amd as V
    with pytest.raises(RuntimeError, match="neither observed nor learned"):
        V.adaround_layer(layer, x, iters=1)
