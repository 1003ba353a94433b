"""Hadamard-rotated group-wise quantization on MI355X (csrc/k_rot.hip), bit for bit: the transform against
its matrix, the host loop and the numpy restatement; every fused kernel against the three-launch
composition hadamard -> group-wise kernel -> hadamard; the manager against the CPU; HIP-graph capture."""
import numpy as np
import pytest
import torch

import vsiquantization_amd as V
from tests import pg_common as P
from tests import rot_common as R
from tests.test_gpu_pg import _captured, _offset_view
from vsiquantization_amd.fakequant import (hadamard_transform, per_group_rot_fake_quant, per_group_rot_observe_fq,
                                           pg_rot_ste_backward)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("G", R.GROUPS)
def test_the_transform_of_the_identity_is_the_matrix(G):
    y = hadamard_transform(3.0 * torch.eye(G, device=DEV), G)
    assert np.array_equal(y.cpu().numpy(), (np.float32(3.0) * R.c_of(G) * R.sylvester(G)).astype(np.float32))


@pytest.mark.parametrize("rows,rowlen,G", R.CASES, ids=P.ids(R.CASES))
def test_transform_equals_host_loop_and_restatement(rows, rowlen, G):
    xc = R.inputs(rows, rowlen, rows + rowlen + G)
    want = torch.from_numpy(R.hadamard_np(xc.numpy(), G))
    assert P.same_bits(hadamard_transform(xc, G), want)
    assert P.same_bits(hadamard_transform(xc.to(DEV), G), want)
    assert P.same_bits(hadamard_transform(_offset_view(xc), G), want)     # the scalar path


def _check_fused(xc, G, symmetric, nbits, tag, x=None):
    """Both forwards, observe-only, a second call on carried state and the backward, every output."""
    rows, rowlen = xc.shape
    qmin, qmax = P.grid(symmetric, nbits)
    x = xc.to(DEV) if x is None else x
    g = (P.weights(rows, rowlen, 77) * 20).to(DEV)
    state = torch.zeros(2, 2, rows, rowlen // G, device=DEV)                       # [composed | fused][min | max]
    kw = dict(group_size=G, symmetric=symmetric, qmin=qmin, qmax=qmax)
    for call, xi in enumerate((x, x * 1.5)):                               # the second call: carried state
        want = R.composed(xi, G, symmetric, qmin, qmax, state[0, 0], state[0, 1])
        only = per_group_rot_observe_fq(xi, quantize=False, run_min=state[1, 0].clone(), run_max=state[1, 1].clone(),
                                        **kw)
        got = per_group_rot_observe_fq(xi, run_min=state[1, 0], run_max=state[1, 1], want_mask=True, want_codes=True,
                                       want_rotated=True, **kw)
        for k in ("y", "yr", "codes", "mask", "run_min", "run_max", "scale", "zp"):
            assert P.same_bits(got[k], want[k]), (tag, call, k)
        for k in ("run_min", "run_max", "scale", "zp"):
            assert P.same_bits(only[k], want[k]), (tag, call, "observe only", k)
    plain = per_group_rot_observe_fq(x * 1.5, run_min=state[1, 0].clone(), run_max=state[1, 1].clone(), **kw)
    assert P.same_bits(plain["y"], got["y"]), tag                         # the state already holds x * 1.5
    sc, zp = got["scale"] * 0.5, got["zp"] + 0.25                         # half the range: both ends clamp
    for zp_round in (False, True):
        want = R.composed_fixed(x, G, sc, zp, qmin, qmax, zp_round)
        y, mask, codes, yr = per_group_rot_fake_quant(x, sc, zp, qmin, qmax, group_size=G, zp_round=zp_round,
                                                      want_mask=True, want_codes=True, want_rotated=True)
        for k, v in (("y", y), ("yr", yr), ("codes", codes), ("mask", mask)):
            assert P.same_bits(v, want[k]), (tag, "fixed", zp_round, k)
    bits = P.unpack_mask(mask, rows, rowlen)
    assert bool(bits.any()) and not bool(bits.all()), tag                  # the backward sees both mask values
    assert P.same_bits(pg_rot_ste_backward(g, mask, sc, G), R.composed_backward(g, mask, sc, G)), tag


@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
@pytest.mark.parametrize("rows,rowlen,G", R.CASES, ids=P.ids(R.CASES))
def test_fused_kernels_equal_the_three_launch_composition(rows, rowlen, G, symmetric, nbits):
    xc = P.weights(rows, rowlen, rows + rowlen)
    _check_fused(xc, G, symmetric, nbits, (rows, rowlen, G, symmetric, nbits))
    if rows == 3:   # a view one element into a buffer: the scalar path
        _check_fused(xc, G, symmetric, nbits, ("offset", rows, rowlen, G, symmetric, nbits), x=_offset_view(xc))


@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
@pytest.mark.parametrize("G", R.GROUPS)
def test_special_groups_next_to_ordinary_ones(G, symmetric, nbits):
    xc = P.with_special_groups(P.weights(2, 9 * G, 11), G)
    _check_fused(xc, G, symmetric, nbits, ("special", G, symmetric, nbits))


@pytest.mark.parametrize("G", R.GROUPS)
def test_four_tasks_per_wave_from_the_grid_size_threshold_on(G):
    """Just above pg_per_wave's threshold (64 chunks per CU) at rowlen 512; the last workgroup is not full."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 64 * cus // 2 + 1
    _check_fused(P.weights(rows, 512, rows), G, False, 4, ("tasks per wave", G))


def test_manager_on_the_gpu_equals_the_cpu():
    """A fused layer's weight manager through calibrate, train and eval against a CPU manager fed the same weight."""
    import torch.nn as nn

    from vsiquantization_amd.modules.fused import LinearBnReLU
    torch.manual_seed(3)
    layer = LinearBnReLU(nn.Linear(256, 6), nn.BatchNorm1d(6), nn.ReLU(), "PerGroupMinMaxObserver",
                         "RotatedPerGroupQuantizer", "MinMaxObserver", "UniformQuantizer", True, True, True, 4, 8).to(DEV)
    wq, x = layer.weight_quantizer, torch.randn(4, 256, device=DEV)
    cpu = V.QuantizationManager("RotatedPerGroupQuantizer", "PerGroupMinMaxObserver", 4, True, False)
    wq.is_learning_scale = layer.activation_quantizer.is_learning_scale = False
    w, g = layer.get_weight_bias()[0].detach(), P.weights(6, 256, 5) * 30
    for quantize in (False, True):                                         # calibrate, then train
        wq.is_quantize = cpu.is_quantize = quantize
        layer(x).square().mean().backward()
        cpu.quantize(w.cpu())
        assert P.same_bits(wq.scale.cpu(), cpu.scale) and P.same_bits(wq.observer.run_max.cpu(), cpu.observer.run_max)
    assert bool(torch.isfinite(layer.linear_fuse.weight.grad).all()) and wq.scale.is_cuda
    layer.eval()
    wq.is_observer_qparam = cpu.is_observer_qparam = False                 # eval: the fixed rotated forward
    with torch.no_grad():
        layer(x)
    a, b = w.clone().requires_grad_(True), w.cpu().requires_grad_(True)
    ya, yb = wq.quantize(a), cpu.quantize(b)
    ya.backward(g.to(DEV))
    yb.backward(g)
    assert P.same_bits(ya.cpu(), yb) and P.same_bits(a.grad.cpu(), b.grad)


def test_graph_replay_equals_eager():
    rows, rowlen, G = 9, 576, 64
    x1, x2 = P.weights(rows, rowlen, 1).to(DEV), (P.weights(rows, rowlen, 20) * 2).to(DEV)
    g1, g2 = P.weights(rows, rowlen, 3).to(DEV), (P.weights(rows, rowlen, 4) * 30).to(DEV)
    kw = dict(group_size=G, symmetric=False, qmin=0, qmax=15, want_mask=True, want_codes=True, want_rotated=True)
    ref_mn, ref_mx = torch.zeros(rows, 9, device=DEV), torch.zeros(rows, 9, device=DEV)
    want = per_group_rot_observe_fq(x2, run_min=ref_mn, run_max=ref_mx, **kw)
    want_gx = pg_rot_ste_backward(g2, want["mask"], want["scale"], G)
    xs = x1.clone()
    state = torch.zeros(2, rows, 9, device=DEV)
    fwd = lambda: per_group_rot_observe_fq(xs, run_min=state[0], run_max=state[1], **kw)   # noqa: E731
    graph, got = _captured(fwd, fwd)
    xs.copy_(x2)
    for _ in range(2):
        state.zero_()
        graph.replay()
    torch.cuda.synchronize()
    for k in ("y", "yr", "scale", "zp", "codes", "mask"):
        assert P.same_bits(got[k], want[k]), k
    assert P.same_bits(state[0], ref_mn) and P.same_bits(state[1], ref_mx)
    # the backward in a capture of its own (never autograd.backward inside a capture)
    gs, mask, scale = g1.clone(), want["mask"].clone(), want["scale"].clone()
    bwd = lambda: pg_rot_ste_backward(gs, mask, scale, G)   # noqa: E731
    bgraph, gx = _captured(bwd, bwd)
    gs.copy_(g2)
    for _ in range(2):
        bgraph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(gx, want_gx)
