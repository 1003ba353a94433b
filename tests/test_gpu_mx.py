"""MX fake quantization on MI355X (csrc/k_mx.hip) against the numpy restatement of tests/mx_common.py and the
host loops, bit for bit; the backward from the 1-bit mask; the Python layers; HIP-graph capture last."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests import mx_common as M
from tests import pg_common as P
from tests.test_gpu_pg import _captured
from vsiquantization_amd import fakequant as FQ
from vsiquantization_amd.modules.fuse import fuse_modules_unified
from vsiquantization_amd.modules.fuse_config import FuseConfig, FuseConfigManager

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# beyond M.ROW_SHAPES (LDS path): 8-lane blocks + tail chunk; rows sharing waves; blocks crossing waves
ROW_EXTRA = [(3, 2080), (40, 96), (2, 8196)]
# beyond M.COL_SHAPES (per-element path): vector path, short channel block, two chunks; two workgroups
COL_EXTRA = [(2, 40, 300), (1, 64, 1028)]


def _unpack(mask, view):
    if mask.dtype == torch.uint8:
        return mask.cpu().numpy().reshape(view)
    return P.unpack_mask(mask, *FQ._mx_mask_view(view)).numpy().astype(np.uint8).reshape(view)


def _run(xt, fmt, axis):
    y, codes, scales, mask = FQ._mx_forward(xt, fmt, axis, True, True)
    return M.bits(y.cpu().numpy()), codes.cpu().numpy(), scales.cpu().numpy(), _unpack(mask, tuple(xt.shape))


def _check(x, fmt, axis, what, xt=None):
    ry, rc, rs, rm = (M.ref_rows if axis == -1 else M.ref_cols)(x, fmt)
    xt = torch.from_numpy(x).to(DEV) if xt is None else xt
    got, host = _run(xt, fmt, axis), _run(torch.from_numpy(x), fmt, axis)
    for name, g, r, h in zip(("y", "codes", "scales", "mask"), got, (M.bits(ry), rc, rs, rm), host):
        assert np.array_equal(g, r), (what, name, "restatement")
        assert np.array_equal(g, h), (what, name, "host")
    plain = FQ._mx_forward(xt, fmt, axis, False, False)[0]
    assert np.array_equal(M.bits(plain.cpu().numpy()), got[0]), (what, "plain")


@pytest.mark.parametrize("fmt", M.NAMES)
def test_rows_equal_the_restatement_and_the_host_loops(fmt):
    _check(M.builder(fmt), fmt, -1, "builder")
    _check(M.special_blocks(), fmt, -1, "special")   # a block of fp32 denormals: no flush to zero
    _check(M.ragged_rows(), fmt, -1, "ragged")
    for i, shape in enumerate(M.ROW_SHAPES + ROW_EXTRA):
        _check(M.fill(shape, fmt), fmt, -1, ("fill", shape))
        _check(M.gaussian(shape, i), fmt, -1, ("gaussian", shape))
    x = M.gaussian((5, 96), 21)                      # one element into a buffer: the per-element path
    buf = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    xt = buf[1:].view(x.shape)
    xt.copy_(torch.from_numpy(x))
    assert xt.data_ptr() % 16 != 0 and xt.is_contiguous()
    _check(x, fmt, -1, "offset view", xt=xt)


def test_four_chunks_per_wave_from_the_grid_size_threshold_on():
    # from 64 chunks of 256 per CU on a wave takes 4 chunks: the smallest such tensor, against the host loops
    rows = -(-64 * torch.cuda.get_device_properties(0).multi_processor_count * 256 // 1056) + 1
    x = torch.from_numpy(M.gaussian((rows, 1056), 5))
    for g, h in zip(_run(x.to(DEV), "fp6_e3m2", -1), _run(x, "fp6_e3m2", -1)):
        assert np.array_equal(g, h)


@pytest.mark.parametrize("fmt", M.NAMES)
def test_columns_equal_the_restatement_and_the_host_loops(fmt):
    for blocks in (M.builder(fmt), M.special_blocks()):
        _check(np.ascontiguousarray(blocks.T)[None], fmt, 1, "blocks as columns")   # [1, 32, blocks]
    for i, shape in enumerate(M.COL_SHAPES + COL_EXTRA):
        _check(M.fill(shape, fmt), fmt, 1, ("fill", shape))
        _check(M.gaussian(shape, i), fmt, 1, ("gaussian", shape))


@pytest.mark.parametrize("shape,axis", [((3, 100), -1), ((4, 64), -1), ((2, 40, 7), 1)])
def test_autograd_is_the_straight_through_mask(shape, axis):
    x = M.gaussian(shape, 11)
    g = torch.from_numpy(np.random.default_rng(12).standard_normal(shape).astype(np.float32))
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    V.mx_fake_quant(xt, "fp4_e2m1", axis=axis).backward(g.to(DEV))
    x2 = x.reshape(-1, shape[-1]) if axis == -1 else x
    mask = (M.ref_rows if axis == -1 else M.ref_cols)(x2, "fp4_e2m1")[3].reshape(shape)
    assert (mask == 0).any() and (mask == 1).any()
    want = np.where(mask == 1, g.numpy(), np.float32(0))
    assert np.array_equal(M.bits(xt.grad.cpu().numpy()), M.bits(want))


def test_manager_layouts_and_a_fused_layer_on_cuda():
    cpu = V.QuantizationManager("MXQuantizer", "MinMaxObserver", 4, True, is_learning_scale=False)
    dev = V.QuantizationManager("MXQuantizer", "MinMaxObserver", 4, True, is_learning_scale=False)
    xc = torch.from_numpy(M.gaussian((5, 100), 2))
    x, y = xc.to(DEV), dev.quantize(xc.to(DEV))
    assert y.device == x.device and P.same_bits(y.cpu(), cpu.quantize(xc))
    assert P.same_bits(dev.quantize(x, act="relu").cpu(), cpu.quantize(xc, act="relu"))
    (codes, scales, fmt), want = dev.export_mx(x), cpu.export_mx(xc)
    assert torch.equal(codes.cpu(), want[0]) and torch.equal(scales.cpu(), want[1]) and fmt == want[2]
    assert P.same_bits(V.mx_dequant(codes, scales, fmt), y)
    a =torch.from_numpy(M.gaussian((2, 40, 6, 5), 3)).to(DEV)
    ya = V.mx_fake_quant(a, "fp6_e3m2", axis=1)
    assert P.same_bits(ya.cpu(), V.mx_fake_quant(a.cpu(), "fp6_e3m2", axis=1))
    cl = a.contiguous(memory_format=torch.channels_last)   # NHWC memory: the row kernel
    ycl, ccl, scl = V.mx_fake_quant(cl, "fp6_e3m2", axis=1, want_codes=True)
    assert ycl.is_contiguous(memory_format=torch.channels_last) and P.same_bits(ycl, ya)
    assert P.same_bits(V.mx_dequant(ccl, scl, "fp6_e3m2", axis=1), ya)
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(3, 40, 3, padding=1, bias=False), nn.BatchNorm2d(40), nn.ReLU())
    cfg = FuseConfig(quantizer_w_name="MXQuantizer", quantizer_a_name="MXQuantizer", bits_w=4, bits_a=8)
    model = fuse_modules_unified(model, [("conv", "bn", "relu")], config_manager=FuseConfigManager(cfg)).to(DEV)
    layer = model[0]
    xin = torch.randn(2, 3, 8, 8, device=DEV)
    out = model(xin)
    w, b = layer.get_weight_bias()
    wq = V.mx_fake_quant(w.detach(), "fp4_e2m1")
    assert P.same_bits(wq.cpu(), V.mx_fake_quant(w.detach().cpu(), "fp4_e2m1"))
    pre = torch.relu(layer._pre_act(xin, wq, b)).detach()
    assert P.same_bits(out.detach(), V.mx_fake_quant(pre, "fp8_e4m3", axis=1))
    assert P.same_bits(out.detach().cpu(), V.mx_fake_quant(pre.cpu(), "fp8_e4m3", axis=1))
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    before = layer.conv_fuse.weight.detach().clone()
    out.square().mean().backward()
    assert layer.conv_fuse.weight.grad is not None and torch.isfinite(layer.conv_fuse.weight.grad).all()
    opt.step()
    assert not torch.equal(layer.conv_fuse.weight.detach(), before)


def test_refusals():
    x = torch.zeros(4, 64, device=DEV)
    with pytest.raises(TypeError):
        V.mx_fake_quant(x.bfloat16(), "fp4_e2m1")
    with pytest.raises(NotImplementedError):
        V.mx_fake_quant(x, "fp4_e2m1", axis=0)


def test_graph_replay_equals_eager():
    # last in the file; forward and backward function in captures of their own, never autograd.backward inside one
    shape = (9, 576)
    x1, x2 = (torch.from_numpy(M.gaussian(shape, s)).to(DEV) for s in (1, 2))
    g1, g2 = (P.weights(*shape, s).to(DEV) for s in (3, 4))
    want = FQ._mx_forward(x2, "fp4_e2m1", -1, True, True)
    want_gx = FQ.ste_backward(g2, want[3], 1.0, 0)

    xs = x1.clone()
    fwd = lambda: FQ._mx_forward(xs, "fp4_e2m1", -1, True, True)   # noqa: E731
    graph, got = _captured(fwd, fwd)
    xs.copy_(x2)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert P.same_bits(g, w)

    gs, mask = g1.clone(), want[3].clone()
    bwd = lambda: FQ.ste_backward(gs, mask, 1.0, 0)   # noqa: E731
    bgraph, gx = _captured(bwd, bwd)
    gs.copy_(g2)
    for _ in range(2):
        bgraph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(gx, want_gx)
