"""Hadamard-rotated MX fake quantization on MI355X (csrc/k_mx_rot.hip), bit for bit: every output of the
fused kernels against the numpy restatement hadamard_np(ref(hadamard_np(x))) and against the on-device
three-call composition hadamard_transform -> mx_fake_quant -> hadamard_transform; the backward; the
module path; HIP-graph capture last."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests import mx_common as M
from tests import pg_common as P
from tests import rot_common as R
from tests.test_gpu_pg import _captured, _offset_view
from vsiquantization_amd import fakequant as FQ
from vsiquantization_amd.modules.fuse import fuse_modules_unified
from vsiquantization_amd.modules.fuse_config import FuseConfig, FuseConfigManager
from vsiquantization_amd.modules.fused import LinearBnReLU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# one block, the rest of the wave padding; short rows sharing a wave; one chunk per row; chunks that
# straddle rows with a partial last chunk
ROWS = [(1, 32), (3, 32), (2, 256), (3, 288)]
# one lane; inner % 4 != 0 (per-element arm); a second, partial inner chunk; two channel blocks
COLS = [(1, 32, 1), (2, 64, 7), (1, 32, 260), (2, 96, 8)]


def _cases(shapes):
    """All five formats on the two smallest shapes, fp4_e2m1 and fp8_e4m3 on the rest."""
    return [(s, f) for i, s in enumerate(shapes) for f in (M.NAMES if i < 2 else ("fp4_e2m1", "fp8_e4m3"))]


def _inputs(shape):
    """rot_common's per-element powers of two, and mx_common's special blocks tiled into the shape
    (blocks along the last axis: the column form gets them transposed onto its channel axis)."""
    n = int(np.prod(shape))
    yield "powers of two", R.inputs(1, n, n).numpy().reshape(shape)
    yield "special", np.resize(M.special_blocks().reshape(-1), shape).astype(np.float32)


def _to_rows(a, cols):
    """Blocks as consecutive runs of 32: the tensor itself, or [outer, inner, channels] of the column form."""
    return a.transpose(1, 2).contiguous() if cols else a


def _reference(x, fmt):
    """numpy, x with its blocks along the last axis: (y, yr, codes, scales, mask)."""
    with np.errstate(all="ignore"):   # 3e38 blocks overflow in the transform, as on the device
        r = R.hadamard_np(x.reshape(-1, x.shape[-1]), 32)
        yr, codes, scales, mask = M.ref_rows(r, fmt)
        y = R.hadamard_np(yr, 32)
    return tuple(t.reshape(x.shape[:-1] + (-1,)) for t in (y, yr, codes, scales, mask))


def _composed(x, fmt, cols):
    """The three existing device calls (and, for the column form, the two transposing copies)."""
    yr, codes, scales, mask = FQ._mx_forward(FQ.hadamard_transform(_to_rows(x, cols), 32), fmt, -1, True, True)
    mask = P.unpack_mask(mask, 1, yr.numel()).reshape(yr.shape)
    return tuple(_to_rows(t, cols).contiguous() for t in (FQ.hadamard_transform(yr, 32), yr, codes, scales, mask))


def _fused(x, fmt, cols):
    y, yr, codes, scales, mask = FQ._mx_rot_forward(x, fmt, 1 if cols else -1, True, True, want_rotated=True)
    view = FQ._mx_rot_view(x.shape, 1 if cols else -1)[0]
    return y, yr, codes, scales, P.unpack_mask(mask, *FQ._mx_mask_view(view)).reshape(x.shape)


def _check(xn, fmt, cols, tag, x=None, restatement=True):
    x = torch.from_numpy(xn).to(DEV) if x is None else x
    got, want = _fused(x, fmt, cols), _composed(x, fmt, cols)
    names = ("y", "yr", "codes", "scales", "mask")
    for name, g, w in zip(names, got, want):
        assert P.same_bits(g.cpu(), w.cpu()), (tag, name, "composition")
    plain = FQ._mx_rot_forward(x, fmt, 1 if cols else -1, False, False)[0]   # the arm without codes and mask
    assert P.same_bits(plain, got[0]), (tag, "plain")
    if not restatement:
        return
    xr = np.ascontiguousarray(xn.transpose(0, 2, 1)) if cols else xn
    for name, g, r in zip(names, got, _reference(xr, fmt)):
        g = _to_rows(g, cols).cpu().numpy()
        same = np.array_equal(M.bits(g), M.bits(r)) if r.dtype == np.float32 else np.array_equal(g, r.astype(g.dtype))
        assert same, (tag, name, "restatement")
    deq = V.mx_dequant(got[2].cpu(), got[3].cpu(), fmt, axis=1 if cols else -1)
    assert P.same_bits(deq, got[1].cpu()), (tag, "mx_dequant(codes, scales) is yr")


@pytest.mark.parametrize("shape,fmt", _cases(ROWS), ids=P.ids(_cases(ROWS)))
def test_rows_equal_the_restatement_and_the_composition(shape, fmt):
    for what, xn in _inputs(shape):
        _check(xn, fmt, False, (what, shape, fmt))
        if shape == (3, 288):   # a view one float into a buffer: the per-element arm
            _check(xn, fmt, False, (what, "offset", fmt), x=_offset_view(torch.from_numpy(xn)))


@pytest.mark.parametrize("shape,fmt", _cases(COLS), ids=P.ids(_cases(COLS)))
def test_columns_equal_the_restatement_and_the_composition(shape, fmt):
    o, c, n = shape
    for what, xn in _inputs((o, n, c)):
        _check(np.ascontiguousarray(xn.transpose(0, 2, 1)), fmt, True, (what, shape, fmt))


def test_four_chunks_per_wave_from_the_grid_size_threshold_on():
    # from 64 chunks of 256 per CU on a wave takes 4 chunks: the smallest such tensor; the last workgroup is not full
    rows = -(-64 * torch.cuda.get_device_properties(0).multi_processor_count * 256 // 1056) + 1
    _check(M.gaussian((rows, 1056), 5), "fp4_e2m1", False, "four chunks per wave", restatement=False)


@pytest.mark.parametrize("scale", [1.0, 1.7])
@pytest.mark.parametrize("shape", [(3, 288), (2, 64, 7)], ids=P.ids([(3, 288), (2, 64, 7)]))
def test_backward_equals_the_composition_and_the_restatement(shape, scale):
    cols, fmt = len(shape) == 3, "fp4_e2m1"
    n = int(np.prod(shape))
    xn = (R.inputs(1, n, 3).numpy() * np.float32(scale)).reshape(shape)
    gn = R.inputs(1, n, 4).numpy().reshape(shape)
    xr, gr = (np.ascontiguousarray(a.transpose(0, 2, 1)) if cols else a for a in (xn, gn))
    mask = _reference(xr, fmt)[4]
    assert (mask == 0).any() and (mask == 1).any()   # some rotated elements overflow the element grid
    want = R.hadamard_np(np.where(mask == 1, R.hadamard_np(gr, 32), np.float32(0)), 32)
    want = np.ascontiguousarray(want.transpose(0, 2, 1)) if cols else want
    g = torch.from_numpy(gn).to(DEV)
    a, b = (torch.from_numpy(xn).to(DEV).requires_grad_(True) for _ in range(2))
    V.mx_rot_fake_quant(a, fmt, axis=1 if cols else -1).backward(g)
    q = V.mx_fake_quant(FQ.hadamard_transform(_to_rows(b, cols).contiguous(), 32), fmt)
    _to_rows(FQ.hadamard_transform(q, 32), cols).backward(g)
    assert P.same_bits(a.grad, b.grad)
    assert np.array_equal(M.bits(a.grad.cpu().numpy()), M.bits(want))


def test_a_fused_layer_with_rotated_weights_and_activations():
    torch.manual_seed(0)
    layer = LinearBnReLU(nn.Linear(64, 32), nn.BatchNorm1d(32), nn.ReLU(), "MinMaxObserver", "RotatedMXQuantizer",
                         "MinMaxObserver", "RotatedMXQuantizer", True, True, True, 4, 8).to(DEV)
    xin = torch.randn(8, 64, device=DEV)
    out = layer(xin)
    w, b = layer.get_weight_bias()
    wq = V.mx_rot_fake_quant(w.detach(), "fp4_e2m1")
    assert P.same_bits(layer.quantize_weights(w).detach(), wq)
    codes, scales, fmt = layer.weight_quantizer.export_mx(w.detach())
    assert fmt == "fp4_e2m1" and P.same_bits(V.hadamard_transform(V.mx_dequant(codes, scales, fmt), 32), wq)
    pre = torch.relu(layer._pre_act(xin, wq, b)).detach()
    assert P.same_bits(out.detach(), V.mx_rot_fake_quant(pre, "fp8_e4m3", axis=1))
    out.square().mean().backward()
    grad = layer.linear_fuse.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.ne(0).any())
    conv = nn.Sequential(nn.Conv2d(3, 40, 3, padding=1, bias=False), nn.BatchNorm2d(40), nn.ReLU())
    cfg = FuseConfig(quantizer_w_name="MXQuantizer", quantizer_a_name="RotatedMXQuantizer", bits_w=4, bits_a=8)
    conv = fuse_modules_unified(conv, [("conv", "bn", "relu")], config_manager=FuseConfigManager(cfg)).to(DEV)
    with pytest.raises(ValueError, match="multiple of 32"):   # 40 channels: the activation quantizer
        conv(torch.randn(2, 3, 8, 8, device=DEV))


def test_refusals():
    x = torch.zeros(4, 64, device=DEV)
    with pytest.raises(TypeError):
        V.mx_rot_fake_quant(x.bfloat16(), "fp4_e2m1")
    with pytest.raises(NotImplementedError):
        V.mx_rot_fake_quant(x, "fp4_e2m1", axis=0)


def test_graph_replay_equals_eager():
    # last in the file; the forward alone in one single-stream capture
    x1, x2 = (torch.from_numpy(M.gaussian((9, 576), s)).to(DEV) for s in (1, 2))
    want = FQ._mx_rot_forward(x2, "fp4_e2m1", -1, True, True, want_rotated=True)
    xs = x1.clone()
    fwd = lambda: FQ._mx_rot_forward(xs, "fp4_e2m1", -1, True, True, want_rotated=True)   # noqa: E731
    graph, got = _captured(fwd, fwd)
    xs.copy_(x2)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert P.same_bits(g, w)
