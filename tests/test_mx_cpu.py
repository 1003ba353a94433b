"""MX block-scaled fake quantization on CPU tensors: the host loops (csrc/k_host.hip, the
element code of csrc/k_mx.cuh) against the numpy restatement of
tests/mx_common.py bit for bit, torch's own FP8 / E8M0 casts as an independent cross-check,
and the Python layers on CPU tensors (mx_fake_quant, mx_dequant, MXFakeQuantFn, MXQuantizer
through QuantizationManager, a fused ConvBnReLU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from vsiquantization_amd import _hip as H
from vsiquantization_amd import fakequant as FQ
from vsiquantization_amd.modules.fuse import fuse_modules_unified
from vsiquantization_amd.modules.fuse_config import FuseConfig, FuseConfigManager
from tests import mx_common as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(x, fmt, axis):
    y, codes, scales, mask = FQ._mx_forward(torch.from_numpy(x), fmt, axis, True, True)
    return y.numpy(), codes.numpy(), scales.numpy(), mask.numpy()


def _check(x, fmt, axis, what):
    ry, rc, rs, rm = (M.ref_rows if axis == -1 else M.ref_cols)(x, fmt)
    y, codes, scales, mask = _host(x, fmt, axis)
    assert np.array_equal(M.bits(y), M.bits(ry)), (what, "y")
    assert np.array_equal(codes, rc), (what, "codes")
    assert np.array_equal(scales, rs), (what, "scales")
    assert np.array_equal(mask, rm), (what, "mask")


def test_symbols_exist_and_the_abi_is_still_13():
    lib = H.lib()
    assert lib.vsiq_abi_version() == 13 and H.ABI_VERSION == 13
    for name in ("vsiq_mx_blocks", "vsiq_host_mx_fq_fwd_f32", "vsiq_host_mx_fq_fwd_cols_f32"):
        assert name in H.EXPORTED and hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "vsiq.h")).read()
    codes = dict(re.findall(r"#define VSIQ_MX_(\w+) (\d+)", hdr))
    assert {k.lower(): int(v) for k, v in codes.items()} == {n: M.FORMATS[n][0] for n in M.NAMES}
    assert {n: v[0] for n, v in H.MX_FORMATS.items()} == {n: M.FORMATS[n][0] for n in M.NAMES}
    assert lib.vsiq_mx_blocks(3, 27) == 3 and lib.vsiq_mx_blocks(2, 64) == 4 and lib.vsiq_mx_blocks(5, 100) == 20
    assert {V.MXQuantizer, V.mx_fake_quant, V.mx_dequant} and V.CLASS_REGISTRY["MXQuantizer"] is V.MXQuantizer


@pytest.mark.parametrize("fmt", M.NAMES)
def test_host_rows_equal_the_restatement(fmt):
    _check(M.builder(fmt), fmt, -1, "builder")
    _check(M.special_blocks(), fmt, -1, "special")
    _check(M.ragged_rows(), fmt, -1, "ragged")
    for i, shape in enumerate(M.ROW_SHAPES):
        _check(M.fill(shape, fmt), fmt, -1, ("fill", shape))
        _check(M.gaussian(shape, i), fmt, -1, ("gaussian", shape))


@pytest.mark.parametrize("fmt", M.NAMES)
def test_host_columns_equal_the_restatement(fmt):
    for blocks in (M.builder(fmt), M.special_blocks()):
        _check(np.ascontiguousarray(blocks.T)[None], fmt, 1, "blocks as columns")   # [1, 32, blocks]
    for i, shape in enumerate(M.COL_SHAPES):
        _check(M.fill(shape, fmt), fmt, 1, ("fill", shape))
        _check(M.gaussian(shape, i), fmt, 1, ("gaussian", shape))


def test_builder_holds_what_it_promises():
    for fmt in M.NAMES:
        emax, maxn, ovf = M.FORMATS[fmt][5:8]
        g = M.grid(fmt)
        for k in M.PIN_EXPONENTS:
            b = M.builder_blocks(fmt, k)
            assert b.shape[1] == 32 and np.all(np.abs(b[:, 7]) == np.float32(2.0 ** (k + emax)))
            assert np.array_equal(M.ref_rows(b, fmt)[2], np.full((len(b), 1), k + 127, np.uint8))
            a = np.ldexp(np.abs(b.astype(np.float64)), -k)
            if k != -127:   # (at -127 the neighbours of a midpoint are denormal steps apart)
                for v in list(g[:-1]) + list((g[:-1] + g[1:]) / 2):
                    assert (a == v).any(), (fmt, k, v)
            assert ((a > maxn) & (a < 2.0 ** (emax + 1))).any() and (a == (maxn + ovf) / 2).any()
            assert np.signbit(b[b == 0]).any() and not np.signbit(b[b == 0]).all()
        y, _, _, m = M.ref_rows(M.builder(fmt), fmt)
        assert (m == 0).any() and (m == 1).any()


@pytest.mark.parametrize("fmt,dtype", [("fp8_e4m3", "float8_e4m3fn"), ("fp8_e5m2", "float8_e5m2")])
def test_fp8_rounding_equals_torch_cast(fmt, dtype):
    """Independent of the restatement: torch's CPU cast is RNE with subnormals, and the clamp
    saturates.  The E = 0 blocks of the builder have X = 1, so y is q itself."""
    maxn = M.FORMATS[fmt][6]
    t8 = getattr(torch, dtype)
    probe = torch.tensor([464.0, 2.0 ** -10, 1.5 * 2.0 ** -9]).to(torch.float8_e4m3fn).float()
    assert probe.tolist() == [448.0, 0.0, 2.0 ** -8]
    x = M.builder_blocks(fmt, 0)
    y = V.mx_fake_quant(torch.from_numpy(x), fmt)
    want = torch.from_numpy(x).clamp(-maxn, maxn).to(t8).float()
    assert np.array_equal(M.bits(y.numpy()), M.bits(want.numpy()))


def test_scale_bytes_equal_torch_e8m0():
    t8 = getattr(torch, "float8_e8m0fnu", None)
    x = np.concatenate([M.builder("fp4_e2m1"), M.gaussian((40, 32), 5)])
    _, _, scales = V.mx_fake_quant(torch.from_numpy(x), "fp4_e2m1", want_codes=True)
    s = scales.reshape(-1).to(torch.int32)
    X = torch.where(s == 0, torch.full_like(s, 0x00400000), s << 23).view(torch.float32)
    assert torch.equal(X.double(), torch.pow(2.0, (s - 127).double()))
    try:   # the cast where this torch defines it on CPU tensors (normal X: E8M0 of 2^-127 is byte 0)
        got = X.to(t8).view(torch.uint8)
    except (TypeError, RuntimeError, NotImplementedError):
        return
    assert torch.equal(got.to(torch.int32), s)


@pytest.mark.parametrize("fmt", M.NAMES)
def test_dequant_and_idempotence(fmt):
    for x, axis in ((M.builder(fmt), -1), (M.special_blocks(), -1), (M.gaussian((5, 100), 1), -1),
                    (M.gaussian((2, 33, 7), 2), 1), (M.fill((1, 64, 65), fmt), 1)):
        xt = torch.from_numpy(x)
        y, codes, scales = V.mx_fake_quant(xt, fmt, axis=axis, want_codes=True)
        assert codes.shape == xt.shape and codes.dtype == torch.uint8 and scales.dtype == torch.uint8
        d = V.mx_dequant(codes, scales, fmt, axis=axis)
        assert np.array_equal(M.bits(d.numpy()), M.bits(y.numpy()))
        y2 = V.mx_fake_quant(y, fmt, axis=axis)
        assert np.array_equal(M.bits(y2.numpy()), M.bits(y.numpy()))
        assert np.array_equal(M.bits(V.mx_fake_quant(xt, fmt, axis=axis).numpy()), M.bits(y.numpy()))


def test_axes_and_layouts():
    x = torch.from_numpy(M.gaussian((2, 40, 6, 5), 3))
    y = V.mx_fake_quant(x, "fp6_e3m2", axis=1)
    ref = M.ref_cols(x.numpy().reshape(2, 40, 30), "fp6_e3m2")[0].reshape(2, 40, 6, 5)
    assert np.array_equal(M.bits(y.numpy()), M.bits(ref))
    assert torch.equal(V.mx_fake_quant(x, "fp6_e3m2", axis=-3), y)
    cl = x.contiguous(memory_format=torch.channels_last)   # NHWC memory: the row form, same values
    ycl, ccl, scl = V.mx_fake_quant(cl, "fp6_e3m2", axis=1, want_codes=True)
    assert ycl.is_contiguous(memory_format=torch.channels_last) and torch.equal(ycl, y)
    assert scl.shape == (2, 2, 6, 5) and torch.equal(V.mx_dequant(ccl, scl, "fp6_e3m2", axis=1), y)
    nc = torch.from_numpy(M.gaussian((6, 70), 4))
    assert torch.equal(V.mx_fake_quant(nc, "fp4_e2m1", axis=1), V.mx_fake_quant(nc, "fp4_e2m1", axis=-1))
    t = nc.t()   # non-contiguous: made contiguous first
    assert torch.equal(V.mx_fake_quant(t, "fp4_e2m1"), V.mx_fake_quant(t.contiguous(), "fp4_e2m1"))
    for axis in (0, 2):
        with pytest.raises(NotImplementedError):
            V.mx_fake_quant(x, "fp4_e2m1", axis=axis)


@pytest.mark.parametrize("shape,axis", [((3, 100), -1), ((4, 64), -1), ((2, 40, 7), 1)])
def test_autograd_is_the_straight_through_mask(shape, axis):
    x = M.gaussian(shape, 11)
    g = torch.from_numpy(np.random.default_rng(12).standard_normal(shape).astype(np.float32))
    xt = torch.from_numpy(x).requires_grad_(True)
    y = V.mx_fake_quant(xt, "fp4_e2m1", axis=axis)
    y.backward(g)
    x2 = x.reshape(-1, shape[-1]) if axis == -1 else x
    mask = (M.ref_rows if axis == -1 else M.ref_cols)(x2, "fp4_e2m1")[3].reshape(shape)
    assert (mask == 0).any() and (mask == 1).any()
    want = np.where(mask == 1, g.numpy(), np.float32(0))
    assert np.array_equal(M.bits(xt.grad.numpy()), M.bits(want))


def test_quantizer_through_the_manager():
    m = V.QuantizationManager("MXQuantizer", "MinMaxObserver", 4, True, is_learning_scale=False)
    assert isinstance(m.quantizer, V.MXQuantizer) and m.quantizer.elem_format == "fp4_e2m1"
    assert m.quantizer.self_scaled and m.quantizer.block_axis == -1
    state = (m.observer.min_val, m.observer.max_val)
    x = torch.from_numpy(M.gaussian((5, 100), 2))
    y = m.quantize(x)
    assert torch.equal(y, V.mx_fake_quant(x, "fp4_e2m1"))
    assert (m.observer.min_val, m.observer.max_val) == state          # no observer call
    assert m.mean_abs_x == [] and m.mean_x == [] and m.std == []      # no stats
    assert m.scale == 1 and m.zero_point == 0
    assert torch.equal(m.quantize(x, act="relu"), V.mx_fake_quant(torch.relu(x), "fp4_e2m1"))
    m.is_quantize = False
    assert m.quantize(x) is x
    assert torch.equal(m.quantize(x, act="relu"), torch.relu(x))
    m.is_quantize = True
    m.make_learn_qparameter()
    m.init_scaling_factor_for_learning()
    assert m.scale == 1 and m.zero_point == 0 and not list(m.parameters())
    codes, scales, fmt = m.export_mx(x)
    assert fmt == "fp4_e2m1" and torch.equal(V.mx_dequant(codes, scales, fmt), y)
    for call in (m.export_packed, m.current_grid):
        with pytest.raises(NotImplementedError, match="MXQuantizer"):
            call(x)
    with pytest.raises(NotImplementedError, match="UniformQuantizer"):
        V.QuantizationManager("UniformQuantizer", "MinMaxObserver", 8, True).export_mx(x)
    # the state_dict round-trips
    m2 = V.QuantizationManager("MXQuantizer", "MinMaxObserver", 4, True)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2.quantize(x), y)


def test_quantizer_formats():
    assert V.MXQuantizer().elem_format == "fp4_e2m1"
    assert V.MXQuantizer(6).elem_format == "fp6_e2m3" and V.MXQuantizer(8, True).elem_format == "fp8_e4m3"
    q = V.MXQuantizer(6)
    q.elem_format = "fp6_e3m2"
    x = torch.from_numpy(M.gaussian((3, 64), 9))
    assert torch.equal(q.quantize(x, 1, 0, False), V.mx_fake_quant(x, "fp6_e3m2"))
    q.elem_format = "fp8_e5m2"
    assert q.num_bits == 8
    for bits in (2, 3, 5, 7, 16):
        with pytest.raises(ValueError):
            V.MXQuantizer(bits)
    with pytest.raises(ValueError):
        q.elem_format = "fp8_e3m4"


def test_fused_conv_bn_relu_runs_forward_and_backward():
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(3, 40, 3, padding=1, bias=False), nn.BatchNorm2d(40), nn.ReLU())
    cfg = FuseConfig(quantizer_w_name="MXQuantizer", quantizer_a_name="MXQuantizer", bits_w=4, bits_a=8)
    model = fuse_modules_unified(model, [("conv", "bn", "relu")], config_manager=FuseConfigManager(cfg))
    layer = model[0]
    assert type(layer).__name__ == "ConvBnReLU"
    wq, aq = layer.weight_quantizer.quantizer, layer.activation_quantizer.quantizer
    assert (wq.elem_format, wq.block_axis, aq.elem_format, aq.block_axis) == ("fp4_e2m1", -1, "fp8_e4m3", 1)
    x = torch.randn(2, 3, 8, 8)
    out = model(x)
    w, b = layer.get_weight_bias()
    pre = torch.relu(layer._pre_act(x, V.mx_fake_quant(w.detach(), "fp4_e2m1"), b)).detach()
    assert torch.equal(out.detach(), V.mx_fake_quant(pre, "fp8_e4m3", axis=1))
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    before = layer.conv_fuse.weight.detach().clone()
    out.square().mean().backward()
    assert layer.conv_fuse.weight.grad is not None and torch.isfinite(layer.conv_fuse.weight.grad).all()
    opt.step()
    assert not torch.equal(layer.conv_fuse.weight.detach(), before)


def test_bad_arguments():
    lib = H.lib()
    buf = (ctypes.c_float * 64)()
    out = (ctypes.c_float * 64)()
    p, o = ctypes.addressof(buf), ctypes.addressof(out)
    assert lib.vsiq_host_mx_fq_fwd_f32(p, o, None, None, None, 2, 32, 0) == 0
    assert lib.vsiq_host_mx_fq_fwd_f32(p, o, None, None, None, 2, 32, 5) == -1      # unknown format
    assert lib.vsiq_host_mx_fq_fwd_f32(p, o, None, None, None, 2, 32, -1) == -1
    assert lib.vsiq_host_mx_fq_fwd_f32(p, o, None, None, None, 0, 32, 0) == -1      # sizes
    assert lib.vsiq_host_mx_fq_fwd_f32(p, o, None, None, None, 2, 0, 0) == -1
    assert lib.vsiq_host_mx_fq_fwd_f32(p, None, o, None, None, 2, 32, 0) == -1      # codes without y
    assert lib.vsiq_host_mx_fq_fwd_cols_f32(p, o, None, None, None, 1, 2, 32, 0) == 0
    assert lib.vsiq_host_mx_fq_fwd_cols_f32(p, o, None, None, None, 1, 0, 32, 0) == -1
    assert lib.vsiq_host_mx_fq_fwd_cols_f32(p, None, None, o, None, 1, 2, 32, 0) == -1
    assert lib.vsiq_host_mx_fq_fwd_cols_f32(p, o, None, None, None, 1, 2, 32, 7) == -1
    assert lib.vsiq_mx_blocks(0, 32) == -1 and lib.vsiq_mx_blocks(4, 0) == -1
    x = torch.zeros(4, 64)
    with pytest.raises(ValueError):
        V.mx_fake_quant(x, "fp5_e2m2")
    with pytest.raises(ValueError):
        V.mx_fake_quant(torch.zeros(0, 32), "fp4_e2m1")
    with pytest.raises(NotImplementedError):
        V.mx_fake_quant(x, "fp4_e2m1", axis=0)
    with pytest.raises((TypeError, H.VsiqError)):
        V.mx_fake_quant(x.double(), "fp4_e2m1")
    with pytest.raises(TypeError):
        V.mx_fake_quant([1.0], "fp4_e2m1")
    with pytest.raises(H.VsiqError, match="no HIP kernel"):   # never a quiet copy to the host
        V.mx_fake_quant(torch.zeros(4, 64, device="meta"), "fp4_e2m1")
