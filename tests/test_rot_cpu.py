"""Hadamard-rotated group-wise quantization without a GPU: the host loop of hadamard_G against the
numpy restatement (bit for bit) and the f64 matrix product (within the rounding bound of log2 G
addition stages plus the scale), autograd, a fused layer through the manager, every refusal."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests import pg_common as P
from tests import rot_common as R
from vsiquantization_amd import _hip as H
from vsiquantization_amd.fakequant import (PerGroupRotFQFn, PerGroupRotObserveFQFn, hadamard_transform,
                                           per_group_rot_fake_quant, per_group_rot_observe_fq, pg_rot_ste_backward)
from vsiquantization_amd.modules.fuse import fuse_modules_unified
from vsiquantization_amd.modules.fuse_config import FuseConfig, FuseConfigManager
from vsiquantization_amd.modules.fused import ConvBnReLU, LinearBnReLU


@pytest.mark.parametrize("G", R.GROUPS)
def test_the_transform_of_the_identity_is_the_matrix(G):
    y = hadamard_transform(3.0 * torch.eye(G), G)
    assert np.array_equal(y.numpy(), (np.float32(3.0) * R.c_of(G) * R.sylvester(G)).astype(np.float32))


@pytest.mark.parametrize("rows,rowlen,G", R.CASES, ids=P.ids(R.CASES))
def test_host_loop_equals_the_restatement_within_the_f64_bound(rows, rowlen, G):
    x = R.inputs(rows, rowlen, rows + rowlen + G)
    want = R.hadamard_np(x.numpy(), G)
    assert P.same_bits(hadamard_transform(x, G), torch.from_numpy(want))
    xg = x.double().numpy().reshape(-1, G)
    exact = xg @ R.sylvester(G) / np.sqrt(G)
    bound = (np.log2(G) + 2) * 2.0 ** -24 * np.abs(xg).sum(1, keepdims=True) / np.sqrt(G)
    ratio = (np.abs(want.reshape(-1, G) - exact) / bound).max()
    print(f"G={G} {rows}x{rowlen}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_autograd():
    G = 32
    x, g = P.weights(2, 96, 1).requires_grad_(True), P.weights(2, 96, 2)
    hadamard_transform(x, G).backward(g)
    assert P.same_bits(x.grad, hadamard_transform(g, G))            # symmetric: its own adjoint
    a = P.weights(2, 96, 3).requires_grad_(True)
    y, s, z = PerGroupRotObserveFQFn.apply(a, G, True, -8, 7, 8, 1e-8, None, None)
    y.backward(g)
    want = R.composed(a.detach(), G, True, -8, 7, None, None)
    assert P.same_bits(y, want["y"]) and P.same_bits(a.grad, R.composed_backward(g, want["mask"], s, G))
    b = a.detach().clone().requires_grad_(True)
    PerGroupRotFQFn.apply(b, s, z, -8, 7, G).backward(g)
    assert P.same_bits(b.grad, a.grad)


def test_registry_and_fused_layer_through_the_manager():
    assert V.CLASS_REGISTRY["RotatedPerGroupQuantizer"] is V.RotatedPerGroupQuantizer
    assert V.RotatedPerGroupQuantizer.rotate and not V.PerGroupUniformQuantizer.rotate
    torch.manual_seed(0)
    model = nn.Sequential(nn.Linear(256, 5), nn.BatchNorm1d(5), nn.ReLU())
    cfg = FuseConfig(observer_w_name="PerGroupMinMaxObserver", quantizer_w_name="RotatedPerGroupQuantizer", bits_w=4)
    layer = fuse_modules_unified(model, [("linear", "bn", "relu")], config_manager=FuseConfigManager(cfg))[0]
    assert isinstance(layer, LinearBnReLU)
    wq, x = layer.weight_quantizer, torch.randn(3, 256)
    for q in (wq, layer.activation_quantizer):
        q.is_learning_scale = False
    wq.is_quantize = False                                            # calibrate
    layer(x)
    w = layer.get_weight_bias()[0]
    first = R.composed(w.detach(), 128, True, -8, 7, None, None)
    assert wq.observer.rotate and P.same_bits(wq.scale, first["scale"]) and wq.scale.shape == (5, 2)
    wq.is_quantize = True                                             # train with observed qparams
    layer(x).square().mean().backward()
    want = R.composed(w.detach(), 128, True, -8, 7, first["run_min"], first["run_max"])
    assert P.same_bits(wq.scale, want["scale"]) and bool((layer.linear_fuse.weight.grad != 0).any())
    layer.eval()
    wq.is_observer_qparam = False                                     # eval: the fixed rotated forward
    assert P.same_bits(wq.quantize(w.detach()), want["y"])


def test_refusals():
    lib, null, name = H.lib(), None, "RotatedPerGroupQuantizer"
    for rowlen, group in ((96, 64), (200, 128), (64, 48)):            # rowlen % G != 0, a bad group
        assert {lib.vsiq_pg_hadamard_f32(16, 16, 2, rowlen, group, null),
                lib.vsiq_host_pg_hadamard_f32(16, 16, 2, rowlen, group),
                lib.vsiq_pg_rot_observe_fq_f32(16, 16, null, null, null, 2, rowlen, group, 16, 16, 16, 16, 1, -8, 7,
                                               127.0, 1e-8, null),
                lib.vsiq_pg_rot_fq_fwd_f32(16, 16, null, null, null, 2, rowlen, group, 16, 16, 0, -8, 7, null),
                lib.vsiq_pg_rot_ste_bwd_f32(16, 16, 16, 2, rowlen, group, 16, null)} == {-1}
    assert lib.vsiq_pg_hadamard_f32(null, null, 0, 64, 32, null) == 0
    assert lib.vsiq_pg_hadamard_f32(null, 16, 2, 64, 32, null) == -1
    x, one = P.weights(4, 96, 1), torch.ones(4, 2)

    def layer(n):
        m = LinearBnReLU(nn.Linear(n, 4), nn.BatchNorm1d(4), nn.ReLU(), "PerGroupMinMaxObserver", name,
                         "MinMaxObserver", "UniformQuantizer", True, True, True, 4, 8)
        m.weight_quantizer.is_learning_scale = False
        m.weight_quantizer.quantizer.group_size = 64
        return m
    for call in (lambda: hadamard_transform(x, 64),
                 lambda: per_group_rot_observe_fq(x, group_size=64, symmetric=True, qmin=-8, qmax=7),
                 lambda: per_group_rot_fake_quant(x, one, one, -8, 7, group_size=64),
                 lambda: pg_rot_ste_backward(x, torch.ones(4, 96, dtype=torch.uint8), one, 64),
                 lambda: layer(96)(torch.randn(3, 96))):              # a layer: at its first call
        with pytest.raises(ValueError, match="rowlen = 96.*G = 64"):
            call()
    x, ada = P.weights(4, 64, 1), layer(64)
    ada.weight_quantizer.quantize(ada.get_weight_bias()[0].detach())
    qm = V.QuantizationManager(name, "PerGroupMinMaxObserver", 4, True, False)
    qm.quantizer.group_size = 32
    qm.quantize(x)
    for match, call in (
            ("PerGroupMSEObserver", lambda: V.QuantizationManager(name, "PerGroupMSEObserver", 4, True, False).quantize(x)),
            (name, lambda: V.QuantizationManager(name, "PerGroupMinMaxObserver", 4, True).quantize(x)),   # is_learning_scale
            (name, lambda: V.RotatedPerGroupQuantizer(4, True).quantize(x, one, one, True)),
            ("PerGroup", lambda: qm.quantize(x, act="relu")),
            (name, lambda: ConvBnReLU(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.ReLU(), "MinMaxObserver",
                                      "UniformQuantizer", "MinMaxObserver", name, True, True, True, 4, 8)),
            (name, lambda: qm.export_packed(x)), (name, lambda: qm.current_grid(x)),
            (name, lambda: V.adaround_layer(ada, torch.randn(8, 64))),
            ("codes", lambda: per_group_rot_observe_fq(x, group_size=32, symmetric=True, qmin=-8, qmax=7, want_codes=True))):
        with pytest.raises(NotImplementedError, match=match):
            call()
