"""GPTQ over the group-wise FakeQuantize layers of a calibrated model (post-training).

``gptq_layer(layer, x)`` rounds one fused conv / linear layer's weight with error compensation
(Frantar et al. 2022): the Hessian of the layer's inputs ``x`` (``gptq_hessian``), the upper
Cholesky factor of its damped inverse (``gptq_factor``), then ``fakequant.per_group_gptq`` -- the
HIP kernels of csrc/k_gptq.hip on the GPU, the host loop on CPU tensors.  The result ``y`` is
written into the parameter ``get_weight_bias()`` returns and GPTQ's own group (scale, zero point)
are installed as the weight manager's fixed qparams: the eval forward's quantized weight is then
``y`` bit for bit (``y`` lies on that grid; observing ``y`` again would give other qparams, so the
manager stops observing).

``gptq_model(model, batches)`` does this layer by layer in forward order, each layer seeing the
input the model produces with the layers before it already rounded.

Not supported (``NotImplementedError`` naming the class from gptq_layer; gptq_model lists them in
``skipped`` and goes on): weight quantizers other than PerGroupUniformQuantizer with
PerGroupMinMaxObserver (no rotated groups, no LSQ, no MSE observer), group_size 256, a row length
that is not a multiple of the group size, grouped or dilated convs, an unfolded BatchNorm, a weight
that is not a leaf parameter.  fp32 weights, one GPU (or CPU tensors).
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..fakequant import GPTQ_GROUPS, per_group_gptq, per_group_observe_fq
from ..observers.per_group import PerGroupMinMaxObserver
from ..quantizers.fake_quantize import FakeQuantize
from ..quantizers.per_group import PerGroupUniformQuantizer
from .adaround import _forward_order, _layer_input


def _columns(layer, x):
    """The layer's input as the [n, rowlen] matrix whose columns match the weight's rows
    ([O, I] of a linear, [O, I * kh * kw] of a conv: F.unfold's order)."""
    conv = getattr(layer, "conv_fuse", None)
    if conv is None:
        return x.reshape(-1, x.shape[-1])
    cols = F.unfold(x, conv.kernel_size, dilation=conv.dilation, padding=conv.padding, stride=conv.stride)
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


def gptq_hessian(layer, x) -> torch.Tensor:
    """H = X^T X / n in fp32, [rowlen, rowlen], of ``layer``'s input batch ``x`` (plumbing: one
    addmm_ on x's device)."""
    X = _columns(layer, x.detach().to(torch.float32))
    H = torch.zeros(X.shape[1], X.shape[1], dtype=torch.float32, device=X.device)
    return H.addmm_(X.t(), X, beta=0.0, alpha=1.0 / X.shape[0])


def gptq_factor(H: torch.Tensor, percdamp: float = 0.01) -> torch.Tensor:
    """The fp32 upper Cholesky factor U of the damped inverse Hessian, as GPTQ builds it: dead
    columns (H[i, i] == 0) get a 1 on the diagonal, percdamp * mean(diag) is added to it, then, in
    float64, Cholesky -> cholesky_inverse -> upper Cholesky.  The three f64 factorizations run
    on the host (a [rowlen, rowlen] problem once per layer; no dependence on the GPU build's
    linalg backend) and U is copied to H's device."""
    Hd = H.detach().to("cpu", torch.float64).clone()
    d = torch.diagonal(Hd)
    d[d == 0] = 1.0
    d += float(percdamp) * d.mean()
    Hinv = torch.cholesky_inverse(torch.linalg.cholesky(Hd))
    return torch.linalg.cholesky(Hinv, upper=True).to(torch.float32).to(H.device).contiguous()


def _checked(layer):
    """(weight parameter, bias, quantizer, observer) of a layer gptq_layer supports, or the refusal."""
    if not isinstance(layer, FakeQuantize):
        raise TypeError(f"gptq_layer takes a FakeQuantize layer, got {type(layer).__name__}")
    name = type(layer).__name__
    mgr = layer.weight_quantizer
    q, obs = mgr.quantizer, mgr.observer
    if type(q) is not PerGroupUniformQuantizer or type(obs) is not PerGroupMinMaxObserver:
        raise NotImplementedError(f"gptq_layer: {name} quantizes its weight with {type(q).__name__} / "
                                  f"{type(obs).__name__}; GPTQ needs PerGroupUniformQuantizer with "
                                  "PerGroupMinMaxObserver")
    if q.group_size not in GPTQ_GROUPS:
        raise NotImplementedError(f"gptq_layer: {name}'s {type(q).__name__} has group_size {q.group_size}; GPTQ takes "
                                  f"{GPTQ_GROUPS}")
    if not getattr(layer, "is_fuse_bn", True):
        raise NotImplementedError(f"gptq_layer: {name} keeps an unfolded BatchNorm between its weight and its output "
                                  "(is_fuse_bn=False); fold the BN first")
    conv = getattr(layer, "conv_fuse", None)
    if conv is not None and (conv.groups != 1 or tuple(conv.dilation) != (1, 1)):
        raise NotImplementedError(f"gptq_layer: {name}'s conv has groups={conv.groups}, dilation={tuple(conv.dilation)}; "
                                  "grouped and dilated convs are not supported")
    w, b = layer.get_weight_bias()
    if not (isinstance(w, nn.Parameter) and w.is_leaf):
        raise NotImplementedError(f"gptq_layer: {name}.get_weight_bias() returns a {type(w).__name__} that is not a "
                                  "leaf nn.Parameter; there is no parameter to write the rounded weight into")
    rowlen = w.numel() // w.shape[0]
    if rowlen % q.group_size:
        raise NotImplementedError(f"gptq_layer: {name}'s weight rows have {rowlen} elements, not a multiple of "
                                  f"group_size {q.group_size}")
    return w, b, q, obs


def gptq_layer(layer, x, percdamp: float = 0.01) -> dict:
    """GPTQ ``layer``'s weight on the input batch ``x``, write it into the layer and freeze its
    group qparams.  Returns {"mse_nearest", "mse_gptq"}: the layer's output error on ``x`` of
    round-to-nearest (per_group_observe_fq of the same weight) and of GPTQ."""
    w, b, q, obs = _checked(layer)
    mgr = layer.weight_quantizer
    x = x.detach()
    grid = dict(group_size=q.group_size, symmetric=obs.symmetric, qmin=q.qmin, qmax=q.qmax, obs_bits=obs.num_bits,
                eps=obs.eps)
    with torch.no_grad():
        bd = None if b is None else b.detach()
        H = gptq_hessian(layer, x)
        wd = w.detach().clone()
        wd.view(wd.shape[0], -1)[:, torch.diagonal(H) == 0] = 0.0   # dead inputs: their weights do not matter
        r = per_group_gptq(wd, gptq_factor(H, percdamp), **grid)
        target = layer.run_forward_core(x, w.detach(), bd)
        nearest = per_group_observe_fq(wd, **grid)["y"]
        mse_nearest = torch.mean((layer.run_forward_core(x, nearest, bd) - target) ** 2)
        mse_gptq = torch.mean((layer.run_forward_core(x, r["y"], bd) - target) ** 2)
        w.copy_(r["y"])
    # y is on the grid of GPTQ's own group qparams: the manager keeps exactly those
    mgr.scale, mgr.zero_point = r["scale"], r["zp"]
    mgr.is_observer_qparam = False
    mgr.is_learning_scale = False   # PerGroupUniformQuantizer has nothing to learn; eval takes the fixed forward
    return {"mse_nearest": float(mse_nearest), "mse_gptq": float(mse_gptq)}


def gptq_model(model, batches, percdamp: float = 0.01) -> dict:
    """GPTQ every FakeQuantize layer of ``model`` in forward order on ``batches`` (a list of
    input tensors on the model's device).  Returns {"layers": {name: gptq_layer's record},
    "skipped": {name: reason}}; a layer gptq_layer does not support is left as it is, listed and
    warned about."""
    batches = list(batches)
    if not batches:
        raise ValueError("gptq_model needs at least one input batch")
    was_training = model.training
    model.eval()
    done, skipped = {}, {}
    try:
        for name, layer in _forward_order(model, batches[0]):
            try:
                _checked(layer)
            except NotImplementedError as e:
                skipped[name] = str(e)
                warnings.warn(f"gptq_model: layer {name!r} skipped: {e}", RuntimeWarning, stacklevel=2)
                continue
            done[name] = gptq_layer(layer, _layer_input(model, layer, batches), percdamp=percdamp)
    finally:
        model.train(was_training)
    return {"layers": done, "skipped": skipped}
