"""AdaRound over the FakeQuantize layers of a calibrated model (post-training).

``adaround_layer(layer, x, ...)`` learns, for one fused conv / linear layer, whether each
weight rounds down or up so that the LAYER'S OUTPUT on ``x`` -- not the weight -- is
reproduced: Adam on ``AdaRoundWeight.V`` minimises the mean squared error between
``run_forward_core(x, soft-quantized weight)`` and ``run_forward_core(x, weight)`` plus
``lam * R``.  Each step is two HIP launches for the rounding (csrc/k_adaround.hip) around
the layer's own conv / linear (MIOpen / hipBLASLt through ``run_forward_core``).  The
hardened weight is then written into the parameter ``get_weight_bias()`` returns: it lies
on the quantizer's grid, so ``quantize_weights``, eval and ``export_packed_weight()``
reproduce the learned codes with no special case.

``adaround_model(model, batches, ...)`` does this layer by layer in forward order, each
layer seeing the input the model produces with the layers before it already rounded.

Not supported (``NotImplementedError`` from adaround_layer; adaround_model lists them in
``skipped`` and goes on): layers with an unfolded BatchNorm (``is_fuse_bn=False``: the BN
sits between the weight and the output and its batch statistics would follow the
optimisation), layers whose ``get_weight_bias()`` returns something other than a leaf
``nn.Parameter`` (nothing to write the result into), and weight quantizers other than
UniformQuantizer / LSQQuantizer / PerChannelUniformQuantizer.  fp32 weights, per tensor or
per out-channel (axis 0), one GPU (or CPU tensors, on the host loops).
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

from ..quantizers.adaround import AdaRoundWeight
from ..quantizers.fake_quantize import FakeQuantize


def _resolved_grid(layer, w):
    """The weight quantizer's current (s, z, qmin, qmax) as constants: detached, a learnable
    zero point already rounded and clamped as the forward does."""
    s, z, qmin, qmax, _axis, zp_round = layer.weight_quantizer.current_grid(w, "adaround_layer")
    s = s.detach() if isinstance(s, torch.Tensor) else s
    z = z.detach() if isinstance(z, torch.Tensor) else z
    if zp_round:
        z = torch.clamp(torch.round(torch.as_tensor(z, dtype=torch.float64)), qmin, qmax)
    return s, z, qmin, qmax


def _writable_weight(layer):
    if not isinstance(layer, FakeQuantize):
        raise TypeError(f"adaround_layer takes a FakeQuantize layer, got {type(layer).__name__}")
    if not getattr(layer, "is_fuse_bn", True):
        raise NotImplementedError(f"adaround_layer: {type(layer).__name__} keeps an unfolded BatchNorm between its "
                                  "weight and its output (is_fuse_bn=False); fold the BN first")
    w, b = layer.get_weight_bias()
    if not (isinstance(w, nn.Parameter) and w.is_leaf):
        raise NotImplementedError(f"adaround_layer: {type(layer).__name__}.get_weight_bias() returns a "
                                  f"{type(w).__name__} that is not a leaf nn.Parameter; there is no parameter to "
                                  "write the rounded weight into")
    return w, b


def adaround_layer(layer, x, iters: int = 1000, lr: float = 1e-2, lam: float = 0.01, beta_range=(20.0, 2.0),
                   warmup: float = 0.2) -> dict:
    """Learn the rounding of ``layer``'s weight on the input batch ``x`` and write the
    hardened weight into the layer.  ``lam`` is 0 for the first ``warmup`` fraction of the
    iterations; afterwards beta goes linearly from beta_range[0] to beta_range[1].
    Returns {"mse_nearest", "mse_adaround", "regulariser", "flipped"}: the output errors of
    round-to-nearest and of the learned rounding with the same qparams, the final R, and
    how many weights round the other way."""
    w, b = _writable_weight(layer)
    s, z, qmin, qmax = _resolved_grid(layer, w)
    wd = w.detach()
    bd = None if b is None else b.detach()
    x = x.detach()
    ada = AdaRoundWeight().init_from(wd, s, z, qmin, qmax)
    ada.train()
    with torch.no_grad():
        target = layer.run_forward_core(x, wd, bd)
        nearest = ada.harden(wd)   # init_from: the hard rounding starts at round-to-nearest
        mse_nearest = torch.mean((layer.run_forward_core(x, nearest, bd) - target) ** 2)
    opt = torch.optim.Adam([ada.V], lr=lr)
    iters = int(iters)
    n_warm = int(round(float(warmup) * iters))
    b0, b1 = float(beta_range[0]), float(beta_range[1])
    for i in range(iters):
        if i < n_warm:
            ada.lam, ada.beta = 0.0, b0
        else:
            ada.lam = float(lam)
            ada.beta = b0 + (b1 - b0) * (i - n_warm) / max(1, iters - n_warm - 1)
        out = layer.run_forward_core(x, ada(wd), bd)
        loss = torch.mean((out - target) ** 2)   # lam * R reaches V through ada's backward
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    with torch.no_grad():
        hard = ada.harden(wd)
        mse_ada = torch.mean((layer.run_forward_core(x, hard, bd) - target) ** 2)
        flipped = (hard != nearest).sum()
        reg = ada.regulariser(b1)
        w.copy_(hard)
    # the rounding was learned for these qparams: an observing manager must not move them
    layer.weight_quantizer.is_observer_qparam = False
    return {"mse_nearest": float(mse_nearest), "mse_adaround": float(mse_ada), "regulariser": float(reg),
            "flipped": int(flipped)}


class _Captured(Exception):
    pass


def _forward_order(model, batch):
    """The FakeQuantize layers of ``model`` in the order one forward of ``batch`` calls them."""
    order, hooks = [], []
    names = {m: n for n, m in model.named_modules()}
    for m in names:
        if isinstance(m, FakeQuantize):
            hooks.append(m.register_forward_pre_hook(lambda mod, _inp: order.append(mod) if mod not in order else None))
    try:
        with torch.no_grad():
            model(batch)
    finally:
        for h in hooks:
            h.remove()
    return [(names[m], m) for m in order]


def _layer_input(model, layer, batches):
    """``layer``'s input over ``batches`` from the model as it stands (the forward is cut at
    the layer)."""
    got = []

    def grab(_mod, inp):
        got.append(inp[0].detach())
        raise _Captured

    h = layer.register_forward_pre_hook(grab)
    try:
        with torch.no_grad():
            for bt in batches:
                try:
                    model(bt)
                except _Captured:
                    pass
    finally:
        h.remove()
    return torch.cat(got, 0)


def adaround_model(model, batches, iters: int = 1000, lr: float = 1e-2, lam: float = 0.01,
                   beta_range=(20.0, 2.0), warmup: float = 0.2) -> dict:
    """AdaRound every FakeQuantize layer of ``model`` in forward order on ``batches`` (a
    list of input tensors on the model's device).  Returns {"layers": {name: adaround_layer's
    record}, "skipped": {name: reason}}; a layer adaround_layer does not support is left as
    it is, listed and warned about."""
    batches = list(batches)
    if not batches:
        raise ValueError("adaround_model needs at least one input batch")
    was_training = model.training
    model.eval()
    done, skipped = {}, {}
    try:
        for name, layer in _forward_order(model, batches[0]):
            try:
                _writable_weight(layer)
                _resolved_grid(layer, layer.get_weight_bias()[0])
            except NotImplementedError as e:
                skipped[name] = str(e)
                warnings.warn(f"adaround_model: layer {name!r} skipped: {e}", RuntimeWarning, stacklevel=2)
                continue
            x = _layer_input(model, layer, batches)
            done[name] = adaround_layer(layer, x, iters=iters, lr=lr, lam=lam, beta_range=beta_range, warmup=warmup)
    finally:
        model.train(was_training)
    return {"layers": done, "skipped": skipped}
