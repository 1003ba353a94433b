"""Export a trained / calibrated model's weights as packed integer codes.

``export_packed_state(model)`` walks the ``FakeQuantize`` layers and returns, per layer,
the weight as a ``PackedTensor.state()`` dict (2 / 4 / 8-bit codes + the fp32 qparams that
reproduce the fake-quantized weight exactly) and the bias: plain tensors, ints, lists and
None, so ``torch.save`` / ``torch.load(weights_only=True)`` round-trips it.
``packed_state_weights(state)`` is the inverse: the dequantized weight of every layer.
Loading a packed state back into a model for inference is out of scope.
"""
from __future__ import annotations

import torch


def export_packed_state(model) -> dict:
    """{module_name: {"weight": PackedTensor.state(), "bias": tensor | None}} for every
    FakeQuantize submodule of ``model`` (FakeQuantize.export_packed_weight)."""
    from ..quantizers.fake_quantize import FakeQuantize
    out = {}
    for name, m in model.named_modules():
        if isinstance(m, FakeQuantize):
            packed, bias = m.export_packed_weight()
            out[name] = {"weight": packed.state(), "bias": None if bias is None else bias.clone()}
    return out


def packed_state_weights(state: dict, dtype=torch.float32, device=None) -> dict:
    """{module_name: dequantized weight} of an export_packed_state dict (fakequant.
    unpack_dequant on ``device``; None: where the packed data lies)."""
    from ..fakequant import PackedTensor, unpack_dequant
    out = {}
    for name, entry in state.items():
        p = PackedTensor.from_state(entry["weight"])
        if device is not None:
            p = p.to(device)
        out[name] = unpack_dequant(p, dtype)
    return out
