"""PerGroupUniformQuantizer — UniformQuantizer arithmetic (quantizers/uniform.py:34-56) with one
(scale, zero point) per group of ``group_size`` (32 / 64 / 128 / 256) consecutive elements of an
out-channel row: "w4 g128".  ``quantize(x, scale, zero_point, False)`` takes the float64
[rows, groups] tensors PerGroupMinMaxObserver returns (csrc/k_pg.hip; CPU tensors: the native
host loops).  ``group_size`` defaults to 128 and is set on the instance, the way
MXQuantizer.elem_format is; QuantizationManager keeps the observer's in step.

Weights only, fp32 only, fixed qparams only (no learnable group scales, no packed export, no
AdaRound yet).  It is deliberately NOT a UniformQuantizer / PerChannelUniformQuantizer, so none of
the per-tensor or per-channel kernels' branches take it.
"""
from __future__ import annotations

import torch

from ..fakequant import PerGroupFQFn, check_group_size, per_group_fake_quant
from ..utils.registry import register_class
from .base import BaseQuantizer


@register_class
class PerGroupUniformQuantizer(BaseQuantizer):
    axis = 0
    learns_zero_point = False
    #: QuantizationManager / FakeQuantize: refused as an activation quantizer
    weights_only = True

    def __init__(self, num_bits=8, symmetric=True, group_size=128):
        self.num_bits = num_bits
        self.symmetric = symmetric
        if symmetric:
            self.qmin, self.qmax = -(2 ** (num_bits - 1)), 2 ** (num_bits - 1) - 1
        else:
            self.qmin, self.qmax = 0, 2 ** num_bits - 1
        self._group_size = check_group_size(group_size)

    @property
    def group_size(self) -> int:
        return self._group_size

    @group_size.setter
    def group_size(self, g):
        self._group_size = check_group_size(g)

    def quantize(self, x, scale, zero_point, is_learning_scale=False, act=None):
        if act is not None:
            raise NotImplementedError("PerGroupUniformQuantizer quantizes weights only: it takes no activation")
        if is_learning_scale:
            raise NotImplementedError("PerGroupUniformQuantizer has no learnable group scales (is_learning_scale): "
                                      "its qparams come from PerGroupMinMaxObserver")
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            what = x.dtype if isinstance(x, torch.Tensor) else type(x).__name__
            raise TypeError(f"PerGroupUniformQuantizer: only float32 tensors are supported, got {what}")
        if not (isinstance(scale, torch.Tensor) and isinstance(zero_point, torch.Tensor)):
            raise RuntimeError("PerGroupUniformQuantizer.quantize needs the [rows, groups] scale and zero point "
                               "PerGroupMinMaxObserver returns (nothing observed yet?)")
        if x.requires_grad and torch.is_grad_enabled():
            return PerGroupFQFn.apply(x, scale, zero_point, self.qmin, self.qmax, self._group_size)
        return per_group_fake_quant(x, scale, zero_point, self.qmin, self.qmax, group_size=self._group_size)[0]

    def __repr__(self):
        return (f"{type(self).__name__}(num_bits={self.num_bits}, symmetric={self.symmetric}, "
                f"qmin={self.qmin}, qmax={self.qmax}, group_size={self._group_size})")
