"""PerGroupUniformQuantizer — UniformQuantizer arithmetic (quantizers/uniform.py:34-56) with one
(scale, zero point) per group of ``group_size`` (32 / 64 / 128 / 256) consecutive elements of an
out-channel row: "w4 g128".  ``quantize(x, scale, zero_point, False)`` takes the float64
[rows, groups] tensors PerGroupMinMaxObserver returns (csrc/k_pg.hip; CPU tensors: the native
host loops).  ``group_size`` defaults to 128 and is set on the instance, the way
MXQuantizer.elem_format is; QuantizationManager keeps the observer's in step.

Weights only, fp32 only, no packed export, no AdaRound yet.  It is deliberately NOT a
UniformQuantizer / PerChannelUniformQuantizer, so none of the per-tensor or per-channel kernels'
branches take it.

PerGroupUniformQuantizer itself has fixed (observed) qparams only and refuses
``is_learning_scale``.  Learnable group scales (LSQ) come under a name of their own,
PerGroupLSQQuantizer below, the way LSQQuantizer sits beside UniformQuantizer.
"""
from __future__ import annotations

import torch

from ..fakequant import PerGroupFQFn, PerGroupLearnFn, _pg_view, check_group_size, per_group_fake_quant
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


@register_class
class PerGroupLSQQuantizer(PerGroupUniformQuantizer):
    """PerGroupUniformQuantizer whose [rows, groups] scale -- and, asymmetric, zero point -- can
    be learned (LSQ): ``quantize(x, scale, zero_point, True)`` runs the group-wise forward with
    the zero point rounded and clamped when it is learned, and one backward launch
    (fakequant.pg_lsq_backward) that returns grad_x and every group's scale / zero-point gradient.
    Used with PerGroupMinMaxObserver, whose observed qparams QuantizationManager.
    make_learn_qparameter turns into Parameters.

    The gradient scale is (qmax * group_size) ** -0.5: group_size is the nominal element count
    per scale, the analogue of PerChannelUniformQuantizer's numel / C.  It is one number for the
    whole tensor, so it also applies to a row's short last group, which holds fewer elements.

    Under torch.no_grad(), or when neither x nor a qparam requires grad, the same forward runs
    without the autograd Function (a frozen x with a scale Parameter still trains the scale).
    ``is_learning_scale`` False behaves as the base class; ``act`` still raises."""

    def __init__(self, num_bits=8, symmetric=True, group_size=128):
        super().__init__(num_bits, symmetric, group_size)
        self.learns_zero_point = not symmetric

    def quantize(self, x, scale, zero_point, is_learning_scale=False, act=None):
        if not is_learning_scale or act is not None:
            return super().quantize(x, scale, zero_point, False, act=act)
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            what = x.dtype if isinstance(x, torch.Tensor) else type(x).__name__
            raise TypeError(f"PerGroupLSQQuantizer: only float32 tensors are supported, got {what}")
        if not isinstance(scale, torch.Tensor):
            raise RuntimeError("PerGroupLSQQuantizer.quantize needs a [rows, groups] scale (observe with "
                               "PerGroupMinMaxObserver, then QuantizationManager.make_learn_qparameter)")
        G = self._group_size
        if not isinstance(zero_point, torch.Tensor):   # the manager's 0 for a symmetric quantizer
            rows, _, ngr = _pg_view(x, G)
            zero_point = torch.full((rows, ngr), float(zero_point), dtype=torch.float64, device=x.device)
        learn_zp = self.learns_zero_point
        if not (x.requires_grad or scale.requires_grad or zero_point.requires_grad) or not torch.is_grad_enabled():
            return per_group_fake_quant(x, scale, zero_point, self.qmin, self.qmax, group_size=G,
                                        zp_round=learn_zp)[0]
        gscale = float((self.qmax * G) ** -0.5)
        return PerGroupLearnFn.apply(x, scale, zero_point, self.qmin, self.qmax, gscale, learn_zp, G)
