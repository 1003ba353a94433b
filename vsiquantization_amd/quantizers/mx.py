"""MXQuantizer: OCP Microscaling (MX v1.0) block-scaled fake quantization behind the
quantizer protocol -- the tensors the MI355X block-scaled MFMA path consumes: 32 elements share one
power-of-two E8M0 scale and each element is a 4-, 6- or 8-bit float (MXFP4 / MXFP6 / MXFP8).

The scale comes from each block's own maximum, so there is nothing to observe and nothing to
learn: ``self_scaled`` tells QuantizationManager to call ``quantize`` without an observer
pass, stats records or qparams.  CPU float32 tensors only so far, on the library's native
host loops (csrc/k_host.hip, element code csrc/k_mx.cuh); a CUDA tensor raises, there is no
HIP kernel for it yet.  Straight-through gradient from the saved mask.
"""
from __future__ import annotations

from ..fakequant import mx_fake_quant
from ..utils.registry import register_class
from .base import BaseQuantizer

_BY_BITS = {4: "fp4_e2m1", 6: "fp6_e2m3", 8: "fp8_e4m3"}
_FORMATS = {"fp4_e2m1": 4, "fp6_e2m3": 6, "fp6_e3m2": 6, "fp8_e4m3": 8, "fp8_e5m2": 8}


@register_class
class MXQuantizer(BaseQuantizer):
    #: QuantizationManager: no observer call, no stats, no qparams for this quantizer
    self_scaled = True
    learns_zero_point = False

    def __init__(self, num_bits=4, symmetric=True):
        if num_bits not in _BY_BITS:
            raise ValueError(f"MXQuantizer: element width must be 4, 6 or 8 bits, got {num_bits!r}")
        self.num_bits = num_bits
        self.symmetric = symmetric   # MX element formats are sign-magnitude: always symmetric
        self._elem_format = _BY_BITS[num_bits]
        #: the axis the blocks of 32 run along: -1 suits weights ([out, in * kh * kw] rows);
        #: the fused layers' activation managers get 1 (the channels of [N, C, ...])
        self.block_axis = -1

    @property
    def elem_format(self) -> str:
        return self._elem_format

    @elem_format.setter
    def elem_format(self, fmt: str):
        if fmt not in _FORMATS:
            raise ValueError(f"MXQuantizer: unknown element format {fmt!r} (one of {sorted(_FORMATS)})")
        self._elem_format = fmt
        self.num_bits = _FORMATS[fmt]

    def quantize(self, x, scale=None, zero_point=None, is_learning_scale=False, act=None):
        """MX fake quant of ``x`` (``scale`` / ``zero_point`` / ``is_learning_scale`` belong to
        the protocol and are ignored; ``act`` is applied by the caller, unfused)."""
        if act is not None:
            raise ValueError("MXQuantizer has no fused activation: apply it first (QuantizationManager does)")
        axis = self.block_axis
        if x.dim() < 2 and axis not in (-1, x.dim() - 1):
            axis = -1   # a vector has one axis
        return mx_fake_quant(x, self._elem_format, axis=axis)

    def __repr__(self):
        return f"{type(self).__name__}(elem_format={self._elem_format!r}, block_axis={self.block_axis})"
