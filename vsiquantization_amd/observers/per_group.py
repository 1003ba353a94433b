"""PerGroupMinMaxObserver — group-wise MinMax ("w4 g128"), build-defined like the per-channel
observer: the reference's MinMaxObserver applied independently to every run of
``group_size`` (32 / 64 / 128 / 256) consecutive elements of an out-channel row,

    s[r, j], z[r, j] = MinMaxObserver(symmetric, num_bits).forward(W[r].flatten()[j*G : (j+1)*G])

with groups restarting at every row (the last group of a row may be short) and one running
(min_val, max_val) per group (fresh observers start at 0/0, minmax.py:28-29).  One launch of
csrc/k_pg.hip; scale and zero point come back as float64 [rows, groups] device tensors (no host
sync).  CPU tensors take the native host loops group by group: the same bits.

Weights only, fp32 only (PerGroupLSQQuantizer learns the qparams observed here); it is deliberately NOT a
PerChannelMinMaxObserver, so none of the per-channel kernels' branches take it.
"""
from __future__ import annotations

import torch

from ..fakequant import PerGroupObserveFQFn, check_group_size, per_group_observe_fq
from ..utils.registry import register_class
from .base import BaseObserver


@register_class
class PerGroupMinMaxObserver(BaseObserver):
    axis = 0
    #: QuantizationManager / FakeQuantize: refused as an activation observer
    weights_only = True

    def __init__(self, symmetric=True, num_bits=8, eps=1e-8, group_size=128):
        self.symmetric = symmetric
        self.eps = eps
        self.num_bits = num_bits
        self._group_size = check_group_size(group_size)
        self.run_min = None   # fp32 [rows, groups] on the tensor's device
        self.run_max = None
        self.scale = None     # f64 [rows, groups] from the last observe
        self.zero_point = None

    @property
    def group_size(self) -> int:
        return self._group_size

    @group_size.setter
    def group_size(self, g):
        g = check_group_size(g)
        if g != self._group_size:
            self._group_size = g
            self.reset()   # the running state is per group

    # ------------------------------------------------------------------ state
    @property
    def min_val(self):
        return None if self.run_min is None else self.run_min.to(torch.float64)

    @property
    def max_val(self):
        return None if self.run_max is None else self.run_max.to(torch.float64)

    def _state(self, x):
        rows = x.shape[0] if x.dim() > 0 else 1
        ngr = -(-(x.numel() // max(rows, 1)) // self._group_size)
        if self.run_min is None or tuple(self.run_min.shape) != (rows, ngr) or self.run_min.device != x.device:
            state = torch.zeros(2, rows, ngr, dtype=torch.float32, device=x.device)   # one fill
            self.run_min, self.run_max = state[0], state[1]
        return self.run_min, self.run_max

    def reset(self):
        self.run_min = self.run_max = self.scale = self.zero_point = None

    @staticmethod
    def _check(x):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            what = x.dtype if isinstance(x, torch.Tensor) else type(x).__name__
            raise TypeError(f"PerGroupMinMaxObserver: only float32 tensors are supported, got {what}")
        return x

    # ------------------------------------------------------------------ protocol
    def observe(self, x):
        x = self._check(x).detach()
        mn, mx = self._state(x)
        r = per_group_observe_fq(x, group_size=self._group_size, symmetric=self.symmetric, qmin=0, qmax=0,
                                 obs_bits=self.num_bits, eps=self.eps, run_min=mn, run_max=mx, quantize=False)
        self.scale, self.zero_point = r["scale"], r["zp"]

    def get_scale_zero_point(self):
        """(scale f64[rows, groups], zero_point f64[rows, groups]) from the running state."""
        if self.scale is None:
            raise RuntimeError("PerGroupMinMaxObserver: nothing observed yet")
        return self.scale, self.zero_point

    def forward(self, x):
        self.observe(x)
        return self.get_scale_zero_point()

    def observe_quantize(self, x, quantizer):
        """Fused observe + fake quant of ``x`` on ``quantizer``'s integer range, one pass; y
        carries the STE gradient."""
        x = self._check(x)
        mn, mx = self._state(x)
        args = dict(group_size=self._group_size, symmetric=self.symmetric, qmin=quantizer.qmin, qmax=quantizer.qmax,
                    obs_bits=self.num_bits, eps=self.eps, run_min=mn, run_max=mx)
        if x.requires_grad and torch.is_grad_enabled():
            y, s, z = PerGroupObserveFQFn.apply(x, args["group_size"], args["symmetric"], args["qmin"], args["qmax"],
                                                args["obs_bits"], args["eps"], mn, mx)
        else:
            r = per_group_observe_fq(x, **args)
            y, s, z = r["y"], r["scale"], r["zp"]
        self.scale, self.zero_point = s, z
        return y

    def __repr__(self):
        return (f"PerGroupMinMaxObserver(symmetric={self.symmetric}, num_bits={self.num_bits}, eps={self.eps}, "
                f"group_size={self._group_size})")
