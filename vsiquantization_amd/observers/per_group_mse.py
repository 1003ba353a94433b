"""PerGroupMSEObserver: PerGroupMinMaxObserver whose per-group range is shrunk to the least
quantization error.

Group-wise quantization exists for 2- to 4-bit weights, and that is where a group's plain
min / max spends its few levels on one outlier.  Here every group (r, j) of
PerGroupMinMaxObserver's view is searched as PerChannelMSEObserver searches a row holding the
group's elements: ``candidates`` ranges ``ratios[k] * (min, max)`` of that call, each scored by
the f64 sum of squared errors of fake-quantizing the group on the quantizer's own grid, the
smallest (ties: the widest) through the group's running update and f64 qparams.  A group that
holds a NaN, is constant (a one-element last group included) or not finite is
PerGroupMinMaxObserver's; one group's fallback never affects another.  include/vsiq.h states
the definition.  ``candidates=1`` is PerGroupMinMaxObserver bit for bit.

One launch and one read of the tensor on the device (csrc/k_pg_mse.hip), no host sync,
capturable in a HIP graph; a CPU tensor takes the native host loops.  Weights only, fp32 only.
Because it is a PerGroupMinMaxObserver, QuantizationManager pairs it with
PerGroupUniformQuantizer and PerGroupLSQQuantizer as it pairs its parent.
"""
from __future__ import annotations

import torch

from ..fakequant import PerGroupObserveMSEFn, check_mse_ratios, mse_ratios, per_group_observe_mse
from ..utils.registry import register_class
from .per_group import PerGroupMinMaxObserver


@register_class
class PerGroupMSEObserver(PerGroupMinMaxObserver):
    # QuantizationManager sets num_bits = bits_width after construction: the errors are those
    # of the grid the quantizer uses
    follows_bits_width = True

    def __init__(self, symmetric=True, num_bits=8, eps=1e-8, group_size=128, candidates=64, min_ratio=2 ** -8,
                 ratios=None):
        super().__init__(symmetric, num_bits, eps, group_size)
        self.candidates = candidates
        self.min_ratio = min_ratio
        self.ratios = check_mse_ratios(ratios) if ratios is not None else mse_ratios(candidates, min_ratio)
        if ratios is not None:
            self.candidates = len(self.ratios)
        #: keep every candidate's error of the last call (f64 [rows, groups, candidates]: at 64
        #: candidates and g32 sixteen times the tensor's bytes, so only when asked)
        self.want_errors = False
        self.last_errors = None   # None unless want_errors
        self.last_pick = None     # int32 [rows, groups] of the last call, on its device (no sync)

    def reset(self):
        super().reset()
        self.last_errors = self.last_pick = None

    def grid(self):
        """(qmin, qmax) of PerGroupUniformQuantizer(num_bits, symmetric)."""
        if self.symmetric:
            return -(2 ** (self.num_bits - 1)), 2 ** (self.num_bits - 1) - 1
        return 0, 2 ** self.num_bits - 1

    def _args(self, x, qmin, qmax):
        mn, mx = self._state(x)
        return dict(group_size=self._group_size, symmetric=self.symmetric, qmin=qmin, qmax=qmax,
                    num_bits=self.num_bits, eps=self.eps, run_min=mn, run_max=mx, ratios=self.ratios,
                    want_errors=self.want_errors)

    # ------------------------------------------------------------------ protocol
    def observe(self, x):
        x = self._check(x).detach()
        r = per_group_observe_mse(x, quantize=False, **self._args(x, *self.grid()))
        self.scale, self.zero_point = r["scale"], r["zp"]
        self.last_errors, self.last_pick = r["err"], r["pick"]

    def observe_quantize(self, x, quantizer):
        """Fused observe + search + fake quant of ``x`` on ``quantizer``'s integer range (one
        launch, one read); y carries the STE gradient."""
        x = self._check(x)
        a = self._args(x, quantizer.qmin, quantizer.qmax)
        if x.requires_grad and torch.is_grad_enabled():
            y, s, z, pick, err = PerGroupObserveMSEFn.apply(x, a["group_size"], a["symmetric"], a["qmin"], a["qmax"],
                                                            a["num_bits"], a["eps"], a["run_min"], a["run_max"],
                                                            a["ratios"], a["want_errors"])
            err = err if self.want_errors else None
        else:
            r = per_group_observe_mse(x, **a)
            y, s, z, pick, err = r["y"], r["scale"], r["zp"], r["pick"], r["err"]
        self.scale, self.zero_point = s, z
        self.last_errors, self.last_pick = err, pick
        return y

    def __repr__(self):
        return (f"PerGroupMSEObserver(symmetric={self.symmetric}, num_bits={self.num_bits}, eps={self.eps}, "
                f"group_size={self._group_size}, candidates={self.candidates}, min_ratio={self.min_ratio})")
