"""PerChannelMSEObserver: PerChannelMinMaxObserver whose per-row range is shrunk to the least
quantization error.

Weights at 2 to 4 bits are where a per-channel, error-minimising range matters most: a
per-row min / max spends most of its few levels on a row's one or two outliers.  Here every
out-channel row W[c] (axis 0) is searched as MSEObserver searches a tensor: ``candidates``
ranges ``ratios[k] * (min_c, max_c)`` of that call, each scored by the f64 sum of squared
errors of fake-quantizing the row on the quantizer's own grid, the smallest (ties: the
widest) through the row's running update and f64 qparams.  A row that holds a NaN, is
constant or not finite is PerChannelMinMaxObserver's; one row's fallback never affects
another.  include/vsiq.h states the definition.  ``candidates=1`` is PerChannelMinMaxObserver
bit for bit.

One launch and one read of the tensor on the device (csrc/k_pc_mse.hip: min / max, search,
running update, qparams and optionally the fake-quantized output), no host sync, capturable
in a HIP graph; a CPU tensor takes the native host loops.  fp32 only, axis 0 only.
"""
from __future__ import annotations

import torch

from .. import _hip as H
from .. import host as _host
from ..fakequant import PerChannelObserveMSEFn, check_mse_ratios, mse_ratios, per_channel_observe_mse
from ..utils.registry import register_class
from .per_channel import PerChannelMinMaxObserver


@register_class
class PerChannelMSEObserver(PerChannelMinMaxObserver):
    # QuantizationManager sets num_bits = bits_width after construction: the errors are
    # those of the grid the quantizer uses
    follows_bits_width = True

    def __init__(self, symmetric=True, num_bits=8, eps=1e-8, candidates=64, min_ratio=2 ** -8, ratios=None):
        super().__init__(symmetric, num_bits, eps)
        self.candidates = candidates
        self.min_ratio = min_ratio
        self.ratios = check_mse_ratios(ratios) if ratios is not None else mse_ratios(candidates, min_ratio)
        if ratios is not None:
            self.candidates = len(self.ratios)
        self.last_errors = None   # f64[C, candidates] of the last call, on its device (no sync)
        self.last_pick = None     # int32[C]

    def reset(self):
        super().reset()
        self.last_errors = self.last_pick = None

    def grid(self):
        """(qmin, qmax) of PerChannelUniformQuantizer(num_bits, symmetric)."""
        if self.symmetric:
            return -(2 ** (self.num_bits - 1)), 2 ** (self.num_bits - 1) - 1
        return 0, 2 ** self.num_bits - 1

    def _check(self, x):
        # before _state, which drops the running min / max when the device changes
        return x if _host.is_host(x) else H.require_device_f32(x)

    # ------------------------------------------------------------------ protocol
    # both entry points are overridden: the parent's bound C++ op (_op) is plain min / max
    # and is never taken here
    def observe(self, x, want_row_stats=False):
        x = self._check(x)
        mn, mx = self._state(x)
        qmin, qmax = self.grid()
        r = per_channel_observe_mse(x, symmetric=self.symmetric, qmin=qmin, qmax=qmax, num_bits=self.num_bits,
                                    eps=self.eps, run_min=mn, run_max=mx, ratios=self.ratios, quantize=False,
                                    want_row_stats=want_row_stats)
        self.scale, self.zero_point = r["scale"], r["zp"]
        self.last_errors, self.last_pick = r["err"], r["pick"]
        return r["row_stats"]

    def observe_quantize(self, x, quantizer, want_row_stats=False):
        """Fused observe + search + fake quant of ``x`` on ``quantizer``'s integer range (one
        launch, one read).  Returns (y, row_stats | None); y carries the STE gradient."""
        x = self._check(x)
        mn, mx = self._state(x)
        if x.requires_grad and torch.is_grad_enabled():
            y, s, z, rs, err, pick = PerChannelObserveMSEFn.apply(x, self.symmetric, quantizer.qmin, quantizer.qmax,
                                                                  self.num_bits, self.eps, mn, mx, self.ratios,
                                                                  want_row_stats)
            rs = rs if want_row_stats else None
        else:
            r = per_channel_observe_mse(x, symmetric=self.symmetric, qmin=quantizer.qmin, qmax=quantizer.qmax,
                                        num_bits=self.num_bits, eps=self.eps, run_min=mn, run_max=mx,
                                        ratios=self.ratios, want_row_stats=want_row_stats)
            y, s, z, rs, err, pick = r["y"], r["scale"], r["zp"], r["row_stats"], r["err"], r["pick"]
        self.scale, self.zero_point = s, z
        self.last_errors, self.last_pick = err, pick
        return y, rs

    def get_scale_zero_point(self):
        if self.scale is None:
            raise RuntimeError("PerChannelMSEObserver: nothing observed yet")
        return self.scale, self.zero_point

    def __repr__(self):
        return (f"PerChannelMSEObserver(symmetric={self.symmetric}, num_bits={self.num_bits}, eps={self.eps}, "
                f"candidates={self.candidates}, min_ratio={self.min_ratio}, axis=0)")
