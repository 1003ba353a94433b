"""MSEObserver: MinMaxObserver whose per-call range is shrunk to the least quantization error.

MinMaxObserver and PercentileObserver set the range from order statistics alone; at 2 to 4
bits the range that minimises the quantization error lies well inside the min / max even
on clean data.  Here each call tries ``candidates`` ranges ``ratios[k] * (min, max)`` of
that call (geometric ratios from 1 down to ``min_ratio``), fake-quantizes the call's values
with the qparams of each on the quantizer's own grid, sums the squared errors in f64 and
keeps the range of the smallest sum (ties: the widest); that range goes through
MinMaxObserver's running update and f64 qparams unchanged.  include/vsiq.h states the
definition.  ``candidates=1`` is MinMaxObserver bit for bit.

Two passes over the tensor on the device (K2 for the stats record, then the search pass,
csrc/k_observe_mse.hip: one read serves every candidate), no host sync, capturable in a HIP
graph; a CPU tensor takes the native host loops.  fp32 only, per tensor, single GPU.
"""
from __future__ import annotations

import torch

from .. import _hip as H
from .. import host
from ..fakequant import check_mse_ratios, mse_ratios, observe_mse
from ..utils.registry import register_class
from .minmax import MinMaxObserver


@register_class
class MSEObserver(MinMaxObserver):
    # two passes per call: QuantizationManager keeps it off the single-pass fusions
    # (K8 / K9, K2o, the deferred K2p / K2m records, the multi-GPU exchange)
    single_pass = False
    # QuantizationManager sets num_bits = bits_width after construction: the errors are
    # those of the grid the quantizer uses (the reference-parity observers stay 8-bit)
    follows_bits_width = True

    def __init__(self, symmetric=True, num_bits=8, eps=1e-8, candidates=64, min_ratio=2 ** -8, ratios=None):
        super().__init__(symmetric, num_bits, eps)
        self.candidates = candidates
        self.min_ratio = min_ratio
        self.ratios = check_mse_ratios(ratios) if ratios is not None else mse_ratios(candidates, min_ratio)
        if ratios is not None:
            self.candidates = len(self.ratios)
        self.last_errors = None   # f64[candidates] of the last call, on its device (no sync)
        self.last_pick = None     # int32[1]

    def grid(self):
        """(qmin, qmax) of UniformQuantizer(num_bits, symmetric)."""
        if self.symmetric:
            return -(2 ** (self.num_bits - 1)), 2 ** (self.num_bits - 1) - 1
        return 0, 2 ** self.num_bits - 1

    def observe_device(self, x, want_stats=True, want_qp=True, act=None):
        """K2 + the search pass: update the running state from the chosen range, return
        (qp f64[4], stats f64[10]) on x.device; the stats are the whole tensor's."""
        if host.is_host(x):   # CPU tensor: a CPU fp32[2] state and no observer stream to join
            dev = x.device
        else:
            dev = H.require_device_f32(x).device
            if self._obs_stream is not None and self._obs_stream != torch.cuda.current_stream(dev):
                self._join()
        state = self.device_state(dev)
        qmin, qmax = self.grid()
        qp, st, _, self.last_errors, self.last_pick = observe_mse(
            x, symmetric=self.symmetric, num_bits=self.num_bits, eps=self.eps, run_minmax=state, ratios=self.ratios,
            qmin=qmin, qmax=qmax, act=act)
        self._dirty = True
        return qp, st

    def __repr__(self):
        return (f"MSEObserver(symmetric={self.symmetric}, num_bits={self.num_bits}, eps={self.eps}, "
                f"candidates={self.candidates}, min_ratio={self.min_ratio})")
