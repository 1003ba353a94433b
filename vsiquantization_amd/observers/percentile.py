"""PercentileObserver: MinMaxObserver whose per-call range is clipped to a percentile.

MinMaxObserver sets the range from the single largest element ever seen; at 4 bits one
outlier in a 50M-element activation costs most of the 16 levels.  Here each call's
``(min, max)`` is first clipped to the ``percentile`` of that call's values (each end of
the range may lose up to ``floor(N * (100 - percentile) / 100)`` elements, found in a
``bins``-bin histogram between the call's min and max; include/vsiq.h states the
definition), and the clipped pair goes through MinMaxObserver's running update and f64
qparams unchanged.  ``percentile=100`` is MinMaxObserver bit for bit.

Two passes over the tensor on the device (K2 for the stats record, then the histogram
pass, csrc/k_observe_hist.hip), no host sync, capturable in a HIP graph; a CPU tensor takes
the native host loops.  The histogram holds integer counts, so GPU, CPU and a numpy
restatement agree bit for bit.  fp32 only, per tensor, single GPU.
"""
from __future__ import annotations

import torch

from .. import _hip as H
from .. import host
from ..fakequant import observe_percentile, percentile_tail
from ..utils.registry import register_class
from .minmax import MinMaxObserver


@register_class
class PercentileObserver(MinMaxObserver):
    # two passes per call: QuantizationManager keeps it off the single-pass fusions
    # (K8 / K9, K2o, the deferred K2p / K2m records, the multi-GPU exchange)
    single_pass = False

    def __init__(self, symmetric=True, num_bits=8, eps=1e-8, percentile=99.99, bins=2048):
        super().__init__(symmetric, num_bits, eps)
        self.percentile = percentile
        self.bins = bins

    def observe_device(self, x, want_stats=True, want_qp=True, act=None):
        """K2 + the histogram pass: update the running state from the clipped range, return
        (qp f64[4], stats f64[10]) on x.device; the stats are the unclipped tensor's."""
        if host.is_host(x):   # CPU tensor: a CPU fp32[2] state and no observer stream to join
            dev = x.device
        else:
            dev = H.require_device_f32(x).device
            if self._obs_stream is not None and self._obs_stream != torch.cuda.current_stream(dev):
                self._join()
        state = self.device_state(dev)
        qp, st, _ = observe_percentile(x, symmetric=self.symmetric, num_bits=self.num_bits, eps=self.eps,
                                       run_minmax=state, tail=percentile_tail(self.percentile), bins=self.bins,
                                       act=act)
        self._dirty = True
        return qp, st

    def __repr__(self):
        return (f"PercentileObserver(symmetric={self.symmetric}, num_bits={self.num_bits}, eps={self.eps}, "
                f"percentile={self.percentile}, bins={self.bins})")
