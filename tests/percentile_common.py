"""Shared by tests/test_percentile_cpu.py and tests/test_gpu_percentile.py: the numpy oracle
of PercentileObserver's definition (include/vsiq.h, vsiq_act_observe_hist_f32) in float64
with integer counts, the input families and bit-level comparisons.  Nothing here touches a
GPU."""
import math

import numpy as np
import torch

from vsiquantization_amd import _hip as H
from vsiquantization_amd.fakequant import qden

BINS = (256, 2048, 4096)
PERCENTILES = (99.0, 99.99, 100)
OUTLIER = 1e4


def tail_of(percentile):
    return (100.0 - percentile) / 100.0


def oracle_clip(v, mn, mx, tail, bins):
    """(lo, hi) as np.float32 of one call on the fp32 array ``v`` (already activated) whose K2
    record holds ``mn`` / ``mx`` (np.float32): steps 2-4 of the definition."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    nan = int(np.isnan(v).sum())
    mn, mx = np.float32(mn), np.float32(mx)
    if nan > 0 or mn == mx or not np.isfinite(mn) or not np.isfinite(mx) or tail == 0:
        return mn, mx
    N = v.size - nan
    dmn, dmx = np.float64(mn), np.float64(mx)
    W = dmx - dmn
    invw = np.float64(bins) / W
    step = W / np.float64(bins)
    b = np.minimum(bins - 1, ((v.astype(np.float64) - dmn) * invw).astype(np.int64))
    h = np.bincount(b, minlength=bins).astype(np.uint64)
    K = int(math.floor(float(N) * tail))
    bl = int(np.argmax(np.cumsum(h) > K))
    bh = bins - 1 - int(np.argmax(np.cumsum(h[::-1]) > K))
    assert bl <= bh
    lo = mn if bl == 0 else max(mn, np.float32(dmn + np.float64(bl) * step))
    hi = mx if bh == bins - 1 else min(mx, np.float32(dmn + np.float64(bh + 1) * step))
    return np.float32(lo), np.float32(hi)


class OracleObserver:
    """The running update (strict compares from the int 0 / 0 start, a NaN call changes
    nothing: minmax.py:42-47) and the f64 qparams (minmax.py:49-74) on clipped ranges."""

    def __init__(self, symmetric, num_bits=8, eps=1e-8):
        self.symmetric, self.num_bits, self.eps = symmetric, num_bits, eps
        self.mn = np.float32(0.0)
        self.mx = np.float32(0.0)

    def update(self, lo, hi, has_nan):
        if not has_nan:
            if lo < self.mn:
                self.mn = np.float32(lo)
            if hi > self.mx:
                self.mx = np.float32(hi)

    def qparams(self):
        """(scale, zero point) as Python floats, the device record's f64 values."""
        mn, mx = float(self.mn), float(self.mx)
        den = qden(self.symmetric, self.num_bits, self.eps)
        if self.symmetric:
            return max(abs(mn), abs(mx)) / den, 0.0
        s = (mx - mn) / den
        v = -mn / (s + self.eps)
        z = float(round(v)) if math.isfinite(v) else float("nan")
        return s, z + 0.0

    def qp_record(self):
        s, z = self.qparams()
        return np.array([s, z, float(self.mn), float(self.mx)], dtype=np.float64)


def k2_minmax(st):
    """(mn, mx, has_nan) of a stats record (tensor f64[ST_LEN], any device)."""
    st = st.cpu()
    return np.float32(float(st[H.ST_MIN])), np.float32(float(st[H.ST_MAX])), float(st[H.ST_NAN]) > 0


def same_bits(a, b):
    """Bit equality of two float arrays / tensors of one dtype (NaN == NaN, -0.0 != 0.0)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return a.tobytes() == b.tobytes()


FAMILIES = ("outliers", "relu", "constant", "nan", "inf", "denormal")


def make_input(family, n, seed):
    """fp32 CPU tensor of ``n`` elements."""
    g = torch.Generator().manual_seed(1000 * seed + n % 997)
    x = torch.randn(n, generator=g) * 3
    if family in ("outliers", "relu"):
        k = min(10, n)
        idx = torch.randperm(n, generator=g)[:k]
        sign = torch.where(torch.arange(k) % 2 == 0, 1.0, -1.0)
        x[idx] = sign * OUTLIER
        if family == "relu":
            x = torch.relu(x)
    elif family == "constant":
        x = torch.full((n,), 1.5 + seed)
    elif family == "nan":
        x[n // 2] = float("nan")
    elif family == "inf":
        x[n // 3] = float("inf")
    elif family == "denormal":
        x = x * 1e-41   # fp32 denormals
        x[::2] = -0.0
        if n > 1:
            x[1] = 1e-39
    return x.contiguous()
