"""Shared by tests/test_mse_cpu.py and tests/test_gpu_mse.py: the numpy oracle of MSEObserver's
definition (include/vsiq.h, vsiq_act_observe_mse_f32) -- fp32 element values, every E_k the
math.fsum of its float64 terms, qparams through percentile_common.OracleObserver -- the
input families, the margin of a search and the comparisons.  Nothing here touches a GPU."""
import math

import numpy as np
import torch

from oracle import fakequant_np as O
from tests.percentile_common import OracleObserver, k2_minmax, make_input as percentile_input, same_bits  # noqa: F401
from vsiquantization_amd.fakequant import mse_ratios

REL = 1e-9        # every E_k against the fsum oracle: the project's bar for its f64 sums
MARGIN = 1e-6     # bit-equality of the pick needs the two smallest E_k further apart than this
HEAVY = 30.0

FAMILIES = ("gauss", "heavy", "relu", "constant", "nan", "inf", "denormal", "ongrid")
# ongrid: three candidates that round to one fp32 range (exact ties), then real ones
ONGRID_RATIOS = (1.0, 1.0 - 2.0 ** -40, 1.0 - 2.0 ** -35, 0.75, 0.5, 0.25)


def grid_of(num_bits, symmetric):
    """UniformQuantizer's (qmin, qmax)."""
    return O.qrange(num_bits, symmetric)


def make_input(family, n, seed):
    """fp32 CPU tensor of ``n`` elements."""
    if family in ("constant", "nan", "inf", "denormal"):
        return percentile_input(family, n, seed)
    g = torch.Generator().manual_seed(1000 * seed + n % 997)
    if family == "ongrid":   # integers x 0.5 in [-63.5, 64]: the asymmetric 8-bit grid holds them exactly
        x = torch.randint(-127, 129, (n,), generator=g).float() * 0.5
        x[0] = -63.5
        if n > 1:
            x[1] = 64.0
        return x.contiguous()
    x = torch.randn(n, generator=g) * 3
    if family in ("heavy", "relu"):
        k = min(10, n)
        idx = torch.randperm(n, generator=g)[:k]
        x[idx] = torch.where(torch.arange(k) % 2 == 0, 1.0, -1.0) * HEAVY
        if family == "relu":
            x = torch.relu(x)
    return x.contiguous()


def ratios_of(family, count=64):
    """The default geometric table; denormal: down to 2^-24, where the fp32 scale of a 1e-39
    range underflows to 0 and the candidates go invalid; ongrid: its own."""
    if family == "ongrid":
        return ONGRID_RATIOS
    return mse_ratios(count, 2.0 ** -24) if family == "denormal" else mse_ratios(count)


def candidate(mn, mx, r, symmetric, num_bits, eps=1e-8):
    """(lo, hi, s32, z32, valid) of one candidate: the qparams a fresh observer returns."""
    lo = np.float32(np.float64(mn) * np.float64(r))
    hi = np.float32(np.float64(mx) * np.float64(r))
    obs = OracleObserver(symmetric, num_bits, eps)
    obs.update(lo, hi, False)
    with np.errstate(all="ignore"):
        s, z = obs.qparams()
        s32, z32 = np.float32(s), np.float32(z)
    valid = bool(np.isfinite(s32)) and s32 > 0 and math.isfinite(z)
    return lo, hi, s32, z32, valid


def oracle_search(v, mn, mx, has_nan, ratios, symmetric, num_bits, eps=1e-8):
    """(lo, hi, E list, pick) of one call on the fp32 array ``v`` (already activated) whose K2
    record holds ``mn`` / ``mx`` (np.float32) and the NaN flag."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    mn, mx = np.float32(mn), np.float32(mx)
    K = len(ratios)
    E = [math.inf] * K
    if has_nan or mn == mx or not np.isfinite(mn) or not np.isfinite(mx) or K == 1:
        return mn, mx, E, 0
    qmin, qmax = grid_of(num_bits, symmetric)
    v64 = v.astype(np.float64)
    cands = [candidate(mn, mx, r, symmetric, num_bits, eps) for r in ratios]
    for k, (_, _, s32, z32, valid) in enumerate(cands):
        if not valid:
            continue
        y = O.fq_forward(v, s32, z32, qmin, qmax)[0]
        with np.errstate(all="ignore"):
            d = y.astype(np.float64) - v64
            t = d * d
        E[k] = math.fsum(t.tolist()) if np.isfinite(t).all() else float(np.sum(t))
    pick = 0
    for k in range(1, K):
        if E[k] < E[pick]:
            pick = k
    return cands[pick][0], cands[pick][1], E, pick


def margin(E):
    """(E_second - E_best) / E_best over the finite-or-inf list E; 0.0 for an exact tie (also
    all zero, all inf), inf for a zero best with a non-zero second."""
    if len(E) < 2:
        return 0.0
    s = sorted(E)
    best, second = s[0], s[1]
    if second == best:
        return 0.0
    if best == 0.0 or math.isinf(second):
        return math.inf
    return (second - best) / best


def decidable(E):
    """The precondition of comparing picks bit for bit: a clear margin or an exact tie."""
    m = margin(E)
    return m > MARGIN or m == 0.0


def errors_close(got, want):
    """Every E_k within REL of the oracle's: inf matches inf, 0 matches 0 exactly."""
    got = [float(g) for g in (got.detach().cpu().tolist() if isinstance(got, torch.Tensor) else got)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if math.isinf(w) or w == 0.0:
            if g != w:
                return False
        elif not abs(g - w) <= REL * w:
            return False
    return True
