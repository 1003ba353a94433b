"""Shared by tests/test_adaround_cpu.py and tests/test_gpu_adaround.py: a numpy restatement
of AdaRound's arithmetic (include/vsiq.h, "AdaRound"), the input builders and the
comparisons.  Nothing here touches a GPU.

The oracle does not re-derive the fp32 exponential: it takes the library's own h bits from
the host loop with s = 1, z = 0, w = 0, lo = 0, hi = 1 (then y == h exactly), and the
library's own h' bits from the host backward with the same qparams, g = 1 and lambda = 0
(then grad_V == h' exactly: (1 * 1 * 1 + 0) * h').  Everything downstream -- the quotient,
floor, clamp, dequantise, mask, regulariser, its derivative and the gradient's single
rounding -- is restated here; h and h' themselves are pinned against an f64 closed form
in test_adaround_cpu.py."""
import numpy as np
import torch

from vsiquantization_amd.fakequant import adaround_backward, adaround_forward

F32 = np.float32
F64 = np.float64

# one workgroup: 256 lanes x 2 groups x 4 elements of one row (kBlock * kFlatU * 4)
WG_SPAN = 2048
N_FLAT = (1, 5, 1023, WG_SPAN + 1)
SHAPES_PC = ((1, 7), (64, 27), (128, 9), (3, 1030), (8, WG_SPAN + 4))
# the regulariser's fold takes another path above 128 and above 2048 workgroups
SHAPES_FOLD = ((130, 5), (2050, 3))
GRIDS = tuple((bits, sym) for bits in (2, 4, 8) for sym in (True, False))
BETAS = (2.0, 3.7, 20.0)


def grid(bits, symmetric):
    return (-(2 ** (bits - 1)), 2 ** (bits - 1) - 1) if symmetric else (0, 2 ** bits - 1)


def bits_equal(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ulp_distance(a, b):
    """Elementwise distance in fp32 ulps (finite values; +0 and -0 coincide)."""
    def key(x):
        i = np.ascontiguousarray(x, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def make_case(rows, rowlen, bits, symmetric, per_row, seed):
    """(w, V, g fp32 [rows, rowlen]; scale f64 [nq]; zp f64 [nq] | None; lo; hi): weights whose
    range slightly exceeds the grid (both clamp edges are hit), V across the sigmoid's
    rectified range and beyond it."""
    rng = np.random.default_rng(seed)
    lo, hi = grid(bits, symmetric)
    w = (rng.standard_normal((rows, rowlen)) * 0.05).astype(F32)
    nq = rows if per_row else 1
    if symmetric:
        scale = (0.11 / hi) * (1.0 + 0.3 * rng.random(nq))
        zp = None
    else:
        scale = (0.22 / (hi - lo)) * (1.0 + 0.3 * rng.random(nq))
        zp = np.rint((hi - lo) * (0.4 + 0.2 * rng.random(nq)))
    V = (rng.uniform(-4.0, 4.0, (rows, rowlen))).astype(F32)
    g = rng.standard_normal((rows, rowlen)).astype(F32)
    return w, V, g, scale.astype(F64), (None if zp is None else zp.astype(F64)), lo, hi


def qp32(scale, zp, rows):
    """fp32 (s, z) per row, broadcast from nq = 1."""
    s = np.broadcast_to(np.asarray(scale, F64).reshape(-1).astype(F32), (rows,)) if np.size(scale) == 1 \
        else np.asarray(scale, F64).astype(F32)
    if zp is None:
        z = np.zeros(rows, F32)
    else:
        z = np.broadcast_to(np.asarray(zp, F64).reshape(-1).astype(F32), (rows,)) if np.size(zp) == 1 \
            else np.asarray(zp, F64).astype(F32)
    return s.reshape(rows, 1), z.reshape(rows, 1)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def lib_h(V):
    """The library's h bits: host soft forward, w = 0, s = 1, z = 0, grid [0, 1]."""
    v = torch.from_numpy(np.ascontiguousarray(V, dtype=F32).reshape(1, -1))
    y, _ = adaround_forward(torch.zeros_like(v), v, 1.0, 0.0, 0, 1)
    return y.numpy().reshape(np.shape(V))


def lib_hp(V):
    """The library's h' bits: host backward, g = 1, w = 0, s = 1, z = 0, grid [0, 1], lambda = 0."""
    v = torch.from_numpy(np.ascontiguousarray(V, dtype=F32).reshape(1, -1))
    gv = adaround_backward(torch.ones_like(v), torch.zeros_like(v), v, 1.0, 0.0, 0, 1, lam=0.0, beta=2.0)
    return gv.numpy().reshape(np.shape(V))


def h64(V):
    """f64 closed form of the rectified sigmoid and its derivative (exact constants)."""
    v = np.asarray(V, F64)
    with np.errstate(all="ignore"):
        sig = 1.0 / (1.0 + np.exp(-v))
    hr = 1.2 * sig - 0.1
    h = np.clip(hr, 0.0, 1.0)
    hp = np.where((hr > 0) & (hr < 1), 1.2 * sig * (1 - sig), 0.0)
    return np.where(np.isnan(v), 0.0, h), np.where(np.isnan(v), 0.0, hp)


def oracle_forward(w, V, scale, zp, lo, hi, hard=False, h=None):
    """(y fp32, m bool, r fp32) of [rows, rowlen] inputs; h: the library's bits (soft)."""
    rows = w.shape[0]
    s, z = qp32(scale, zp, rows)
    with np.errstate(all="ignore"):
        t = (w / s).astype(F32) + z          # RN(RN(w/s) + z): numpy fp32 ops are IEEE
        b = np.floor(t)
        if hard:
            hh = np.where(V >= 0, F32(1), F32(0)).astype(F32)   # NaN >= 0 is False
        else:
            hh = lib_h(V) if h is None else h
        r = (b + hh).astype(F32)
        c = np.where(r < lo, F32(lo), np.where(r > hi, F32(hi), r)).astype(F32)   # NaN propagates
        y = ((c - z).astype(F32) * s).astype(F32)
        m = (r >= lo) & (r <= hi)
    return y, m, r


def _pow1(u, e):
    with np.errstate(all="ignore"):
        return np.where(u == 1.0, 1.0, np.power(u, e))


def oracle_reg(h, beta):
    """R = sum(1 - |2h - 1|^beta) in f64 from the fp32 h."""
    u = np.abs(2.0 * h.astype(F64) - 1.0)
    return float(np.sum(1.0 - _pow1(u, beta)))


def oracle_dreg(h, beta):
    d = 2.0 * h.astype(F64) - 1.0
    u = np.abs(d)
    return np.where(u == 0.0, 0.0, ((-2.0 * beta) * np.where(d > 0, 1.0, -1.0)) * _pow1(u, beta - 1.0))


def oracle_grad(g, w, V, scale, zp, lo, hi, lam, beta, h=None, hp=None):
    """grad_V = fp32(((double)g (double)s m + lam dR/dh) (double)h'), rounded once."""
    rows = w.shape[0]
    h = lib_h(V) if h is None else h
    hp = lib_hp(V) if hp is None else hp
    s, _ = qp32(scale, zp, rows)
    _, m, _ = oracle_forward(w, V, scale, zp, lo, hi, h=h)
    with np.errstate(all="ignore"):
        dy = (g.astype(F64) * s.astype(F64)) * np.where(m, 1.0, 0.0)
        return ((dy + lam * oracle_dreg(h, beta)) * hp.astype(F64)).astype(F32)


def run(w, V, scale, zp, lo, hi, per_row, device="cpu", **kw):
    """adaround_forward on `device` from numpy inputs; a flat (per-tensor) case is one row."""
    axis = 0 if per_row else None
    return adaround_forward(_t(w).to(device), _t(V).to(device), _t(scale), _t(zp), lo, hi, axis=axis, **kw)


def run_bwd(g, w, V, scale, zp, lo, hi, per_row, device="cpu", **kw):
    axis = 0 if per_row else None
    return adaround_backward(_t(g).to(device), _t(w).to(device), _t(V).to(device), _t(scale), _t(zp), lo, hi,
                             axis=axis, **kw)


def build_layer(seed, device="cpu", bits=4):
    """One fused conv layer (BN folded, ReLU) with per-channel `bits`-bit weights whose weight
    quantizer has observed its qparams once, and its input [4, 3, 12, 12]; fixed seed."""
    import torch.nn as nn

    from vsiquantization_amd.modules.fused import ConvBnReLU
    gen = torch.Generator().manual_seed(seed)
    cv = nn.Conv2d(3, 8, 3, padding=1)
    bn = nn.BatchNorm2d(8)
    with torch.no_grad():
        cv.weight.copy_(torch.randn(cv.weight.shape, generator=gen) * 0.2)
        cv.bias.copy_(torch.randn(8, generator=gen) * 0.1)
        bn.weight.copy_(1.0 + 0.2 * torch.rand(8, generator=gen))
        bn.running_var.copy_(0.5 + torch.rand(8, generator=gen))
        bn.running_mean.copy_(0.1 * torch.randn(8, generator=gen))
    layer = ConvBnReLU(cv, bn, nn.ReLU(), "PerChannelMSEObserver", "PerChannelUniformQuantizer",
                       "MinMaxObserver", "UniformQuantizer", True, True, True, bits, 8).to(device)
    x = torch.randn((4, 3, 12, 12), generator=gen).to(device)
    wq = layer.weight_quantizer
    wq.is_learning_scale = False
    wq.quantize(layer.get_weight_bias()[0].detach())   # observe: per-channel scale / zero point
    return layer, x


def all_cases():
    """(tag, rows, rowlen, per_row) over the flat sizes and the per-channel shapes."""
    out = [(f"flat{n}", 1, n, False) for n in N_FLAT]
    out += [(f"pc{r}x{c}", r, c, True) for r, c in SHAPES_PC]
    return out
