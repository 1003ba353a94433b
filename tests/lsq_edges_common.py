"""Inputs and the one comparison of the learnable-backward edge tests
(tests/test_lsq_edges_cpu.py, tests/test_gpu_lsq_edges.py, tests/golden/gen_goldens.py).

The learnable (LSQ) backward is autograd of quantizers/uniform.py:47-56 in closed form.
These builders plant, among ordinary randn data, the values at which a closed form can
leave the reference: signed zeros, denormals, NaN and infinities in x and in the incoming
gradient, exact rounding ties (k + 0.5) * s, x on and one ulp either side of the clamp
bounds, a gradient whose product with the scale overflows, learned zero points that are
fractional, on a .5 tie or outside [qmin, qmax], and scales that are negative, zero, NaN
or outside the fast division's [2^-63, 2^63].

The comparison (check): y and grad_x bit for bit (NaN positions equal); a scale or
zero-point gradient of the same class as the expected one -- NaN, +inf, -inf or finite --
and, where finite, within a relative bound plus an absolute floor.
"""
import math
from collections import namedtuple

import numpy as np

from oracle import fakequant_np as O
from tests import goldens as G

F32 = np.float32
NAN, INF = float("nan"), float("inf")

# sym / bits: the quantizer; learn_zp 0: zero point 0 (symmetric), 1: a learned zero
# point that zero_point_rounding rounds and clamps (asymmetric), 2: a symmetric quantizer
# given a gradient-requiring tensor zero point, used as it is
QCase = namedtuple("QCase", "name sym bits learn_zp scale zp")


def _q(sym, bits, learn_zp, scale, zp):
    return QCase(f"{'s' if sym else 'a'}{bits}_z{learn_zp}_s{scale!r}_zp{zp!r}", sym, bits, learn_zp, scale, zp)


TINY_S, HUGE_S = 1e-30, 1e30        # below 2^-63 and above 2^63: every division is IEEE
QCASES = (
    # ordinary scales at 2 / 4 / 8 bits in the three zero-point modes; 0.25 makes the
    # planted ties exact in fp32, 4.0 lets a finite gradient overflow g * s
    [_q(True, 2, 0, 0.3, 0), _q(True, 4, 0, 0.25, 0), _q(True, 8, 0, 0.03, 0), _q(True, 4, 0, 4.0, 0),
     _q(True, 2, 2, 0.3, 1.0), _q(True, 4, 2, 0.25, 0.75), _q(True, 8, 2, 0.03, 2.5), _q(True, 4, 2, 0.3, 9.0),
     _q(False, 2, 1, 0.3, 1.3), _q(False, 4, 1, 0.25, 3.0), _q(False, 8, 1, 0.03, 2.5), _q(False, 4, 1, 4.0, 3.0),
     # learned zero points: fractional, .5 ties (rint to even: 2 and 4), outside the range
     _q(False, 4, 1, 0.3, 6.7), _q(False, 4, 1, 0.3, 3.5), _q(False, 4, 1, 0.3, 20.0), _q(False, 4, 1, 0.3, -1.7),
     _q(False, 8, 1, 0.03, 300.0)]
    # scales that training has driven negative, to zero or to NaN, or out of the fast range
    + [_q(sym, 4, lz, s, zp) for s in (-0.3, TINY_S, HUGE_S, 0.0, NAN)
       for sym, lz, zp in ((True, 0, 0), (False, 1, 3.0))]
    + [_q(True, 4, 2, -0.3, 0.75), _q(True, 4, 2, NAN, 0.75), _q(False, 4, 1, -0.3, 20.0)])

# what is planted besides the finite edge values (see special_block)
VARIANTS = ("finite", "x_nonfinite", "g_inf_clamped", "g_nan_in_range", "g_inf_in_range", "g_overflow", "all")


def qrange(qc):
    return O.qrange(qc.bits, qc.sym)


def zp_used(qc):
    """The zero point the element arithmetic sees (uniform.py:98-102 for a learned one)."""
    qmin, qmax = qrange(qc)
    if qc.learn_zp == 1:
        return float(min(max(np.rint(np.float64(qc.zp)), qmin), qmax))
    return float(qc.zp)


def _nominal_scale(qc):
    """The scale the planted x values are placed with: the case's own, or 0.3 where that
    places nothing (zero, NaN)."""
    s = float(F32(qc.scale))
    return s if math.isfinite(s) and s != 0.0 else 0.3


def special_block(qc, variant):
    """(x, g, k) fp32: the variant's own k pairs first, then the finite edge values.
    x_in / x_cl below are an in-range and a clamped element (for the case's own scale)."""
    assert variant in VARIANTS
    qmin, qmax = qrange(qc)
    s, z = _nominal_scale(qc), zp_used(qc)
    mid = (qmin + qmax) // 2
    at = lambda k: F32((k - z) * s)    # noqa: E731  x whose x / s + z is k (up to fp32 rounding)
    x_in, x_cl = at(mid + 0.25), at(qmax + 5)
    ordinary = (0.7, -1.3, 2.0, -0.5)
    xs, gs = [], []
    # finite x edges, each under an ordinary gradient
    fx = [0.0, -0.0, 1e-40, -1e-40]
    fx += [at(k + 0.5) for k in (qmin - 1, qmin, mid - 1, mid, qmax - 1, qmax)]       # ties
    for b in (qmin, qmax):                                                           # clamp bounds
        e = at(b)
        fx += [e, np.nextafter(e, F32(-INF)), np.nextafter(e, F32(INF))]
    for i, v in enumerate(fx):
        xs.append(v)
        gs.append(ordinary[i % 4])
    # finite g edges, each once in range and once clamped
    for gv in (0.0, -0.0, 1e-40, -1e-40):
        xs += [x_in, x_cl]
        gs += [gv, gv]
    key_x, key_g = [], []
    if variant in ("x_nonfinite", "all"):
        key_x += [INF, -INF, NAN]
        key_g += [0.7, -1.3, 2.0]
    plant = {"g_inf_clamped": [(x_cl, INF)], "g_nan_in_range": [(x_in, NAN)], "g_inf_in_range": [(x_in, INF)],
             # g * s overflows where |s| >= 4; 1e38 and not more, so that below that the
             # reference's fp32 sum of the planted -(g * s) stays finite like the f64 one
             "g_overflow": [(x_in, 1e38), (x_cl, 1e38)],
             "all": [(xv, gv) for gv in (NAN, INF, -INF, 1e38) for xv in (x_in, x_cl)]}.get(variant, [])
    for xv, gv in plant:
        key_x.append(xv)
        key_g.append(gv)
    return np.array(key_x + xs, dtype=F32), np.array(key_g + gs, dtype=F32), len(key_x)


def build_inputs(qc, variant, n, seed=0):
    """fp32 x and g of n elements: randn around the quantizer's range with special_block
    planted in the first group of four (from element 0, the variant's own pairs first), up
    to the end of the last whole group (rotated, so those pairs end it) and in the scalar
    tail n % 4 (those pairs again)."""
    rng = np.random.default_rng(seed)
    qmin, qmax = qrange(qc)
    s, z = _nominal_scale(qc), zp_used(qc)
    u = rng.standard_normal(n) * (qmax - qmin + 1) / 3.0 + (qmin + qmax) / 2.0
    x = ((u - z) * s).astype(F32)
    g = rng.standard_normal(n).astype(F32)
    bx, bg, nkey = special_block(qc, variant)
    nkey = nkey or 4                   # a "finite" block: its first four values stand in
    L = min(len(bx), n)
    x[:L], g[:L] = bx[:L], bg[:L]
    whole = 4 * (n // 4)
    rx, rg = np.roll(bx, -nkey), np.roll(bg, -nkey)       # the variant's pairs last
    k = min(len(rx), whole - 4)
    if k > 0:
        x[whole - k:whole], g[whole - k:whole] = rx[len(rx) - k:], rg[len(rg) - k:]
    for i in range(whole, n):
        x[i], g[i] = bx[(i - whole) % nkey], bg[(i - whole) % nkey]
    return x, g


# --------------------------------------------------------------------------- oracle
Expect = namedtuple("Expect", "y gx gs gz mag_s mag_z")


def _magnitudes(a, g, scale, zp_eff, qmin, qmax, learn_zp):
    """Sums of the finite terms' magnitudes of the two gradient sums (before gscale): what
    a different summation order can move, per unit of relative rounding."""
    s, z = F32(scale), F32(zp_eff)
    _, q, mask = O.fq_forward(a, scale, zp_eff, qmin, qmax)
    with np.errstate(all="ignore"):
        gq = (g * s).astype(F32)
        gm = np.where(mask, gq, F32(0.0)).astype(F32)
        t1 = (g * (q - z).astype(F32)).astype(F32)
        t2 = ((-gm).astype(F32) * ((a / s).astype(F32) / s).astype(F32)).astype(F32)

        def mag(*ts):
            return float(sum(np.abs(t.astype(np.float64))[np.isfinite(t)].sum() for t in ts))

        return mag(t1, t2), (mag(gm, gq) if learn_zp else 0.0)


def oracle(x, g, qc, gscale, act=None, silu_ref=O.SILU_REF_DEFAULT):
    """The oracle's forward + backward of one case on the pre-activation x (act None:
    the quantizer's input itself)."""
    x, g = np.asarray(x, dtype=F32), np.asarray(g, dtype=F32)
    qmin, qmax = qrange(qc)
    a = O.act_forward(x, act, silu_ref)
    with np.errstate(all="ignore"):
        y, gx, gs, gz = O.lsq_forward_backward(a, g, qc.scale, qc.zp, qmin, qmax, gscale, learn_zp=qc.learn_zp)
    gx = O.act_backward(gx, x, act, silu_ref)
    ms, mz = _magnitudes(a, g, qc.scale, zp_used(qc), qmin, qmax, qc.learn_zp)
    return Expect(y, gx, gs, 0.0 if gz is None else gz, ms * abs(gscale), mz * (1.0 if qc.learn_zp == 2 else abs(gscale)))


def pc_oracle(x, g, scales, zps, qmin, qmax, gscale, axis, learn_zp):
    """Per-channel: every channel slice the per-tensor oracle with its own qparams."""
    with np.errstate(all="ignore"):
        y, gx, gs, gz = O.pc_lsq_forward_backward(x, g, scales, zps, qmin, qmax, gscale, axis=axis,
                                                  learn_zp=learn_zp)
    C = x.shape[axis]
    ms, mz = np.zeros(C), np.zeros(C)
    for c in range(C):
        idx = tuple([slice(None)] * axis + [c])
        zr = float(min(max(np.rint(np.float64(zps[c])), qmin), qmax)) if learn_zp else float(zps[c])
        ms[c], mz[c] = _magnitudes(x[idx], g[idx], float(scales[c]), zr, qmin, qmax, learn_zp)
    return Expect(y, gx, gs, gz, ms * abs(gscale), mz * abs(gscale))


# --------------------------------------------------------------------------- the comparison
def grad_class(v):
    v = float(v)
    if math.isnan(v):
        return "nan"
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return "finite"


def assert_grad(got, want, what, rel, floor):
    """Same class as the expected gradient (NaN, +inf, -inf, finite); a finite one within
    rel * |want| + floor."""
    cg, cw = grad_class(got), grad_class(want)
    assert cg == cw, f"{what}: got {float(got)!r} ({cg}), expected {float(want)!r} ({cw})"
    if cw == "finite":
        assert abs(float(got) - float(want)) <= rel * abs(float(want)) + floor, \
            f"{what}: got {float(got)!r}, expected {float(want)!r} (rel {rel}, floor {floor})"


# against the oracle's f64 closed form: 1e-9 relative plus 1e-13 of the sum of the terms'
# magnitudes (f64 summation order; tests/test_gpu_deferred_grads.py test_fast_path_bounds_k4_k4d)
ORACLE_REL, ORACLE_CANCEL = 1e-9, 1e-13
# against the reference's own fp32 autograd sums (the goldens): 1e-4 relative, or 3e-6
# absolute where the sums cancel (tests/test_oracle_golden.py test_learnable_sym_tensor_zp)
GOLDEN_REL, GOLDEN_FLOOR = 1e-4, 3e-6


def check(got_y, got_gx, got_gs, got_gz, exp, what, zp_grad=True):
    """One result against the oracle: y (None: not produced by this form) and grad_x bit
    for bit, the gradients by class and, finite, to f64 summation order.  got_gs / got_gz /
    exp.gs / exp.gz: numbers, or [C] arrays per channel."""
    if got_y is not None:
        G.assert_bitwise_f32(got_y, exp.y, f"{what}: y")
    G.assert_bitwise_f32(got_gx, exp.gx, f"{what}: grad_x")
    pairs = [("grad_scale", got_gs, exp.gs, exp.mag_s)]
    if zp_grad:
        pairs.append(("grad_zp", got_gz, exp.gz, exp.mag_z))
    for name, got, want, mag in pairs:
        got, want, mag = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(mag)
        assert got.shape == want.shape, f"{what}: {name} shape {got.shape} vs {want.shape}"
        for c in range(got.size):
            assert_grad(got[c], want[c], f"{what}: {name}[{c}]", ORACLE_REL, ORACLE_CANCEL * mag[c])


def check_golden(y, gx, gs, gz, case, what):
    """One result against a reference fixture (the reference's fp32 sums: the looser bars).
    The fixture's gradients are numbers, their repr (JSON has no NaN / inf) or the key of a
    [C] array; gs / gz None: not compared."""
    G.assert_bitwise_f32(y, G.arr(case["y"]), f"{what}: y")
    G.assert_bitwise_f32(gx, G.arr(case["grad_x"]), f"{what}: grad_x")
    for name, got, key in (("grad_scale", gs, "scale_grad"), ("grad_zp", gz, "zp_grad")):
        if got is None:
            continue
        want = golden_grad(case, key)
        got = np.atleast_1d(got).reshape(-1)
        assert got.shape == want.shape, f"{what}: {name} shape {got.shape} vs {want.shape}"
        for c in range(got.size):
            assert_grad(got[c], want[c], f"{what}: {name}[{c}]", GOLDEN_REL, GOLDEN_FLOOR)


def golden_grad(case, key):
    """A fixture's gradient as a flat f64 array."""
    v = case[key]
    try:
        return np.atleast_1d(np.float64(float(v)))
    except ValueError:
        return np.asarray(G.arr(v), dtype=np.float64).reshape(-1)


# --------------------------------------------------------------------------- per-channel
def pc_build(shape, axis, sym, bits, seed, learn_zp):
    """A learnable per-channel case: ordinary channels and three special ones -- channel 1
    holds a NaN gradient on an in-range element, channel 2 has a negative scale, channel 3
    is clamped everywhere.  Returns x, g, scales f64[C], zps f64[C]."""
    rng = np.random.default_rng(seed)
    C = shape[axis]
    assert C >= 4
    qmin, qmax = O.qrange(bits, sym)
    s = rng.uniform(0.02, 0.06, C) * (1.0 if bits == 8 else 8.0)
    s[2] = -s[2]
    z = np.rint(rng.uniform(qmin + 1, qmax - 1, C)) + 0.2 if learn_zp else np.zeros(C)
    zr = np.rint(z)
    x = np.empty(shape, dtype=F32)
    g = rng.standard_normal(shape).astype(F32)
    for c in range(C):
        idx = tuple([slice(None)] * axis + [c])
        u = rng.standard_normal(x[idx].shape) * (qmax - qmin + 1) / 3.0 + (qmin + qmax) / 2.0
        if c == 3:
            u = np.abs(u) + qmax + 4                      # every element above qmax
        x[idx] = ((u - zr[c]) * s[c]).astype(F32)
    first = tuple([0] * axis + [1] + [0] * (len(shape) - axis - 1))   # channel 1's first element: in range
    x[first] = F32(((qmin + qmax) // 2 + 0.25 - zr[1]) * s[1])
    g[first] = NAN
    return x, g, s, z
