"""Every device form of the learnable (LSQ) backward -- they share one element function,
lsq_elem in csrc/k_body.cuh -- against the oracle at non-finite, tie and clamp-edge inputs:
K4 (FQ.lsq_backward) at 2 / 4 / 8 / 16 groups per lane, K4d (records-only + fold), K7
(multi-tensor), K6 (per-channel, axis 0 and 1, every launch form) and the typed K4 / K4d.

tests/lsq_edges_common.py builds the inputs (the special values stand in the first group
of four, in the last whole group and in the scalar tail) and states the comparison: y and
grad_x bit for bit with NaN positions equal; a scale / zero-point gradient of the oracle's
class (NaN, +inf, -inf, finite) and, finite, within 1e-9 relative plus 1e-13 of the sum of
the terms' magnitudes.  The oracle itself is pinned to the reference on these inputs by
tests/test_lsq_edges_cpu.py.  Nothing is filtered: a form that cannot take an input
raises, and the raise is asserted.
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from vsiquantization_amd import _hip as H
from vsiquantization_amd import fakequant as FQ
from vsiquantization_amd.quantizers import deferred as D
from oracle import fakequant_np as O
from tests import goldens as G
from tests import lsq_edges_common as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vsiquantization_amd", "csrc")
with open(os.path.join(CSRC, "vsiq_common.cuh")) as _f:
    KBLOCK = int(re.search(r"constexpr int kBlock = (\d+);", _f.read()).group(1))
GROUPS = (2, 4, 8, 16)
SILU = H.SiluAct(*O.SILU_REF_DEFAULT)      # the host layout the oracle's SiLU names
ACTS = {"none": None, "relu": "relu", "silu": SILU}
GSCALE = 0.37


def sizes(groups):
    """The smallest n at which each launch form differs: one partial workgroup (scalar
    tail), one full workgroup plus a tail, several workgroups (a real fold)."""
    span = 4 * KBLOCK * groups
    return (37, span + 3, 3 * span + 5)


def cu(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(grad) if grad else t


def npy(t):
    return t.detach().cpu().numpy()


def offset_view(x):
    """x's values one element into a buffer: off 16-byte alignment, the scalar path"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:].copy_(x)
    v = buf[1:]
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def qparams(qc, on_device):
    """(scale, zero point) of a case as host numbers or as device f64 tensors (load_qp<true>)"""
    s, z = float(qc.scale), float(qc.zp)
    if on_device:
        return (torch.tensor(s, dtype=torch.float64, device=DEV), torch.tensor(z, dtype=torch.float64, device=DEV))
    return s, z


def run_k4d(gd, xd, s, z, qc, act):
    """D.lsq_backward_part + D.fold: (grad_x, f64[2])"""
    qmin, qmax = EC.qrange(qc)
    e = D._Fold()
    e.nrec = int(H.lib().vsiq_lsq_part_records(H.c_i64(xd.numel())))
    e.records = torch.full((2 * e.nrec,), float("nan"), dtype=torch.float64, device=DEV)
    gx, e.zd, e.zh = D.lsq_backward_part(gd, xd, s, z, qmin, qmax, qc.learn_zp, act, e.records)
    e.gscale, e.qmin, e.qmax, e.learn_zp = GSCALE, qmin, qmax, bool(qc.learn_zp)
    e.out = torch.empty(2, dtype=torch.float64, device=DEV)
    e.keep = (s, z)
    D.fold([e])
    return gx, e.out


def same_class(a, b, what):
    assert EC.grad_class(a) == EC.grad_class(b), f"{what}: {float(a)!r} vs {float(b)!r}"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    H.lib()   # raises if the HIP library is missing: no silent fallback


# --------------------------------------------------------------------------- K4 and K4d
@pytest.mark.parametrize("learn_zp", [0, 1, 2])
@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("groups", GROUPS)
def test_k4_k4d_vs_oracle(groups, act, learn_zp):
    """K1 / K5 forward and K4 backward of every case and variant, aligned and one element
    off, qparams from the host and from the device; K4d on the same inputs (grad_x bit
    equal to K4's, the folded gradients of K4's and the oracle's class) -- or, learn_zp 2,
    its raise."""
    act = ACTS[act]
    H.set_tuning(H.TUNE_LSQ_GROUPS, groups)
    try:
        for qc in (q for q in EC.QCASES if q.learn_zp == learn_zp):
            qmin, qmax = EC.qrange(qc)
            for vi, variant in enumerate(EC.VARIANTS):
                for n in sizes(groups):
                    x, g = EC.build_inputs(qc, variant, n, seed=vi + n)
                    exp = EC.oracle(x, g, qc, GSCALE, act)
                    xd0, gd0 = cu(x), cu(g)
                    for off in (False, True):
                        xd, gd = (offset_view(xd0), offset_view(gd0)) if off else (xd0, gd0)
                        for on_device in (False, True):
                            what = f"{qc.name} {variant} n={n} off={off} device-qp={on_device}"
                            s, z = qparams(qc, on_device)
                            y = FQ.fake_quant(xd, s, z, qmin, qmax, zp_round=learn_zp == 1, act=act)[0]
                            gx, grads = FQ.lsq_backward(gd, xd, s, z, qmin, qmax, GSCALE, learn_zp, act=act)
                            grads = npy(grads)
                            EC.check(npy(y), npy(gx), grads[0], grads[1], exp, "K4 " + what, zp_grad=bool(learn_zp))
                            if learn_zp == 2:
                                with pytest.raises(ValueError, match="learn_zp"):
                                    run_k4d(gd, xd, s, z, qc, act)
                                continue
                            gxd, out = run_k4d(gd, xd, s, z, qc, act)
                            out = npy(out)
                            assert torch.equal(gxd.view(torch.int32), gx.view(torch.int32)), "K4d grad_x " + what
                            same_class(out[0], grads[0], "K4d / K4 grad_scale " + what)
                            same_class(out[1], grads[1], "K4d / K4 grad_zp " + what)
                            EC.check(None, npy(gxd), out[0], out[1], exp, "K4d " + what, zp_grad=bool(learn_zp))
    finally:
        H.set_tuning(H.TUNE_LSQ_GROUPS, 0)


def test_in_range_nonfinite_gradient_makes_zero_point_gradient_nan():
    """The reference's zero-point gradient is sum(gm) + sum(-gq): one in-range element
    whose g * s is NaN or +-inf makes it NaN (NaN, or inf + -inf) -- on the device too, in
    every place of a launch (first group, last whole group, scalar tail)."""
    qc = next(q for q in EC.QCASES if q.learn_zp == 1 and q.scale == 0.25 and q.zp == 3.0)
    qmin, qmax = EC.qrange(qc)
    n = 4 * KBLOCK * 4 + 3
    x, g = EC.build_inputs(qc, "finite", n, seed=5)
    x_in = np.float32((7 + 0.25 - 3.0) * 0.25)
    for bad in (np.nan, np.inf, -np.inf):
        for pos in (1, n - 5, n - 1):
            xs, gs = x.copy(), g.copy()
            xs[pos], gs[pos] = x_in, bad
            exp = EC.oracle(xs, gs, qc, GSCALE)
            assert np.isnan(exp.gz)
            gx, grads = FQ.lsq_backward(cu(gs), cu(xs), 0.25, 3.0, qmin, qmax, GSCALE, 1)
            grads = npy(grads)
            EC.check(None, npy(gx), grads[0], grads[1], exp, f"g={bad} at {pos}")


# --------------------------------------------------------------------------- K7
@pytest.mark.parametrize("learn_zp", [0, 1])
def test_k7_middle_tensor_vs_oracle_neighbours_untouched(learn_zp):
    """Three tensors in one launch each way, the middle one carrying the special values:
    it equals the oracle, and its neighbours' outputs are their single-tensor results bit
    for bit -- a NaN does not leak across descriptors."""
    n_side = (4 * KBLOCK * 4 + 3, 1023)
    for qc in (q for q in EC.QCASES if q.learn_zp == learn_zp):
        qmin, qmax = EC.qrange(qc)
        for vi, variant in enumerate(EC.VARIANTS):
            n = sizes(4)[vi % 3]
            x, g = EC.build_inputs(qc, variant, n, seed=31 + vi)
            exp = EC.oracle(x, g, qc, GSCALE)
            gen = torch.Generator(device=DEV).manual_seed(vi)
            sides = [(torch.randn(m, device=DEV, generator=gen) * 0.5, torch.randn(m, device=DEV, generator=gen))
                     for m in n_side]
            data = [sides[0], (cu(x), cu(g)), sides[1]]

            def params():
                ps = []
                for i in range(3):
                    s = float(qc.scale) if i == 1 else 0.05 + 0.01 * i
                    z = float(qc.zp) if i == 1 else 3.0
                    ps.append((nn.Parameter(torch.tensor(s, dtype=torch.float64, device=DEV)),
                               nn.Parameter(torch.tensor(z, dtype=torch.float64, device=DEV)) if learn_zp else 0))
                return ps

            pm = params()
            xs = [d[0].clone().requires_grad_(True) for d in data]
            specs = [FQ.LsqSpec(s, z, qmin, qmax, GSCALE, learn_zp) for s, z in pm]
            ys = FQ.lsq_fake_quant_multi(xs, specs)
            torch.autograd.backward(ys, [d[1] for d in data])
            what = f"K7 {qc.name} {variant} n={n}"
            EC.check(npy(ys[1]), npy(xs[1].grad), float(pm[1][0].grad), float(pm[1][1].grad) if learn_zp else 0.0,
                     exp, what, zp_grad=bool(learn_zp))
            ps = params()
            for i in (0, 2):
                xr = data[i][0].clone().requires_grad_(True)
                yr = FQ.FakeQuantLearnFn.apply(xr, ps[i][0], ps[i][1], qmin, qmax, GSCALE, learn_zp, None)
                yr.backward(data[i][1])
                assert torch.equal(ys[i].detach().view(torch.int32), yr.detach().view(torch.int32)), what
                assert torch.equal(xs[i].grad.view(torch.int32), xr.grad.view(torch.int32)), what
                assert torch.equal(pm[i][0].grad, ps[i][0].grad) and torch.isfinite(pm[i][0].grad), what
                if learn_zp:
                    assert torch.equal(pm[i][1].grad, ps[i][1].grad) and torch.isfinite(pm[i][1].grad), what


def test_k7_and_k4d_refuse_a_zero_point_used_as_given():
    """learn_zp 2 is the per-tensor K4's alone: the multi-tensor spec and the records-only
    backward raise instead of running it as a rounded, clamped zero point."""
    with pytest.raises(ValueError, match="learn_zp"):
        FQ.LsqSpec(0.3, 0.75, -8, 7, GSCALE, 2)
    x = torch.randn(64, device=DEV)
    rec = torch.empty(2 * int(H.lib().vsiq_lsq_part_records(H.c_i64(64))), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="learn_zp"):
        D.lsq_backward_part(x, x, 0.3, 0.75, -8, 7, 2, None, rec)


# --------------------------------------------------------------------------- K6
@pytest.mark.parametrize("learn_zp", [False, True])
@pytest.mark.parametrize("form,shape,axis,packed", [
    ("axis 0 row-resident", (6, 5, 3, 3), 0, 1), ("axis 0 row-resident", (5, 1030), 0, 1),
    ("axis 0 two-stage", (6, 5, 3, 3), 0, 0), ("axis 0 two-stage", (5, 1030), 0, 0),
    ("axis 1 packed short rows", (3, 7, 4), 1, 1), ("axis 1 channel columns", (100, 8, 10, 10), 1, 1)])
def test_k6_vs_oracle(form, shape, axis, packed, learn_zp):
    """Per-channel forward and K6 backward with three special channels (an in-range NaN
    gradient, a negative scale, clamped everywhere) among ordinary ones; the channel
    counters are left at zero."""
    for bits in (4, 8):
        sym = not learn_zp
        qmin, qmax = O.qrange(bits, sym)
        x, g, s, z = EC.pc_build(shape, axis, sym, bits, seed=sum(shape) + bits, learn_zp=learn_zp)
        C = shape[axis]
        gscale = (qmax * x.size / C) ** -0.5
        exp = EC.pc_oracle(x, g, s, z, qmin, qmax, gscale, axis, learn_zp)
        assert np.isnan(exp.gs[1]) and np.isfinite(np.delete(exp.gs, 1)).all()
        sd, zd = cu(s), cu(z)
        H.set_tuning(H.TUNE_PC_PACKED, packed)
        try:
            y = FQ.per_channel_fake_quant(cu(x), sd, zd, qmin, qmax, zp_round=learn_zp, axis=axis)[0]
            gx, gs, gz = FQ.pc_lsq_backward(cu(g), cu(x), sd, zd, qmin, qmax, gscale, learn_zp, axis)
        finally:
            H.set_tuning(H.TUNE_PC_PACKED, 1)
        EC.check(npy(y), npy(gx), npy(gs), npy(gz), exp, f"K6 {form} {shape} {bits} bits", zp_grad=learn_zp)
        assert int(H.workspace(torch.device(DEV)).channel_counters(C).abs().sum()) == 0


# --------------------------------------------------------------------------- the fixtures on the device
@pytest.mark.parametrize("case", G.cases("learnable_fq_edges"), ids=lambda c: f"{c['key']}-{c['qcase']}-{c['variant']}")
def test_golden_learnable_edges(case):
    x, g = G.arr(case["x"]), G.arr(case["g"])
    lz = case["learn_zp"]
    qmin, qmax = O.qrange(case["bits"], case["sym"])
    scale = nn.Parameter(torch.tensor(float(case["scale"]), dtype=torch.float64, device=DEV))
    zp = nn.Parameter(torch.tensor(float(case["zp"]), dtype=torch.float64, device=DEV)) if lz else 0
    xg = cu(x, grad=True)
    y = FQ.FakeQuantLearnFn.apply(xg, scale, zp, qmin, qmax, O.grad_scale(qmax, x.size), lz, None)
    y.backward(cu(g))
    EC.check_golden(npy(y), npy(xg.grad), float(scale.grad), float(zp.grad) if lz else None, case, case["key"])


@pytest.mark.parametrize("case", G.cases("per_channel_learnable_edges"), ids=lambda c: c["key"])
def test_golden_per_channel_learnable_edges(case):
    w, g = G.arr(case["x"]), G.arr(case["g"])
    sym = case["sym"]
    q = V.PerChannelUniformQuantizer(case["bits"], sym)
    scale = nn.Parameter(cu(G.arr(case["scale"]).copy()))
    zp = 0 if sym else nn.Parameter(cu(G.arr(case["zp"]).copy()))
    xg = cu(w, grad=True)
    y = q.quantize(xg, scale, zp, True)
    y.backward(cu(g))
    EC.check_golden(npy(y), npy(xg.grad), npy(scale.grad), None if sym else npy(zp.grad), case, case["key"])


def test_golden_lsq_fake_quantize_edges():
    (case,) = [c for c in G.cases("lsq_fake_quantize") if c.get("edges")]
    x, g = G.arr(case["x"]), G.arr(case["g"])
    sp, zp = nn.Parameter(cu(G.arr(case["scale"]).copy())), nn.Parameter(cu(G.arr(case["zp"]).copy()))
    gsc = O.lsq_module_grad_scale(x.shape, case["qmax"], True, case["config_act"])
    xg = cu(x, grad=True)
    y = FQ.PerChannelLearnFn.apply(xg, sp, zp, case["qmin"], case["qmax"], gsc, True, 1)
    y.backward(cu(g))
    EC.check_golden(npy(y), npy(xg.grad), npy(sp.grad), npy(zp.grad), case, case["key"])


# --------------------------------------------------------------------------- typed K4 / K4d
def _all_patterns(dtype):
    return torch.arange(-32768, 32768, dtype=torch.int32, device=DEV).to(torch.int16).view(dtype)


def _assert_bits_t(got, exp32, what):
    """got (T) is the fp32 expectation rounded once to T, as raw 16-bit patterns"""
    exp = torch.from_numpy(exp32).to(DEV).to(got.dtype)
    nan = torch.isnan(exp)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    a, b = got.view(torch.int16)[~nan], exp.view(torch.int16)[~nan]
    bad = (a != b).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {a.numel()} differ, first at {int(bad[0])}"


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_typed_k4_k4d_all_gradient_patterns_vs_oracle(dtype, act):
    """All 65,536 gradient patterns over a permuted x (tests/test_gpu_half.py
    test_lsq_backward's input) against the oracle on the widened arrays: grad_x the
    oracle's rounded once to T, the gradients by class -- and a finite-gradient half of
    the same input to f64 order."""
    act = ACTS[act]
    qc = EC.QCase("typed", False, 8, 1, 0.05, 37.0)
    qmin, qmax = EC.qrange(qc)
    g = _all_patterns(dtype)
    perm = torch.randperm(g.numel(), generator=torch.Generator(device="cpu").manual_seed(5)).to(DEV)
    x = g[perm].contiguous()
    finite = (g.float().abs() < 1e30) & (x.float().abs() < 1e30)   # NaN compares false
    for gd, xd in ((g, x), (g[finite].contiguous(), x[finite].contiguous())):
        exp = EC.oracle(npy(xd.float()), npy(gd.float()), qc, GSCALE, act)
        gx, grads = FQ.lsq_backward(gd, xd, 0.05, 37.0, qmin, qmax, GSCALE, 1, act=act)
        gxd, out = run_k4d(gd, xd, 0.05, 37.0, qc, act)
        assert gx.dtype == dtype and gxd.dtype == dtype
        what = f"{dtype} n={gd.numel()}"
        _assert_bits_t(gx, exp.gx, "K4 " + what)
        assert torch.equal(gx.view(torch.int16), gxd.view(torch.int16)), "K4d " + what
        for name, got in (("K4", npy(grads)), ("K4d", npy(out))):
            EC.assert_grad(got[0], exp.gs, f"{name} grad_scale {what}", EC.ORACLE_REL, EC.ORACLE_CANCEL * exp.mag_s)
            EC.assert_grad(got[1], exp.gz, f"{name} grad_zp {what}", EC.ORACLE_REL, EC.ORACLE_CANCEL * exp.mag_z)
