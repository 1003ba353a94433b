"""bf16 / fp16 activations through the typed kernels (ABI 12: vsiq_act_fq_fwd_t,
vsiq_act_ste_bwd_t, vsiq_act_lsq_bwd_t, vsiq_act_observe_t).

The rule under test: a typed call is its fp32 counterpart applied to the exactly widened
inputs, with every tensor output of element type T rounded once to T (nearest even);
codes, the 1-bit mask, qparams, running state, stats record and the f64 gradients are the
fp32 call's, bit for bit (the grids and fold orders depend on n only).  So the oracle
everywhere is this library's own fp32 entry point on ``x.float()`` followed by torch's
``.to(T)``; tensor outputs are compared as raw 16-bit patterns.
"""
import os
import re

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from vsiquantization_amd import _hip as H                      # noqa: E402
from vsiquantization_amd import fakequant as FQ                # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
ACTS = [None, "relu", "silu"]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vsiquantization_amd", "csrc")
# (qmin, qmax, scale, zero point): sym int8, asym uint8, 4-bit
CONFIGS = [(-128, 127, 0.05, 0), (0, 255, 0.02, 37), (-8, 7, 0.3, 0)]

# Workgroup spans (elements) of the launchers, 4 * kBlock * U: the forward and the STE
# backward pick U = kFlatU (2) or 9, K4 picks 4 or 8 groups per lane by size
# (test_spans_match_the_source reads them from the source).
KBLOCK, FLAT_U, GATED_U, LSQ_G = 256, 2, 9, (4, 8)
SPANS = sorted({4 * KBLOCK * u for u in (FLAT_U, GATED_U) + LSQ_G})
EDGE_N = sorted({1, 3, 4, 5, 255, 256, 257, 1023, 1025} | {k * s + d for s in SPANS for k in (1, 2) for d in (-1, 1)}
                | {s + 4 for s in SPANS})   # + vector-path sizes of more than one workgroup


def all_patterns(dtype):
    """Every one of the 65,536 bit patterns of a 16-bit type: +-0, denormals, +-inf, every NaN."""
    return torch.arange(-32768, 32768, dtype=torch.int32, device=DEV).to(torch.int16).view(dtype)


def permuted(x, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return x[torch.randperm(x.numel(), generator=g).to(x.device)].contiguous()


def assert_bits(got, exp32, what=""):
    """got (T) == RNE_T(exp32) as raw 16-bit patterns; NaN positions agree (payload free)."""
    assert got.dtype in DTYPES and exp32.dtype == torch.float32 and got.shape == exp32.shape, what
    exp = exp32.to(got.dtype)
    nan = torch.isnan(exp)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    g, e = got.view(torch.int16)[~nan], exp.view(torch.int16)[~nan]
    bad = (g != e).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {g.numel()} differ, first at {int(bad[0])}"


def same_bits(a, b):
    """two tensors of one dtype, bit for bit (NaNs included)"""
    v = {8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.int8}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def offset_view(x):
    """x's values at an address one element past an aligned one: the scalar path"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:].copy_(x)
    v = buf[1:]
    assert v.is_contiguous() and v.data_ptr() % 8 != 0
    return v


def test_spans_match_the_source():
    """The U / G values EDGE_N is built from are the launchers' (read from the source)."""
    common = open(os.path.join(CSRC, "vsiq_common.cuh")).read()
    assert int(re.search(r"constexpr int kBlock = (\d+);", common).group(1)) == KBLOCK
    assert int(re.search(r"constexpr int kFlatU = (\d+);", common).group(1)) == FLAT_U
    m = re.search(r"return groups >= \(int64_t\)5 << 20 \? (\d+) : (\d+);", common)
    assert (int(m.group(2)), int(m.group(1))) == LSQ_G
    for f, kern in (("k_fq.cuh", "fq_fwd_kernel"), ("k_ste.cuh", "ste_bwd_kernel")):
        src = open(os.path.join(CSRC, f)).read()
        us = set(re.findall(rf"{kern}<T, [A-Z, ]+, (\w+)>\(\)", src))
        assert us == {str(GATED_U), "kFlatU"}, (f, us)


# --------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_every_input_value(dtype, act):
    x = all_patterns(dtype)
    xf = x.float()
    for qmin, qmax, s, zp in CONFIGS:
        y, m, c = FQ.fake_quant(x, s, zp, qmin, qmax, want_mask=True, want_codes=True, act=act)
        yo, mo, co = FQ.fake_quant(xf, s, zp, qmin, qmax, want_mask=True, want_codes=True, act=act)
        assert y.dtype == dtype and y.shape == x.shape
        assert_bits(y, yo, f"y {qmin}..{qmax}")
        assert c.dtype == co.dtype and torch.equal(c, co)
        assert torch.equal(m, mo)


# --------------------------------------------------------------------------- 2. narrowing
@pytest.mark.parametrize("discrete", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_narrowing_ties(dtype, discrete):
    """(q - zp) * s with s = 1 + half an ulp of 1 in T: every odd q lands exactly on a tie."""
    s = 1.0 + (2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11)
    for qmin, qmax, zp in ((-128, 127, 0), (0, 255, 37)):
        x = (torch.arange(qmin - 2, qmax + 3, device=DEV, dtype=torch.float32) - zp).to(dtype)
        assert torch.equal(x.float(), torch.arange(qmin - 2, qmax + 3, device=DEV, dtype=torch.float32) - zp)
        y, _, c = FQ.fake_quant(x, s, zp, qmin, qmax, want_codes=True, discrete=discrete)
        yo, _, co = FQ.fake_quant(x.float(), s, zp, qmin, qmax, want_codes=True, discrete=discrete)
        assert_bits(y, yo, "ties")
        assert torch.equal(c, co)
        assert torch.equal(co.to(torch.int32).unique(), torch.arange(qmin, qmax + 1, device=DEV, dtype=torch.int32))
        if not discrete:   # the case is what it claims: fp32 results half way between two T values
            inexact = yo != yo.to(dtype).float()
            assert int(inexact.sum()) >= (qmax - qmin) // 2


def test_fp16_overflow_gives_inf():
    inf = float("inf")
    x = torch.tensor([inf, -inf, 65504.0, -65504.0, 60000.0, -60000.0, 1000.0, 0.0], device=DEV).half()
    y, _, c = FQ.fake_quant(x, 1000.0, 0, -128, 127, want_codes=True)
    yo, _, co = FQ.fake_quant(x.float(), 1000.0, 0, -128, 127, want_codes=True)
    assert yo[:2].tolist() == [127000.0, -128000.0]
    assert y[:2].tolist() == [inf, -inf]
    assert_bits(y, yo, "overflow")
    assert torch.equal(c, co)
    d, _, _ = FQ.fake_quant(x, 1000.0, 0, -128, 127, discrete=True)
    assert d[:2].tolist() == [127.0, -128.0]


# --------------------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_of_the_grid_and_the_vector_path(dtype, aligned):
    """n around the vector width, the mask chunk and one / two workgroup spans of every U
    the launchers pick (forward, STE: 2 and 9 -> 2048, 9216 elements; K4: 4 and 8 -> 4096,
    8192), 8-byte aligned (vector path when n % 4 == 0) and one element off (scalar path)."""
    torch.manual_seed(11)
    place = (lambda t: t) if aligned else offset_view
    for n in EDGE_N:
        x0 = (torch.randn(n, device=DEV) * 3).to(dtype)
        g0 = torch.randn(n, device=DEV).to(dtype)
        x, g = place(x0), place(g0)
        xf, gf = x0.float(), g0.float()
        for act in (None, "relu"):
            y, m, c = FQ.fake_quant(x, 0.05, 0, -128, 127, want_mask=True, want_codes=True, act=act)
            yo, mo, co = FQ.fake_quant(xf, 0.05, 0, -128, 127, want_mask=True, want_codes=True, act=act)
            assert_bits(y, yo, f"fwd n={n}")
            assert torch.equal(c, co) and torch.equal(m, mo), n
            gx = FQ.ste_backward(g, mo, 0.05, pre=x if act else None, act=act)
            gxo = FQ.ste_backward(gf, mo, 0.05, pre=xf if act else None, act=act)
            assert_bits(gx, gxo, f"ste n={n}")
            kx, kg = FQ.lsq_backward(g, x, 0.05, 3.0, 0, 255, 0.01, 1, act=act)
            kxo, kgo = FQ.lsq_backward(gf, xf, 0.05, 3.0, 0, 255, 0.01, 1, act=act)
            assert_bits(kx, kxo, f"k4 n={n}")
            assert same_bits(kg, kgo), (n, kg.tolist(), kgo.tolist())


# --------------------------------------------------------------------------- 4. STE backward
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ste_backward_every_gradient_value(dtype, act):
    g = all_patterns(dtype)
    x = permuted(g)
    _, mask, _ = FQ.fake_quant(x, 0.05, 0, -128, 127, want_mask=True, act=act)
    _, mask32, _ = FQ.fake_quant(x.float(), 0.05, 0, -128, 127, want_mask=True, act=act)
    assert torch.equal(mask, mask32)
    gx = FQ.ste_backward(g, mask, 0.05, pre=x if act else None, act=act)
    gxo = FQ.ste_backward(g.float(), mask, 0.05, pre=x.float() if act else None, act=act)
    assert gx.dtype == dtype
    assert_bits(gx, gxo, "gx")


# --------------------------------------------------------------------------- 5. K4
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("zp_learn", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lsq_backward(dtype, zp_learn, act):
    """grad_x bit-equal; grad_out bit-equal too: the typed K4 keeps the fp32 launch's grid
    and fold order (both functions of n only)."""
    torch.manual_seed(3)
    qmin, qmax, zp = (0, 255, 37.0) if zp_learn else (-128, 127, 0.0)
    cases = [(all_patterns(dtype), permuted(all_patterns(dtype)))]
    for n in (4099, 3 * 4 * KBLOCK * LSQ_G[0] + 5):
        cases.append((torch.randn(n, device=DEV).to(dtype), (torch.randn(n, device=DEV) * 4).to(dtype)))
    for g, x in cases:
        gx, grads = FQ.lsq_backward(g, x, 0.05, zp, qmin, qmax, 0.02, zp_learn, act=act)
        gxo, gradso = FQ.lsq_backward(g.float(), x.float(), 0.05, zp, qmin, qmax, 0.02, zp_learn, act=act)
        assert gx.dtype == dtype
        assert_bits(gx, gxo, f"gx n={g.numel()}")
        assert same_bits(grads, gradso), (g.numel(), grads.tolist(), gradso.tolist())
    assert torch.isfinite(grads).all() and float(grads[0]) != 0.0   # the randn case says something


def test_grad_output_dtype_must_match():
    x = torch.randn(64, device=DEV).bfloat16()
    with pytest.raises(TypeError, match="float32"):
        FQ.lsq_backward(torch.randn(64, device=DEV), x, 0.05, 0, -128, 127, 1.0, 0)
    _, mask, _ = FQ.fake_quant(x, 0.05, 0, -128, 127, want_mask=True, act="relu")
    with pytest.raises(TypeError, match="float16"):
        FQ.ste_backward(x, mask, 0.05, pre=x.half(), act="relu")


# --------------------------------------------------------------------------- 6. observer
def _observe(x, state, act=None, symmetric=False):
    run = torch.tensor(state, dtype=torch.float32, device=DEV)
    qp, st = FQ.observe_tensor(x, symmetric=symmetric, run_minmax=run, act=act)
    return qp, st, run


@pytest.mark.parametrize("dtype", DTYPES)
def test_observer_every_value(dtype):
    x = all_patterns(dtype)
    qp, st, run = _observe(x, [-1.0, 2.0])
    qpo, sto, runo = _observe(x.float(), [-1.0, 2.0])
    mant = 7 if dtype == torch.bfloat16 else 10
    assert float(st[H.ST_NAN]) == 2 * (2 ** mant - 1) == float(torch.isnan(x).sum())
    assert float(st[H.ST_N]) == 65536.0
    assert run.tolist() == [-1.0, 2.0]                       # a call holding a NaN changes nothing
    assert same_bits(st, sto) and same_bits(qp, qpo) and same_bits(run, runo)
    assert float(st[H.ST_MIN]) == -float("inf") and float(st[H.ST_MAX]) == float("inf")


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_observer_edges(dtype, act):
    """min / max / n / qparams / running state and (same grid and fold order) the f64 sums
    are the fp32 call's on the widened tensor, bit for bit; aligned and one element off."""
    torch.manual_seed(7)
    for n in EDGE_N + [70001, 600001]:                       # the last two: several workgroups / records
        x0 = (torch.randn(n, device=DEV) * 2).to(dtype)
        for x in (x0, offset_view(x0)):
            qp, st, run = _observe(x, [0.0, 0.0], act=act, symmetric=n % 2 == 0)
            qpo, sto, runo = _observe(x0.float(), [0.0, 0.0], act=act, symmetric=n % 2 == 0)
            assert same_bits(st, sto), (n, st.tolist(), sto.tolist())
            assert same_bits(qp, qpo) and same_bits(run, runo), n
            assert float(st[H.ST_N]) == n and float(st[H.ST_NAN]) == 0.0


# --------------------------------------------------------------------------- 7. public path
def _layer(a_sym):
    from vsiquantization_amd.modules.fused import ConvBnReLU
    torch.manual_seed(2)
    cv = nn.Conv2d(2, 4, 3, padding=1, bias=False)
    bn = nn.BatchNorm2d(4)
    bn.running_mean.uniform_(-0.2, 0.2)
    bn.running_var.uniform_(0.5, 2.0)
    m = ConvBnReLU(cv, bn, nn.ReLU(), "MinMaxObserver", "UniformQuantizer", "MinMaxObserver", "UniformQuantizer",
                   True, a_sym, True, 8, 8).to(DEV)
    qms = (m.weight_quantizer, m.activation_quantizer)
    for qm in qms:   # calibrate one batch in fp32: observe and quantize
        qm.is_learning_scale, qm.is_observer_qparam, qm.is_quantize = False, True, True
    m(torch.randn(2, 2, 8, 8, device=DEV))
    return m, qms


@pytest.mark.parametrize("mode", ["fixed", "learn"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_layer_under_autocast(dtype, mode):
    """ConvBnReLU under torch.autocast: the conv output reaches the activation quantizer in
    T and goes through the typed K5 / STE (fixed qparams) or K5 / K4 (learnable scale).
    The conv output is captured at the quantizer's entry (the layer calls F.conv2d, so no
    module hook sees it)."""
    m, qms = _layer(a_sym=True)
    for qm in qms:
        if mode == "fixed":
            qm.is_observer_qparam = False
        else:
            qm.is_learning_scale = True
            qm.init_scaling_factor_for_learning()
            qm.make_learn_qparameter()
    aq = m.activation_quantizer
    seen = []
    inner = aq.quantize
    aq.quantize = lambda c, act=None: (seen.append(c), inner(c, act=act))[1]
    x = torch.randn(2, 2, 8, 8, device=DEV, requires_grad=True)
    with torch.autocast("cuda", dtype=dtype):
        y = m(x)
    aq.quantize = inner
    (c,) = seen
    assert c.dtype == dtype and y.dtype == dtype and y.shape == (2, 4, 8, 8)
    saved = [t for t in y.grad_fn.saved_tensors if t.shape == c.shape]
    assert len(saved) == 1 and saved[0].dtype == dtype            # the pre-activation stays 16-bit
    y.float().square().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().sum()) > 0
    if mode == "learn":
        assert aq.scale.grad is not None and torch.isfinite(aq.scale.grad).all() and float(aq.scale.grad) != 0.0
    with torch.no_grad():
        got = aq.quantize(c.detach(), act="relu")
        exp = aq.quantize(c.detach().float(), act="relu")
    assert got.dtype == dtype and same_bits(got, y.detach())
    assert_bits(got, exp, "manager.quantize")


@pytest.mark.parametrize("dtype", DTYPES)
def test_manager_observes_and_quantizes_half(dtype):
    """Per-call observe + quantize of a half tensor: the typed K2 then K5; the running state,
    qparams and recorded statistics are those of the widened tensor."""
    from vsiquantization_amd import QuantizationManager
    torch.manual_seed(4)
    x = (torch.randn(3, 5, 7, 11, device=DEV) * 2).to(dtype)
    out = []
    for t in (x, x.float()):
        qm = QuantizationManager("UniformQuantizer", "MinMaxObserver", 8, False, is_learning_scale=False)
        qm.is_observer_qparam, qm.is_quantize = True, True
        y = qm.quantize(t, act="relu")
        out.append((y, qm.observer.min_val, qm.observer.max_val, float(qm.scale), float(qm.zero_point),
                    list(qm.mean_abs_x), list(qm.mean_x), list(qm.std)))
    (y, *a), (yo, *b) = out
    assert y.dtype == dtype and a == b
    assert_bits(y, yo, "observe + quantize")


# --------------------------------------------------------------------------- 8. fp32-only paths
def test_f32_only_paths_raise_on_half():
    from vsiquantization_amd import QuantizationManager
    x = torch.randn(4, 6, 8, device=DEV).bfloat16()
    scale = torch.full((4,), 0.05, device=DEV)
    with pytest.raises(TypeError, match="bfloat16"):
        FQ.per_channel_fake_quant(x, scale, None, -128, 127)
    with pytest.raises(TypeError, match="bfloat16"):
        FQ.per_channel_observe_fq(x, symmetric=True, qmin=-128, qmax=127)
    with pytest.raises(TypeError, match="bfloat16"):
        FQ.observe_fake_quant(x, symmetric=True, qmin=-128, qmax=127)                 # K8
    with pytest.raises(TypeError, match="bfloat16"):
        FQ.observe_fake_quant(x, symmetric=True, qmin=-128, qmax=127, parts=True)     # K9
    with pytest.raises(TypeError, match="bfloat16"):
        FQ.observe_parts(x)                                                           # K2p
    with pytest.raises(TypeError, match="bfloat16"):
        FQ.ActivationFn.apply(x, "relu")
    _, mask, _ = FQ.fake_quant(x.float(), 0.05, 0, -128, 127, want_mask=True)
    with pytest.raises(TypeError, match="bfloat16"):
        FQ.ste_backward(x, mask, scale.double(), 48)                                  # per-row scales
    qm = QuantizationManager("UniformQuantizer", "MinMaxObserver", 8, True, is_learning_scale=False)
    qm.is_observer_qparam, qm.is_quantize, qm.dist_defer = True, False, True          # deferred calibration
    with pytest.raises(TypeError, match="bfloat16"):
        qm.quantize(x)
    qm = QuantizationManager("UniformQuantizer", "MinMaxObserver", 8, True, is_learning_scale=False)
    qm.is_observer_qparam, qm.is_quantize = True, True
    H.set_mean_reference(8)
    try:
        with pytest.raises(TypeError, match="bfloat16"):
            qm.quantize(x)                                                            # K11
    finally:
        H.clear_mean_reference()
