"""bf16 / fp16 activations through the records-only learnable backward (K4d, ABI 13:
vsiq_act_lsq_bwd_part_t) and the deferred qparam-gradient fold above it.

The rule under test is ABI 12's: a typed call is vsiq_act_lsq_bwd_part_f32 on the exactly
widened inputs with grad_x rounded once to T (nearest even); the per-workgroup records
{sum t, sum z} are the fp32 call's bit for bit, because their count and layout depend on n
(and VSIQ_TUNE_LSQ_GROUPS) only.  So the oracle everywhere is this library's own fp32 entry
on ``x.float()`` / ``g.float()`` followed by torch's ``.to(T)``; tensors are compared as
raw 16-bit patterns, records and gradients as raw 64-bit patterns.
"""
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from vsiquantization_amd import _hip as H                      # noqa: E402
from vsiquantization_amd import fakequant as FQ                # noqa: E402
from vsiquantization_amd.quantizers import deferred as D       # noqa: E402

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
ACTS = [None, "relu", "silu"]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vsiquantization_amd", "csrc")
# (qmin, qmax, scale, zero point): sym int8, asym uint8, 4-bit (tests/test_gpu_half.py)
CONFIGS = [(-128, 127, 0.05, 0), (0, 255, 0.02, 37), (-8, 7, 0.3, 0)]

# K4d's workgroup span (elements) is 4 * kBlock * groups per lane; 2 groups per lane below
# 48 Mi elements, 4 from there (test_span_matches_the_source reads them from the source)
KBLOCK, PART_G, PART_G_LARGE, PART_LARGE_N = 256, 2, 4, 48 << 20
SPAN = 4 * KBLOCK * PART_G
EDGE_N = [1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 2052, 4095, 4096, 4097]
SENTINEL = 0x7FF8DEAD0000BEEF   # a NaN no sum produces: the records' unwritten words
PAD = 6                         # doubles past the call's records


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
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def offset_view(x):
    """x's values at an address one element past an aligned one: the scalar path"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:].copy_(x)
    v = buf[1:]
    assert v.is_contiguous() and v.data_ptr() % 8 != 0
    return v


def nrec_of(n):
    return int(H.lib().vsiq_lsq_part_records(H.c_i64(n)))


def new_records(n):
    """2 * nrec doubles for a call over n elements + PAD more, every word the sentinel"""
    return torch.full((2 * nrec_of(n) + PAD,), SENTINEL, dtype=torch.int64, device=DEV).view(torch.float64)


def typed_part(g, x, s, zp, qmin, qmax, zpl, act):
    """(grad_x, records incl. the pad) of the entry under test, through its Python wrapper"""
    rec = new_records(g.numel())
    gx, _, _ = D.lsq_backward_part(g, x, s, zp, qmin, qmax, zpl, act, rec)
    return gx, rec


def f32_part(g, x, s, zp, qmin, qmax, zpl, act):
    """The oracle: vsiq_act_lsq_bwd_part_f32 itself (not the typed entry at VSIQ_DT_F32)."""
    assert g.dtype == x.dtype == torch.float32 and g.is_contiguous() and x.is_contiguous()
    rec = new_records(g.numel())
    gx = torch.empty_like(g)
    rc = H.lib().vsiq_act_lsq_bwd_part_f32(H.ptr(g), H.ptr(x), H.ptr(gx), H.c_i64(g.numel()), H.act_code(act), None,
                                           float(s), None, float(zp), int(zpl), qmin, qmax, H.ptr(rec),
                                           H.c_i64(rec.numel()), H.stream_of(g.device))
    H.check(rc, "vsiq_act_lsq_bwd_part_f32")
    return gx, rec


def check_records(rec, reco, n, what=""):
    """the typed call fills exactly vsiq_lsq_part_records(n) records, with the fp32 call's
    bits, and leaves every word past them alone"""
    k = 2 * nrec_of(n)
    r, ro = rec.view(torch.int64), reco.view(torch.int64)
    assert r.numel() == k + PAD
    assert bool((r[k:] == SENTINEL).all()), f"{what}: words past the records were written"
    assert not bool((r[:k] == SENTINEL).any()), f"{what}: a record was not written"
    bad = (r[:k] != ro[:k]).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} of {k} record words differ, first at {int(bad[0])}"


def test_span_matches_the_source():
    """kBlock, the groups per lane and the 48 Mi threshold EDGE_N and the spans below are
    built from are the launcher's, read from the source; the record count follows them."""
    common = open(os.path.join(CSRC, "vsiq_common.cuh")).read()
    assert int(re.search(r"constexpr int kBlock = (\d+);", common).group(1)) == KBLOCK
    src = open(os.path.join(CSRC, "k_lsq.cuh")).read()
    m = re.search(r"return g > 0 \? g : \(n >= \(\(int64_t\)(\d+) << 20\) \? (\d+) : (\d+)\);", src)
    assert (int(m.group(1)) << 20, int(m.group(3)), int(m.group(2))) == (PART_LARGE_N, PART_G, PART_G_LARGE)
    # one launcher for every element type: the grid comes from that function alone
    assert re.search(r"template <typename T>\s*int lsq_bwd_part\(", src)
    assert re.search(r"grid = lsq_grid\(cdiv\(n, 4\), lsq_part_groups_per_lane\(n\)\);", src)
    assert SPAN == 2048 and {SPAN - 1, SPAN, SPAN + 1, SPAN + 4, 2 * SPAN - 1, 2 * SPAN, 2 * SPAN + 1} <= set(EDGE_N)
    for n in EDGE_N:
        assert nrec_of(n) == -(-n // SPAN), n
    big = 4 * KBLOCK * PART_G_LARGE
    assert nrec_of(PART_LARGE_N - 4) == -(-(PART_LARGE_N - 4) // SPAN)
    assert nrec_of(PART_LARGE_N) == PART_LARGE_N // big


# --------------------------------------------------------------------------- 1. every value
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("zp_learn", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_input_value(dtype, zp_learn, act):
    x = permuted(all_patterns(dtype), 5)
    g = permuted(all_patterns(dtype), 9)
    xf, gf = x.float(), g.float()
    for qmin, qmax, s, zp in CONFIGS:
        gx, rec = typed_part(g, x, s, zp, qmin, qmax, zp_learn, act)
        gxo, reco = f32_part(gf, xf, s, zp, qmin, qmax, zp_learn, act)
        assert gx.dtype == dtype and gx.shape == x.shape
        assert_bits(gx, gxo, f"gx {qmin}..{qmax}")
        check_records(rec, reco, x.numel(), f"records {qmin}..{qmax}")


# --------------------------------------------------------------------------- 2. edges
def _edge_case(dtype, n, aligned, seed):
    torch.manual_seed(seed)
    x0 = (torch.randn(n, device=DEV) * 3).to(dtype)
    g0 = torch.randn(n, device=DEV).to(dtype)
    place = (lambda t: t) if aligned else offset_view
    x, g = place(x0), place(g0)
    for act, (qmin, qmax, s, zp), zpl in ((None, CONFIGS[1], 1), ("relu", CONFIGS[2], 0)):
        gx, rec = typed_part(g, x, s, zp, qmin, qmax, zpl, act)
        gxo, reco = f32_part(g0.float(), x0.float(), s, zp, qmin, qmax, zpl, act)
        assert_bits(gx, gxo, f"gx n={n} aligned={aligned}")
        check_records(rec, reco, n, f"records n={n} aligned={aligned}")
        finite = rec[:2 * nrec_of(n)]
        assert bool(torch.isfinite(finite).all()) and (n < 64 or float(finite[0::2].abs().sum()) > 0.0)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_of_the_grid_and_the_scalar_path(dtype, aligned):
    """n around the vector width, a wave, and one / two workgroup spans of the default 2
    groups per lane (2048 elements); 8-byte aligned (vector path when n % 4 == 0) and one
    element off (scalar path): same grad_x, same records."""
    for n in EDGE_N:
        _edge_case(dtype, n, aligned, 11)


@pytest.mark.parametrize("groups", [4, 8, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_at_tuned_groups_per_lane(dtype, groups):
    span = 4 * KBLOCK * groups
    H.set_tuning(H.TUNE_LSQ_GROUPS, groups)
    try:
        for n in (span - 1, span, span + 1, 2 * span + 4):
            assert nrec_of(n) == -(-n // span), n
            for aligned in (True, False):
                _edge_case(dtype, n, aligned, 13)
    finally:
        H.set_tuning(H.TUNE_LSQ_GROUPS, 0)
    assert nrec_of(span) == span // SPAN


def test_grad_output_dtype_must_match():
    x = torch.randn(64, device=DEV).bfloat16()
    rec = new_records(64)
    with pytest.raises(TypeError, match="float32"):
        D.lsq_backward_part(torch.randn(64, device=DEV), x, 0.05, 0, -128, 127, 0, None, rec)
    with pytest.raises(TypeError, match="float16"):
        D.lsq_backward_part(x, x.half(), 0.05, 0, -128, 127, 0, None, rec)


# --------------------------------------------------------------------------- 3. the fold
def _entry(g, x, s, zp, qmin, qmax, zpl, act, gscale):
    e = D._Fold()
    e.nrec = nrec_of(g.numel())
    e.records = torch.empty(2 * e.nrec, dtype=torch.float64, device=DEV)
    gx, e.zd, e.zh = D.lsq_backward_part(g, x, s, zp, qmin, qmax, zpl, act, e.records)
    e.gscale, e.qmin, e.qmax, e.learn_zp = gscale, qmin, qmax, bool(zpl)
    e.out = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    return e


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_fold_over_typed_and_f32_calls(dtype):
    """One vsiq_lsq_fold_multi launch over three typed and three fp32 calls == the fold over
    the six fp32 calls on the widened tensors.  The largest call has more records than one
    chunk workgroup of the fold takes (1024)."""
    torch.manual_seed(17)
    calls = []
    for i, n in enumerate((4099, 70001, SPAN * 1030 + 8, 2048, 33333, 300000)):
        x = (torch.randn(n, device=DEV) * 3).to(dtype)
        g = torch.randn(n, device=DEV).to(dtype)
        qmin, qmax, s, zp = CONFIGS[i % 3]
        calls.append((g, x, s, zp, qmin, qmax, i % 2, ACTS[i % 3], 0.01 * (i + 1)))
    assert nrec_of(calls[2][0].numel()) > 1024
    mixed = [_entry(*(c if i < 3 else (c[0].float(), c[1].float()) + c[2:])) for i, c in enumerate(calls)]
    wide = [_entry(c[0].float(), c[1].float(), *c[2:]) for c in calls]
    D.fold(mixed)
    D.fold(wide)
    for i, (a, b) in enumerate(zip(mixed, wide)):
        assert same_bits(a.out, b.out), (i, a.out.tolist(), b.out.tolist())
        assert bool(torch.isfinite(a.out).all()) and float(a.out[0]) != 0.0
        assert (float(a.out[1]) != 0.0) == bool(i % 2), i


# --------------------------------------------------------------------------- 4. autograd
def _qparams(s, zp, learn_zp):
    sp = nn.Parameter(torch.tensor(s, dtype=torch.float64, device=DEV))
    zpp = nn.Parameter(torch.tensor(float(zp), dtype=torch.float64, device=DEV)) if learn_zp else zp
    return sp, zpp


def _deferred_step(x, g, cfg, learn_zp, act, gscale):
    """DeferredLearnFn behind a bundle node, as the model-level hook builds it"""
    qmin, qmax, s, zp = cfg
    sp, zpp = _qparams(s, zp, learn_zp)
    views = D.QParamBundleFn.apply(*([sp, zpp] if learn_zp else [sp]))
    xi = x.clone().requires_grad_(True)
    y = D.DeferredLearnFn.apply(xi, views[0], views[1] if learn_zp else zpp, qmin, qmax, gscale, learn_zp, act)
    assert "DeferredLearnFn" in type(y.grad_fn).__name__
    y.backward(g)
    assert D.pending_count() == 0
    return y.detach(), xi.grad, sp.grad, (zpp.grad if learn_zp else None)


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("learn_zp", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_deferred_learn_fn_on_half(dtype, learn_zp, act):
    """learn_zp False: a UniformQuantizer's call (sym, 4-bit); True: an LSQQuantizer's
    (asym uint8, learned zero point)."""
    torch.manual_seed(19)
    n = 3 * SPAN + 5
    x = (torch.randn(n, device=DEV) * 3).to(dtype)
    g = torch.randn(n, device=DEV).to(dtype)
    cfg = CONFIGS[1] if learn_zp else CONFIGS[2]
    gscale = (cfg[1] * n) ** -0.5
    y, gx, gs, gz = _deferred_step(x, g, cfg, learn_zp, act, gscale)
    # y and x.grad: FakeQuantLearnFn (the per-call K4) on the same half tensor
    qmin, qmax, s, zp = cfg
    sp, zpp = _qparams(s, zp, learn_zp)
    xi = x.clone().requires_grad_(True)
    yo = FQ.FakeQuantLearnFn.apply(xi, sp, zpp, qmin, qmax, gscale, int(learn_zp), act)
    yo.backward(g)
    assert y.dtype == gx.dtype == dtype
    assert same_bits(y, yo.detach()) and same_bits(gx, xi.grad)
    # the folded gradients: the fp32 DeferredLearnFn on the widened x and g
    _, _, gso, gzo = _deferred_step(x.float(), g.float(), cfg, learn_zp, act, gscale)
    assert gs.dtype == torch.float64 and same_bits(gs, gso), (gs.item(), gso.item())
    assert float(gs) != 0.0 and bool(torch.isfinite(gs))
    if learn_zp:
        assert same_bits(gz, gzo) and float(gz) != 0.0


def test_backward_rejects_a_grad_output_of_another_dtype():
    """autograd casts a mismatched grad_output before a Function sees it, so the check is
    reached by handing the backward function its arguments directly"""
    x = torch.randn(64, device=DEV).bfloat16()
    ctx = types.SimpleNamespace(saved_tensors=(x,), args=(-128, 127, 1.0, False, None), scale=0.05, zp=0,
                                needs_input_grad=(True,) * 8)
    with pytest.raises(TypeError, match=r"float32.*bfloat16"):
        D.DeferredLearnFn.backward(ctx, torch.randn(64, device=DEV))
    with pytest.raises(TypeError, match=r"float16.*bfloat16"):
        D.DeferredLearnFn.backward(ctx, torch.randn(64, device=DEV).half())
    assert D.pending_count() == 0


# --------------------------------------------------------------------------- 5. the model
@pytest.fixture()
def deterministic_convs():
    prev = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    yield
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = prev


class _Fp32Island(nn.Module):
    """its layer outside autocast: an fp32 activation quantizer in a half model"""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x):
        with torch.autocast("cuda", enabled=False):
            return self.layer(x.float())


def _model(launches, island):
    """Three fused ConvBnReLU layers 2 -> 4 -> 4 -> 4 (w4 / a4; the last activation quantizer
    an asymmetric LSQQuantizer with a learned zero point), calibrated on one fp32 batch, then
    the reference's training sequence."""
    from vsiquantization_amd.modules.fused import ConvBnReLU
    from vsiquantization_amd.utils.quantize_manager import (activate_learning_qparam, activate_quantizer,
                                                            calibrate_qat_model, data_calib)
    torch.manual_seed(0)
    layers = []
    for i, (cin, cout) in enumerate(((2, 4), (4, 4), (4, 4))):
        bn = nn.BatchNorm2d(cout)
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
        qa, a_sym = ("LSQQuantizer", False) if i == 2 else ("UniformQuantizer", True)
        layers.append(ConvBnReLU(nn.Conv2d(cin, cout, 3, padding=1, bias=False), bn, nn.ReLU(), "MinMaxObserver",
                                 "UniformQuantizer", "MinMaxObserver", qa, True, a_sym, True, 4, 4))
    fused = list(layers)
    if island:
        layers[0] = _Fp32Island(layers[0])
    m = nn.Sequential(*layers).to(DEV)
    gen = torch.Generator().manual_seed(1)
    loader = [(torch.randint(0, 256, (2, 2, 8, 8), generator=gen, dtype=torch.uint8), None)]
    calibrate_qat_model(m, loader, data_calib, DEV)
    activate_learning_qparam(m, use_init=True, model_launches=launches)
    activate_quantizer(m, model_launches=launches)
    m.to(DEV)
    m.train()
    return m, fused


def _step(m, fused, dtype):
    """one forward / backward under autocast -> (y, x.grad, per layer (input dtype, grad_fn
    type name, grad_fn.name() -- a C++ node's type is CppFunction) of the activation
    quantizer, parameter gradients)"""
    seen, inner = [], []
    for layer in fused:
        aq = layer.activation_quantizer
        inner.append(aq.quantize)

        def spy(c, act=None, _q=aq.quantize):
            y = _q(c, act=act)
            seen.append((c.dtype, type(y.grad_fn).__name__, y.grad_fn.name()))
            return y
        aq.quantize = spy
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(0, 256, (2, 2, 8, 8), generator=g, dtype=torch.uint8).float() / 255).to(DEV)
    x.requires_grad_(True)
    try:
        with torch.autocast("cuda", dtype=dtype):
            y = m(x)
        y.float().square().mean().backward()
    finally:
        for layer, q in zip(fused, inner):
            layer.activation_quantizer.quantize = q
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    return y.detach(), x.grad, seen, grads


@pytest.mark.parametrize("island", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_model_launches_under_autocast(dtype, island, deterministic_convs):
    """The default training configuration under torch.autocast: every activation quantizer
    runs its backward records-only (K4d) and ONE fold per backward produces the qparam
    gradients -- with ``island`` over an fp32 call and two half calls together."""
    import vsiquantization_amd as V
    a, fa = _model(None, island)
    b, fb = _model(False, island)
    assert V.model_launches_enabled(a) and not V.model_launches_enabled(b)
    ya, gxa, seen_a, ga = _step(a, fa, dtype)
    assert D.pending_count() == 0
    yb, gxb, seen_b, gb = _step(b, fb, dtype)
    want = [torch.float32 if island else dtype, dtype, dtype]
    assert [s[0] for s in seen_a] == want == [s[0] for s in seen_b]
    for (_, name_a, _), (_, name_b, _) in zip(seen_a[(1 if island else 0):], seen_b[(1 if island else 0):]):
        assert "DeferredLearnFn" in name_a, name_a          # the half calls: the Python Function
        assert "FakeQuantLearnFn" in name_b, name_b
    if island:   # the fp32 call: the deferred node too (C++ or Python), not the per-call one
        assert "Deferred" in seen_a[0][2] and "Deferred" not in seen_b[0][2], (seen_a[0], seen_b[0])
    assert ya.dtype == dtype and same_bits(ya, yb)
    assert gxa is not None and float(gxa.abs().sum()) > 0 and same_bits(gxa, gxb)
    assert ga.keys() == gb.keys()
    act_scales = [n for n in ga if n.endswith("activation_quantizer.scale")]
    assert len(act_scales) == 3 and any(n.endswith("activation_quantizer.zero_point") for n in ga)
    assert len([n for n in ga if n.endswith("weight_quantizer.scale")]) == 3
    for n in ga:
        if "activation_quantizer" in n:   # K4d fold vs K4's in-kernel fold: f64 summation order
            assert ga[n].dtype == torch.float64 and bool(torch.isfinite(ga[n]).all())
            np.testing.assert_allclose(ga[n].cpu().numpy(), gb[n].cpu().numpy(), rtol=1e-12, atol=0, err_msg=n)
        else:
            assert same_bits(ga[n], gb[n]), n
    assert all(float(ga[n]) != 0.0 for n in act_scales)


# --------------------------------------------------------------------------- 6. still per-call
@pytest.mark.parametrize("why", ["calib_grad_scale tensor", "symmetric tensor zero point"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ineligible_managers_stay_per_call(dtype, why, deterministic_convs):
    """A per-channel calib_grad_scale, or a symmetric quantizer handed a gradient-requiring
    zero point (K4 zp_learn 2), keeps the per-call K4 for half tensors as for fp32."""
    m, fused = _model(None, False)
    aq = fused[1].activation_quantizer
    assert aq.quantizer.symmetric
    if why == "calib_grad_scale tensor":
        aq.quantizer.calib_grad_scale = torch.tensor([0.5, 0.25, 1.0, 0.25], device=DEV)
    else:
        aq.zero_point = nn.Parameter(torch.tensor(0.25, dtype=torch.float64, device=DEV))
    y, gx, seen, grads = _step(m, fused, dtype)
    assert D.pending_count() == 0
    assert [s[0] for s in seen] == [dtype] * 3
    assert "DeferredLearnFn" in seen[0][1] and "DeferredLearnFn" in seen[2][1]
    assert "Deferred" not in seen[1][1] and "FakeQuantLearnFn" in seen[1][1], seen[1]
    gs = grads["1.activation_quantizer.scale"]
    assert bool(torch.isfinite(gs)) and float(gs) != 0.0
    if why != "calib_grad_scale tensor":
        assert bool(torch.isfinite(grads["1.activation_quantizer.zero_point"]))
    assert float(gx.abs().sum()) > 0 and y.dtype == dtype
