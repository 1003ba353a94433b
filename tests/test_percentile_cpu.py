"""PercentileObserver without a GPU: registry and ABI, argument checks of both entry points,
the native host loop against the numpy oracle (tests/percentile_common.py) bit for bit,
the invariants of the definition and the fused-layer calibration flow on CPU tensors."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests.percentile_common import (BINS, FAMILIES, OUTLIER, PERCENTILES, OracleObserver, k2_minmax, make_input,
                                     oracle_clip, same_bits, tail_of)
from vsiquantization_amd import _hip as H
from vsiquantization_amd.fakequant import observe_percentile, observe_tensor
from vsiquantization_amd.modules.fused import ConvBnReLU
from vsiquantization_amd.observers import MinMaxObserver, PercentileObserver
from vsiquantization_amd.utils.quantize_manager import calibrate_qat_model
from vsiquantization_amd.utils.registry import CLASS_REGISTRY

SIZES = (1, 3, 5, 1023, 1025, 65537)


# ------------------------------------------------------------------ 1. registry, construction
def test_registry_and_construction():
    obs = CLASS_REGISTRY["PercentileObserver"](True)
    assert isinstance(obs, PercentileObserver) and isinstance(obs, MinMaxObserver)
    assert (obs.symmetric, obs.num_bits, obs.eps, obs.percentile, obs.bins) == (True, 8, 1e-8, 99.99, 2048)
    assert not obs.single_pass and MinMaxObserver.single_pass and CLASS_REGISTRY["LSQObserver"].single_pass
    assert repr(obs) == "PercentileObserver(symmetric=True, num_bits=8, eps=1e-08, percentile=99.99, bins=2048)"
    qm = V.QuantizationManager("UniformQuantizer", "PercentileObserver", 8, False)
    assert isinstance(qm.observer, PercentileObserver) and qm.observer.symmetric is False


def test_symbols_bound_and_abi_unchanged():
    lib = H.lib()
    for name in ("vsiq_act_observe_hist_f32", "vsiq_host_observe_hist_f32"):
        assert name in H.EXPORTED and hasattr(lib, name)
    assert H.ABI_VERSION == 13 and lib.vsiq_abi_version() == 13


def test_percentile_and_bins_are_validated():
    x = torch.randn(100)
    for p in (50.0, 49.0, 100.5, float("nan")):
        obs = PercentileObserver(percentile=p)
        with pytest.raises(ValueError):
            obs.observe(x)
    for b in (128, 8192, 1000, 0):
        obs = PercentileObserver(bins=b)
        with pytest.raises(ValueError):
            obs.observe(x)


# ------------------------------------------------------------------ 2. argument checks
def _buf(n, dtype):
    t = torch.zeros(n, dtype=dtype)
    return t, H.ptr(t)


def test_argument_checks_without_a_launch():
    lib = H.lib()
    x, px = _buf(8, torch.float32)
    st, pst = _buf(H.ST_LEN, torch.float64)
    hist, ph = _buf(4096, torch.int64)
    cnt, pc = _buf(H.COUNTER_WORDS, torch.int32)
    run, pr = _buf(2, torch.float32)
    qp, pq = _buf(H.QP_LEN, torch.float64)
    clip, pcl = _buf(2, torch.float64)
    n8, hl = H.c_i64(8), H.c_i64(4096)

    def dev(c=px, n=n8, stats=pst, bins=2048, tail=0.01, h=ph, hlen=hl, counter=pc, cl=pcl):
        return lib.vsiq_act_observe_hist_f32(c, n, 0, stats, bins, tail, h, hlen, counter, pr, pq, cl, 1, 127.0, 1e-8,
                                             None)

    def hst(c=px, n=n8, stats=pst, bins=2048, tail=0.01, h=ph, hlen=hl, cl=pcl):
        return lib.vsiq_host_observe_hist_f32(c, n, 0, stats, bins, tail, h, hlen, pr, pq, cl, 1, 127.0, 1e-8)

    E_ARG, E_WS = -1, -3
    for f in (dev, hst):
        assert f(c=None) == E_ARG and f(stats=None) == E_ARG and f(h=None) == E_ARG and f(cl=None) == E_ARG
        assert f(n=H.c_i64(0)) == E_ARG and f(n=H.c_i64(-4)) == E_ARG
        for bins in (0, 128, 255, 1000, 3072, 8192, -2048):
            assert f(bins=bins) == E_ARG, bins
        for tail in (-1e-9, 0.5, 0.75, float("nan"), float("inf")):
            assert f(tail=tail) == E_ARG, tail
        assert f(hlen=H.c_i64(2047)) == E_WS and f(bins=4096, hlen=H.c_i64(2048)) == E_WS
    assert dev(counter=None) == E_ARG
    assert not hist.any() and not cnt.any()


# ------------------------------------------------------------------ 3. host loop == oracle
def _three_calls(family, n):
    xs = [make_input(family, n, seed) for seed in (1, 2, 3)]
    xs[1] = xs[1] * 0.5 if family != "constant" else xs[1]
    return xs


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_equals_oracle_bit_for_bit(family, symmetric):
    for n in SIZES:
        xs = _three_calls(family, n)
        for bins in BINS:
            for pct in PERCENTILES:
                state = torch.zeros(2, dtype=torch.float32)
                ref = OracleObserver(symmetric)
                qm = V.QuantizationManager("UniformQuantizer", "PercentileObserver", 8, symmetric, False)
                qm.is_quantize = False
                qm.observer.percentile, qm.observer.bins = pct, bins
                for x in xs:
                    qp, st, clip = observe_percentile(x, symmetric=symmetric, run_minmax=state, tail=tail_of(pct),
                                                      bins=bins)
                    mn, mx, has_nan = k2_minmax(st)
                    valid = x[~torch.isnan(x)]
                    if valid.numel():   # (a lone NaN: the record's +inf / -inf)
                        assert mn == valid.min().item() and mx == valid.max().item()
                    lo, hi = oracle_clip(x.numpy(), mn, mx, tail_of(pct), bins)
                    ref.update(lo, hi, has_nan)
                    tag = (family, n, bins, pct)
                    assert same_bits(clip, np.array([lo, hi], dtype=np.float64)), tag
                    assert same_bits(state, np.array([ref.mn, ref.mx], dtype=np.float32)), tag
                    assert same_bits(qp, ref.qp_record()), tag
                    assert mn <= lo <= hi <= mx or has_nan, tag
                    # the stats record is the unclipped tensor's: K2's own
                    _, st2 = observe_tensor(x, symmetric=symmetric, want_qp=False)
                    assert same_bits(st, st2), tag
                    qm.collect_qparameter(x)
                    s, z = ref.qparams()
                    assert qm.scale == s and qm.zero_point == int(z) and isinstance(qm.zero_point, int), tag


def test_host_relu_is_the_loop_on_the_activated_tensor():
    x = make_input("outliers", 65537, 5)
    a = torch.zeros(2)
    b = torch.zeros(2)
    ra = observe_percentile(x, symmetric=False, run_minmax=a, tail=1e-3, bins=256, act="relu")
    rb = observe_percentile(torch.relu(x), symmetric=False, run_minmax=b, tail=1e-3, bins=256)
    assert same_bits(a, b) and all(same_bits(p, q) for p, q in zip(ra, rb))


# ------------------------------------------------------------------ 4. invariants
@pytest.mark.parametrize("symmetric", [True, False])
def test_percentile_100_is_minmax(symmetric):
    p = V.QuantizationManager("UniformQuantizer", "PercentileObserver", 8, symmetric, False)
    m = V.QuantizationManager("UniformQuantizer", "MinMaxObserver", 8, symmetric, False)
    p.observer.percentile = 100
    for qm in (p, m):
        qm.is_quantize = False
    for family in FAMILIES:
        for n in (5, 1025, 65537):
            x = make_input(family, n, 4)
            for qm in (p, m):
                qm.collect_qparameter(x)
            assert (p.scale, p.zero_point) == (m.scale, m.zero_point)
            assert same_bits(p.observer._state, m.observer._state)
    assert (p.observer.min_val, p.observer.max_val) == (m.observer.min_val, m.observer.max_val)
    for name in ("mean_abs_x", "mean_x", "std"):
        assert same_bits(np.array(getattr(p, name)), np.array(getattr(m, name)))


def test_planted_outliers_are_clipped():
    x = make_input("outliers", 65537, 1)
    _, st, clip = observe_percentile(x, symmetric=True, tail=tail_of(99.99), bins=2048)
    lo, hi = clip.tolist()
    assert float(st[H.ST_MAX]) == OUTLIER and float(st[H.ST_MIN]) == -OUTLIER
    assert -OUTLIER < lo < -9.0 and 9.0 < hi < OUTLIER   # K = 6: five outliers per side go, randn * 3 stays
    assert hi <= 20.0 and lo >= -20.0


# ------------------------------------------------------------------ 5. fused-layer flow
def test_fused_layer_calibration_on_cpu_tensors():
    torch.manual_seed(0)
    cv = nn.Conv2d(3, 8, 3, padding=1, bias=False)
    bn = nn.BatchNorm2d(8)
    bn.running_var.uniform_(0.5, 2.0)
    layer = ConvBnReLU(cv, bn, nn.ReLU(), "MinMaxObserver", "UniformQuantizer", "PercentileObserver",
                       "UniformQuantizer", True, False, True, 8, 8)
    qa = layer.activation_quantizer
    qa.observer.percentile, qa.observer.bins = 99.0, 256
    g = torch.Generator().manual_seed(3)
    batches = [torch.randn(2, 3, 16, 16, generator=g) for _ in range(3)]
    captured = []
    layer.register_forward_hook(lambda _m, _i, out: captured.append(out.detach().clone()))

    def calib(model, loader, _device):
        for b in loader:
            model(b)

    calibrate_qat_model(layer, batches, calib)
    assert not qa._pending_records and not qa.dist_defer and qa.observer._defer_owner is None
    assert not layer.weight_quantizer._pending_records
    assert len(qa.mean_abs_x) == 3 and len(captured) == 3
    ref = OracleObserver(False)
    for y in captured:   # the layer's output in calibration is relu(pre-activation), unquantized
        v = y.reshape(-1).numpy()
        lo, hi = oracle_clip(v, v.min(), v.max(), tail_of(99.0), 256)
        assert hi < v.max()
        ref.update(lo, hi, False)
    s, z = ref.qparams()
    assert (qa.scale, qa.zero_point) == (s, int(z))
    assert (qa.observer.min_val, qa.observer.max_val) == (0, float(ref.mx))
