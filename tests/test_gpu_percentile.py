"""PercentileObserver on MI355X: the histogram pass (csrc/k_observe_hist.hip) against the host
loop and the numpy oracle (tests/percentile_common.py) bit for bit, the workspace's
histogram / counter discipline, the manager's routing and HIP-graph capture."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests.percentile_common import (BINS, FAMILIES, PERCENTILES, OracleObserver, k2_minmax, make_input, oracle_clip,
                                     same_bits, tail_of)
from vsiquantization_amd import _hip as H
from vsiquantization_amd.fakequant import activation, fake_quant, observe_percentile, qden
from vsiquantization_amd.modules.fused import ConvBnReLU
from vsiquantization_amd.utils.quantize_manager import calibrate_qat_model, data_calib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vsiquantization_amd", "csrc")


def _const(name, text):
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


def _sizes():
    """Read from the source: one workgroup's step, the one-workgroup threshold, the grid."""
    common = open(os.path.join(CSRC, "vsiq_common.cuh")).read()
    k2 = open(os.path.join(CSRC, "k_observe_k2.cuh")).read()
    block, u = _const("kBlock", common), _const("kObsU", common)
    assert "constexpr int64_t kObsSingle = (int64_t)kBlock * kObsU;" in k2
    step = 4 * block * u               # elements of one workgroup's step
    single = 4 * block * u             # kObsSingle groups: the largest one-workgroup tensor
    return step, single


STEP, SINGLE = _sizes()
# 1, 3, 5; a step +- 1; the first sizes of more than one workgroup (scalar path: n % 4 != 0)
# and their vector-path neighbours (n % 4 == 0); several whole steps
SMALL_N = sorted({1, 3, 5, STEP - 1, STEP, STEP + 1, SINGLE + 1, SINGLE + 2, SINGLE + 4, 4 * STEP})
BIG_N = 1_638_400   # C5's smallest layer: 200 workgroups, two-level arrival


def _stats_words(dev=DEV):
    w = H.workspace(torch.device(dev))
    return int(w.histogram().ne(0).sum()) + int(w.counter.ne(0).sum())


def _host_hist(x_act, st, bins, tail, state, symmetric):
    """The host loop on the device call's K2 record."""
    st = st.cpu().contiguous()
    qp = torch.empty(H.QP_LEN, dtype=torch.float64)
    clip = torch.empty(2, dtype=torch.float64)
    hist = torch.zeros(bins, dtype=torch.int64)
    rc = H.lib().vsiq_host_observe_hist_f32(H.ptr(x_act), H.c_i64(x_act.numel()), 0, H.ptr(st), bins, tail,
                                            H.ptr(hist), H.c_i64(bins), H.ptr(state), H.ptr(qp), H.ptr(clip),
                                            int(symmetric), qden(symmetric, 8, 1e-8), 1e-8)
    assert rc == 0 and not hist.any()
    return qp, clip


def _check_sequence(xs_cpu, symmetric, bins, pct, act=None, offset=False):
    """Successive calls on one running state: device == host loop == oracle."""
    dstate = torch.zeros(2, dtype=torch.float32, device=DEV)
    hstate = torch.zeros(2, dtype=torch.float32)
    ref = OracleObserver(symmetric)
    tail = tail_of(pct)
    for xc in xs_cpu:
        n = xc.numel()
        if offset:   # a view one element into a buffer: not 16-byte aligned, the scalar path
            x = torch.empty(n + 1, dtype=torch.float32, device=DEV)[1:]
            x.copy_(xc)
            assert x.data_ptr() % 16 != 0
        else:
            x = xc.to(DEV)
        qp, st, clip = observe_percentile(x, symmetric=symmetric, run_minmax=dstate, tail=tail, bins=bins, act=act)
        va = (activation(x, act) if act else x).cpu().contiguous()
        mn, mx, has_nan = k2_minmax(st)
        lo, hi = oracle_clip(va.numpy(), mn, mx, tail, bins)
        ref.update(lo, hi, has_nan)
        hqp, hclip = _host_hist(va, st, bins, tail, hstate, symmetric)
        tag = (n, symmetric, bins, pct, act, offset)
        assert same_bits(clip, np.array([lo, hi], dtype=np.float64)), tag
        assert same_bits(clip, hclip) and same_bits(qp, hqp) and same_bits(dstate, hstate), tag
        assert same_bits(dstate, np.array([ref.mn, ref.mx], dtype=np.float32)), tag
        assert same_bits(qp, ref.qp_record()), tag
        assert _stats_words() == 0, tag


# ------------------------------------------------------------------ 1. device == host == oracle
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_device_equals_host_and_oracle(family, symmetric):
    xs = [make_input(family, n, 1) for n in SMALL_N]
    for bins in BINS:
        for pct in PERCENTILES:
            _check_sequence(xs, symmetric, bins, pct)


@pytest.mark.parametrize("family", ["outliers", "relu"])
def test_large_tensor(family):
    xs = [make_input(family, BIG_N, 2), make_input(family, BIG_N + 3, 3)]
    for bins, pct, symmetric in ((2048, 99.99, True), (256, 99.0, False), (4096, 99.99, False)):
        _check_sequence(xs, symmetric, bins, pct)


def test_offset_views_take_the_scalar_path():
    xs = [make_input("outliers", n, 4) for n in (5, STEP, SINGLE + 4, 4 * STEP, 20 * STEP + 8)]
    for bins, pct in ((256, 99.0), (2048, 99.99)):
        _check_sequence(xs, False, bins, pct, offset=True)


@pytest.mark.parametrize("act", ["relu", "silu"])
def test_fused_activations(act):
    xs = [make_input("outliers", n, 5) for n in (5, STEP + 1, SINGLE + 4, 4 * STEP, 40 * STEP + 4)]
    for bins, pct, offset in ((256, 99.0, False), (2048, 99.99, False), (2048, 99.0, True)):
        _check_sequence(xs, True, bins, pct, act=act, offset=offset)


# ------------------------------------------------------------------ 2. buffer discipline
def test_back_to_back_calls_equal_each_alone():
    a = make_input("relu", BIG_N, 6).to(DEV)
    b = make_input("outliers", SINGLE + 4, 7).to(DEV)
    kw = dict(symmetric=False, tail=1e-3, bins=2048)

    def alone(x):
        s = torch.zeros(2, dtype=torch.float32, device=DEV)
        r = observe_percentile(x, run_minmax=s, **kw)
        torch.cuda.synchronize()
        return [t.clone() for t in r] + [s]

    ra, rb = alone(a), alone(b)
    sa = torch.zeros(2, dtype=torch.float32, device=DEV)
    sb = torch.zeros(2, dtype=torch.float32, device=DEV)
    qa = observe_percentile(a, run_minmax=sa, **kw)   # no sync in between: one stream orders them
    qb = observe_percentile(b, run_minmax=sb, **kw)
    qa2 = observe_percentile(a, run_minmax=None, **kw)
    torch.cuda.synchronize()
    for got, want in ((list(qa) + [sa], ra), (list(qb) + [sb], rb)):
        assert all(same_bits(g, w) for g, w in zip(got, want))
    assert same_bits(qa2[2], ra[2])
    assert _stats_words() == 0


# ------------------------------------------------------------------ 3. manager
def _manager(observer="PercentileObserver", sym=False, bits=8):
    qm = V.QuantizationManager("UniformQuantizer", observer, bits, sym, False)
    qm.is_observer_qparam, qm.is_learning_scale = True, False
    return qm


@pytest.mark.parametrize("n", [4096, 300_000])
def test_per_call_observe_and_quantize(n):
    qm = _manager(bits=4)
    qm.observer.percentile, qm.observer.bins = 99.0, 256
    ref = OracleObserver(False)
    for seed in (1, 2):
        xc = make_input("outliers", n, seed)
        x = xc.to(DEV)
        y = qm.quantize(x)
        lo, hi = oracle_clip(xc.numpy(), xc.min().item(), xc.max().item(), tail_of(99.0), 256)
        ref.update(lo, hi, False)
        s, z = ref.qparams()
        assert float(qm.scale) == s and float(qm.zero_point) == z
        want, _, _ = fake_quant(x, s, z, qm.quantizer.qmin, qm.quantizer.qmax)
        assert torch.equal(y, want)
    assert len(qm.mean_abs_x) == 2


def _model(middle):
    torch.manual_seed(0)
    layers = []
    for (cin, cout), obs in zip(((3, 16), (16, 32), (32, 32)), ("MinMaxObserver", middle, "MinMaxObserver")):
        cv = nn.Conv2d(cin, cout, 3, padding=1, bias=False)
        bn = nn.BatchNorm2d(cout)
        bn.running_var.uniform_(0.5, 2.0)
        layers.append(ConvBnReLU(cv, bn, nn.ReLU(), "MinMaxObserver", "UniformQuantizer", obs, "UniformQuantizer",
                                 True, False, True, 4, 4))
    return nn.Sequential(*layers).to(DEV)


def _loader(n=3):
    g = torch.Generator().manual_seed(1)
    return [(torch.randint(0, 256, (4, 3, 32, 32), generator=g, dtype=torch.uint8), None) for _ in range(n)]


def _layer_state(layer):
    out = []
    for qm in (layer.weight_quantizer, layer.activation_quantizer):
        out.append((qm.observer.min_val, qm.observer.max_val, float(qm.scale), float(qm.zero_point),
                    list(qm.mean_abs_x), list(qm.mean_x), list(qm.std)))
    return out


@pytest.mark.parametrize("async_observers", [False, True])
def test_calibrate_mixed_model(async_observers):
    plain = _model("MinMaxObserver")
    mixed = _model("PercentileObserver")
    qa = mixed[1].activation_quantizer
    qa.observer.percentile, qa.observer.bins = 99.0, 256
    seen = []
    mixed[1].register_forward_hook(lambda _m, _i, out: seen.append(out.detach().clone()))
    calibrate_qat_model(plain, _loader(), data_calib, DEV)
    calibrate_qat_model(mixed, _loader(), data_calib, DEV, async_observers=async_observers)
    for i in (0, 2):   # the MinMax layers still take the deferred one-pass path: the same bits
        assert _layer_state(mixed[i]) == _layer_state(plain[i])
    assert _layer_state(mixed[1])[0] == _layer_state(plain[1])[0]   # its weight manager too
    for layer in mixed:
        for qm in (layer.weight_quantizer, layer.activation_quantizer):
            assert not qm._pending_records and not qm.dist_defer and qm._side is None
    ref = OracleObserver(False)
    for y in seen:   # calibration output of the layer: relu(pre-activation), what was observed
        v = y.reshape(-1).cpu().numpy()
        lo, hi = oracle_clip(v, v.min(), v.max(), tail_of(99.0), 256)
        assert hi < v.max()
        ref.update(lo, hi, False)
    s, z = ref.qparams()
    assert (float(qa.scale), float(qa.zero_point)) == (s, z)
    assert (qa.observer.min_val, qa.observer.max_val) == (0, float(ref.mx))
    assert len(qa.mean_abs_x) == 3
    assert qa.observer.max_val < plain[1].activation_quantizer.observer.max_val


def test_dist_group_and_half_tensors_raise():
    x = torch.randn(4096, device=DEV)
    for is_quantize in (False, True):
        qm = _manager()
        qm.is_quantize = is_quantize
        qm.dist_group = object()
        with pytest.raises(NotImplementedError, match="PercentileObserver"):
            qm.quantize(x)
    qm = _manager()
    qm.is_quantize = False
    with pytest.raises(TypeError, match="bfloat16"):
        qm.collect_qparameter(x.bfloat16())
    with pytest.raises(TypeError, match="float16"):
        observe_percentile(x.half(), symmetric=True, tail=0.01, bins=256)
    assert _stats_words() == 0


# ------------------------------------------------------------------ 4. HIP-graph capture
def test_graph_replay_equals_eager():
    n = 40 * STEP + 4
    x1, x2 = make_input("relu", n, 8).to(DEV), make_input("outliers", n, 9).to(DEV)
    kw = dict(symmetric=False, tail=1e-3, bins=2048)
    s_ref = torch.zeros(2, dtype=torch.float32, device=DEV)
    want = [t.clone() for t in observe_percentile(x2, run_minmax=s_ref, **kw)]

    xs = x1.clone()
    state = torch.zeros(2, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        observe_percentile(xs, run_minmax=state, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = observe_percentile(xs, run_minmax=state, **kw)
    xs.copy_(x2)
    for _ in range(2):
        state.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert all(same_bits(g, w) for g, w in zip(got, want))
    assert same_bits(state, s_ref)
