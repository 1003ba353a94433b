"""MSEObserver on MI355X: the search pass (csrc/k_observe_mse.hip) against the host loop and the
numpy oracle (tests/mse_common.py) -- every E_k within 1e-9 relative of the fsum oracle; pick,
range, running state and qparams bit for bit wherever the oracle's margin decides the pick
(asserted for every case) -- run-to-run determinism, the workspace / counter discipline,
the manager's routing and HIP-graph capture."""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests.mse_common import (FAMILIES, OracleObserver, decidable, errors_close, grid_of, k2_minmax, make_input, margin,
                              oracle_search, ratios_of, same_bits)
from vsiquantization_amd import _hip as H
from vsiquantization_amd.fakequant import activation, fake_quant, mse_ratios, observe_mse, qden
from vsiquantization_amd.modules.fused import ConvBnReLU
from vsiquantization_amd.utils.quantize_manager import calibrate_qat_model, data_calib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vsiquantization_amd", "csrc")


def _single():
    """The largest one-workgroup tensor, read from the source (kObsSingle groups of 4)."""
    common = open(os.path.join(CSRC, "vsiq_common.cuh")).read()
    k2 = open(os.path.join(CSRC, "k_observe_k2.cuh")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", common).group(1))
    u = int(re.search(r"constexpr int kObsU = (\d+);", common).group(1))
    assert "constexpr int64_t kObsSingle = (int64_t)kBlock * kObsU;" in k2
    return 4 * block * u


SINGLE = _single()
# 1, 3, 4; around one wave-step; an odd size whose scalar tail runs; the last one-workgroup
# size and the first of two workgroups
SMALL_N = (1, 3, 4, 1023, 1024, 1025, 4099, SINGLE, SINGLE + 4)
MID_N = 70001               # 9 workgroups, flat arrival
BIG_N = (1 << 21) + 3       # the full grid of 512 workgroups, two-level arrival


def _counter_words(dev=DEV):
    return int(H.workspace(torch.device(dev)).counter.ne(0).sum())


@functools.lru_cache(maxsize=None)
def _case(family, n, seed, act):
    """(CPU input, act(input) as the device computes it, on the CPU): made once per case."""
    xc = make_input(family, n, seed)
    va = activation(xc.to(DEV), act).cpu().contiguous() if act else xc
    return xc, va


@functools.lru_cache(maxsize=None)
def _oracle(family, n, seed, act, mn, mx, has_nan, ratios, symmetric, bits):
    return oracle_search(_case(family, n, seed, act)[1].numpy(), np.float32(mn), np.float32(mx), has_nan, ratios,
                         symmetric, bits)


def _host_search(va, st, ratios, symmetric, bits, state):
    """The host loop on the device call's K2 record."""
    st = st.cpu().contiguous()
    qp = torch.empty(H.QP_LEN, dtype=torch.float64)
    clip = torch.empty(2, dtype=torch.float64)
    err = torch.empty(len(ratios), dtype=torch.float64)
    pick = torch.empty(1, dtype=torch.int32)
    qmin, qmax = grid_of(bits, symmetric)
    rc = H.lib().vsiq_host_observe_mse_f32(H.ptr(va), H.c_i64(va.numel()), 0, H.ptr(st),
                                           (H.c_d * len(ratios))(*ratios), len(ratios), qmin, qmax, H.ptr(state),
                                           H.ptr(qp), H.ptr(clip), H.ptr(err), H.ptr(pick), int(symmetric),
                                           qden(symmetric, bits, 1e-8), 1e-8)
    assert rc == 0
    return qp, clip, err, pick


def _check_sequence(cases, symmetric, bits, ratios=None, act=None, offset=False):
    """Successive calls (family, n, seed) on one running state: device == host loop == oracle."""
    dstate = torch.zeros(2, dtype=torch.float32, device=DEV)
    hstate = torch.zeros(2, dtype=torch.float32)
    ref = OracleObserver(symmetric, bits)
    qmin, qmax = grid_of(bits, symmetric)
    for family, n, seed in cases:
        r = ratios or ratios_of(family)
        xc, va = _case(family, n, seed, act)
        if offset:   # a view one element into a buffer: not 16-byte aligned, the scalar path
            x = torch.empty(n + 1, dtype=torch.float32, device=DEV)[1:]
            x.copy_(xc)
            assert x.data_ptr() % 16 != 0
        else:
            x = xc.to(DEV)
        kw = dict(symmetric=symmetric, num_bits=bits, ratios=r, qmin=qmin, qmax=qmax, act=act)
        qp, st, clip, err, pick = observe_mse(x, run_minmax=dstate, **kw)
        again = observe_mse(x, run_minmax=None, **kw)   # a repeat: the same bits run to run
        mn, mx, has_nan = k2_minmax(st)
        lo, hi, E, k = _oracle(family, n, seed, act, float(mn), float(mx), has_nan, tuple(r), symmetric, bits)
        ref.update(lo, hi, has_nan)
        hqp, hclip, herr, hpick = _host_search(va, st, r, symmetric, bits, hstate)
        tag = (family, n, seed, symmetric, bits, len(r), act, offset, margin(E))
        print("mse case", tag, "pick", int(pick), k, "E", float(err[int(pick)]), E[k])
        assert decidable(E), tag                                # the precondition, on the oracle alone
        assert errors_close(err, E) and errors_close(herr, E), tag
        assert same_bits(err, again[3]) and same_bits(pick, again[4]) and same_bits(clip, again[2]), tag
        assert int(pick) == k == int(hpick), tag
        assert same_bits(clip, np.array([lo, hi], dtype=np.float64)), tag
        assert same_bits(clip, hclip) and same_bits(qp, hqp) and same_bits(dstate, hstate), tag
        assert same_bits(dstate, np.array([ref.mn, ref.mx], dtype=np.float32)), tag
        assert same_bits(qp, ref.qp_record()), tag
        assert _counter_words() == 0, tag


# ------------------------------------------------------------------ 1. device == host == oracle
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_device_equals_host_and_oracle(family, symmetric):
    cases = [(family, n, 1) for n in SMALL_N]
    for bits in (2, 4, 8):
        _check_sequence(cases, symmetric, bits)


@pytest.mark.parametrize("family", ["gauss", "heavy", "relu", "denormal", "ongrid"])
def test_several_workgroups(family):
    cases = [(family, MID_N, 2), (family, MID_N, 3)]
    for symmetric, bits in ((True, 4), (False, 2), (False, 8)):
        _check_sequence(cases, symmetric, bits)


def test_full_grid():
    _check_sequence([("gauss", BIG_N, 2)], True, 4, ratios=mse_ratios(16))


@pytest.mark.parametrize("count", [2, 64, 128])
def test_candidate_counts(count):
    for symmetric, bits in ((True, 4), (False, 4)):
        _check_sequence([("gauss", SINGLE + 4, 4), ("heavy", MID_N, 4)], symmetric, bits, ratios=mse_ratios(count))


def test_offset_views_take_the_scalar_path():
    cases = [("heavy", n, 4) for n in (4, 1025, SINGLE, SINGLE + 4, MID_N)]
    for symmetric, bits in ((False, 4), (True, 2)):
        _check_sequence(cases, symmetric, bits, offset=True)


@pytest.mark.parametrize("act", ["relu", "silu"])
def test_fused_activations(act):
    cases = [("heavy", n, 5) for n in (3, 1025, 4099, SINGLE + 4, MID_N)]
    for symmetric, bits, offset in ((False, 4, False), (True, 4, False), (False, 2, True)):
        _check_sequence(cases, symmetric, bits, act=act, offset=offset)


# ------------------------------------------------------------------ 2. buffer discipline
def test_back_to_back_calls_equal_each_alone():
    a = make_input("relu", MID_N, 6).to(DEV)
    b = make_input("heavy", 300_000, 7).to(DEV)
    c = make_input("gauss", SINGLE, 7).to(DEV)
    kw = dict(symmetric=False, num_bits=4, ratios=mse_ratios(), qmin=0, qmax=15)

    def alone(x):
        s = torch.zeros(2, dtype=torch.float32, device=DEV)
        r = observe_mse(x, run_minmax=s, **kw)
        torch.cuda.synchronize()
        return [t.clone() for t in r] + [s]

    want = [alone(x) for x in (a, b, c)]
    states = [torch.zeros(2, dtype=torch.float32, device=DEV) for _ in range(3)]
    got = [observe_mse(x, run_minmax=s, **kw) for x, s in zip((a, b, c), states)]   # no sync in between
    last = observe_mse(a, run_minmax=None, **kw)
    torch.cuda.synchronize()
    for g, s, w in zip(got, states, want):
        assert all(same_bits(p, q) for p, q in zip(list(g) + [s], w))
    assert all(same_bits(p, q) for p, q in zip(last, want[0][:5]))
    assert _counter_words() == 0


# ------------------------------------------------------------------ 3. manager
def _manager(observer="MSEObserver", sym=False, bits=4):
    qm = V.QuantizationManager("UniformQuantizer", observer, bits, sym, False)
    qm.is_observer_qparam, qm.is_learning_scale = True, False
    return qm


@pytest.mark.parametrize("n", [4096, 300_000])
def test_per_call_observe_and_quantize(n):
    qm = _manager(bits=4)
    ref = OracleObserver(False, 4)
    for seed in (1, 2):
        xc = make_input("heavy", n, seed)
        x = xc.to(DEV)
        y = qm.quantize(x)
        lo, hi, E, k = oracle_search(xc.numpy(), xc.min().item(), xc.max().item(), False, qm.observer.ratios, False, 4)
        assert decidable(E) and k > 0
        ref.update(lo, hi, False)
        s, z = ref.qparams()
        assert float(qm.scale) == s and float(qm.zero_point) == z
        assert int(qm.observer.last_pick) == k and errors_close(qm.observer.last_errors, E)
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
    mixed = _model("MSEObserver")
    qa = mixed[1].activation_quantizer
    assert qa.observer.num_bits == 4
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
    ref = OracleObserver(False, 4)
    for y in seen:   # calibration output of the layer: relu(pre-activation), what was observed
        v = y.reshape(-1).cpu().numpy()
        lo, hi, E, k = oracle_search(v, v.min(), v.max(), False, qa.observer.ratios, False, 4)
        assert decidable(E) and hi < v.max()
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
        with pytest.raises(NotImplementedError, match="MSEObserver"):
            qm.quantize(x)
    qm = _manager()
    qm.is_quantize = False
    with pytest.raises(TypeError, match="bfloat16"):
        qm.collect_qparameter(x.bfloat16())
    with pytest.raises(TypeError, match="float16"):
        observe_mse(x.half(), symmetric=True, ratios=mse_ratios(), qmin=-8, qmax=7)
    assert _counter_words() == 0


# ------------------------------------------------------------------ 4. HIP-graph capture
def test_graph_replay_equals_eager():
    n = 300_004
    x1, x2 = make_input("relu", n, 8).to(DEV), make_input("heavy", n, 9).to(DEV)
    kw = dict(symmetric=False, num_bits=4, ratios=mse_ratios(), qmin=0, qmax=15)
    s_ref = torch.zeros(2, dtype=torch.float32, device=DEV)
    want = [t.clone() for t in observe_mse(x2, run_minmax=s_ref, **kw)]

    xs = x1.clone()
    state = torch.zeros(2, dtype=torch.float32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        observe_mse(xs, run_minmax=state, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = observe_mse(xs, run_minmax=state, **kw)
    xs.copy_(x2)
    for _ in range(2):
        state.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert all(same_bits(g, w) for g, w in zip(got, want))
    assert same_bits(state, s_ref)
