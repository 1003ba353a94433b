"""MSEObserver without a GPU: registry and ABI, header against binding, argument checks of
both entry points, the native host loop against the numpy oracle (tests/mse_common.py),
the invariants of the definition, the manager's bits rule and the fused-layer calibration
flow on CPU tensors."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests.mse_common import (FAMILIES, OracleObserver, decidable, errors_close, grid_of, k2_minmax, make_input,
                              margin, oracle_search, ratios_of, same_bits)
from vsiquantization_amd import _hip as H
from vsiquantization_amd.fakequant import mse_ratios, observe_mse, observe_tensor
from vsiquantization_amd.modules.fused import ConvBnReLU
from vsiquantization_amd.observers import MinMaxObserver, MSEObserver, PercentileObserver
from vsiquantization_amd.utils.quantize_manager import calibrate_qat_model
from vsiquantization_amd.utils.registry import CLASS_REGISTRY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vsiq.h")
ENTRIES = ("vsiq_act_observe_mse_f32", "vsiq_observe_mse_ws_doubles", "vsiq_host_observe_mse_f32")
SIZES = (1, 3, 4, 1025, 4099)
BITS = (2, 4, 8)


# ------------------------------------------------------------------ 1. registry, construction
def test_registry_and_construction():
    obs = CLASS_REGISTRY["MSEObserver"](True)
    assert isinstance(obs, MSEObserver) and isinstance(obs, MinMaxObserver) and V.MSEObserver is MSEObserver
    assert (obs.symmetric, obs.num_bits, obs.eps, obs.candidates, obs.min_ratio) == (True, 8, 1e-8, 64, 2 ** -8)
    assert not obs.single_pass and obs.follows_bits_width and not getattr(MinMaxObserver, "follows_bits_width", False)
    assert obs.ratios == tuple((2 ** -8) ** (k / 63) for k in range(64))
    assert obs.ratios[0] == 1.0 and obs.ratios[-1] == 2 ** -8 and obs.last_errors is None and obs.last_pick is None
    assert repr(obs) == "MSEObserver(symmetric=True, num_bits=8, eps=1e-08, candidates=64, min_ratio=0.00390625)"
    assert MSEObserver(candidates=1).ratios == (1.0,)
    explicit = MSEObserver(ratios=[1.0, 0.5, 0.75])
    assert explicit.ratios == (1.0, 0.5, 0.75) and explicit.candidates == 3
    assert (MSEObserver(True, 4).grid(), MSEObserver(False, 4).grid()) == ((-8, 7), (0, 15))
    qm = V.QuantizationManager("UniformQuantizer", "MSEObserver", 8, False)
    assert isinstance(qm.observer, MSEObserver) and qm.observer.symmetric is False


def test_symbols_bound_and_abi_unchanged():
    lib = H.lib()
    for name in ENTRIES:
        assert name in H.EXPORTED and hasattr(lib, name)
    assert H.ABI_VERSION == 13 and lib.vsiq_abi_version() == 13
    assert lib.vsiq_observe_mse_ws_doubles(H.c_i64(8192), 64) == 0            # one workgroup: no records
    assert lib.vsiq_observe_mse_ws_doubles(H.c_i64(8196), 64) == 2 * 64       # one f64[count] record each
    assert lib.vsiq_observe_mse_ws_doubles(H.c_i64(1 << 30), 128) == 512 * 128


def test_header_and_binding_declare_the_same_signatures():
    ctype = {"int": H.c_int, "int64_t": H.c_i64, "double": H.c_d}
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    found = {}
    for ret, name, args in re.findall(r"\b(int|int64_t)\s+(vsiq_\w+)\s*\(([^)]*)\)\s*;", text):
        if name in ENTRIES:
            types = []
            for a in args.split(","):
                a = " ".join(a.split())
                types.append(H.c_p if "*" in a else ctype[a.replace("const ", "").rsplit(" ", 1)[0]])
            found[name] = (types, ctype[ret])
    assert sorted(found) == sorted(ENTRIES)
    for name, (types, ret) in found.items():
        assert H._SIGS[name][0] == types and H._SIGS[name][1] is ret, name


# ------------------------------------------------------------------ 2. argument checks
def _buf(n, dtype):
    t = torch.zeros(n, dtype=dtype)
    return t, H.ptr(t)


def _table(vals):
    return (H.c_d * len(vals))(*vals)


def test_argument_checks_without_a_launch():
    lib = H.lib()
    x, px = _buf(8, torch.float32)
    st, pst = _buf(H.ST_LEN, torch.float64)
    ws, pws = _buf(1024, torch.float64)
    cnt, pc = _buf(H.COUNTER_WORDS, torch.int32)
    run, pr = _buf(2, torch.float32)
    qp, pq = _buf(H.QP_LEN, torch.float64)
    clip, pcl = _buf(2, torch.float64)
    err, pe = _buf(128, torch.float64)
    pick, pp = _buf(1, torch.int32)
    good = _table([1.0, 0.5])
    n8 = H.c_i64(8)

    def dev(c=px, n=n8, act=0, stats=pst, ratios=good, count=2, qmin=-8, qmax=7, w=pws, wlen=H.c_i64(1024),
            counter=pc, cl=pcl, e=pe, p=pp):
        return lib.vsiq_act_observe_mse_f32(c, n, act, stats, ratios, count, qmin, qmax, w, wlen, counter, pr, pq, cl,
                                            e, p, 1, 7.0, 1e-8, None)

    def hst(c=px, n=n8, act=0, stats=pst, ratios=good, count=2, qmin=-8, qmax=7, cl=pcl, e=pe, p=pp):
        return lib.vsiq_host_observe_mse_f32(c, n, act, stats, ratios, count, qmin, qmax, pr, pq, cl, e, p, 1, 7.0,
                                             1e-8)

    E_ARG, E_WS = -1, -3
    for f in (dev, hst):
        for null in ("c", "stats", "ratios", "cl", "e", "p"):
            assert f(**{null: None}) == E_ARG, null
        assert f(n=H.c_i64(0)) == E_ARG and f(n=H.c_i64(-4)) == E_ARG
        assert f(act=3) == E_ARG and f(act=-1) == E_ARG
        for count in (0, -1, 129, 1 << 20):
            assert f(ratios=_table([1.0] * 130), count=count) == E_ARG, count
        for bad in ([0.5, 1.0], [1.0, 0.0], [1.0, -0.5], [1.0, 1.5], [1.0, float("nan")], [float("nan"), 0.5],
                    [1.0, float("inf")]):
            assert f(ratios=_table(bad)) == E_ARG, bad
        assert f(qmin=7, qmax=7) == E_ARG and f(qmin=8, qmax=7) == E_ARG
    assert dev(w=None) == E_ARG and dev(counter=None) == E_ARG
    big = H.c_i64(8196)   # two workgroups: 2 * count doubles
    assert lib.vsiq_act_observe_mse_f32(px, big, 0, pst, good, 2, -8, 7, pws, H.c_i64(3), pc, pr, pq, pcl, pe, pp, 1,
                                        7.0, 1e-8, None) == E_WS
    assert not cnt.any() and not ws.any() and not err.any()


def test_ratios_are_validated():
    x = torch.randn(100)
    for bad in ([0.5, 1.0], [1.0, 0.0], [1.0, 1.0001], [1.0, float("nan")], [], [1.0] * 129):
        with pytest.raises(ValueError):
            MSEObserver(ratios=bad)
        with pytest.raises(ValueError):
            observe_mse(x, symmetric=True, ratios=bad, qmin=-8, qmax=7)
    for kw in (dict(candidates=0), dict(candidates=129), dict(min_ratio=0.0), dict(min_ratio=1.5),
               dict(min_ratio=float("nan"))):
        with pytest.raises(ValueError):
            MSEObserver(**kw)
    with pytest.raises(ValueError):
        observe_mse(x, symmetric=True, ratios=[1.0, 0.5], qmin=3, qmax=3)


# ------------------------------------------------------------------ 3. host loop == oracle
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_host_loop_equals_oracle(family, symmetric):
    ratios = ratios_of(family)
    for bits in BITS:
        qmin, qmax = grid_of(bits, symmetric)
        for n in SIZES:
            state = torch.zeros(2, dtype=torch.float32)
            ref = OracleObserver(symmetric, bits)
            for seed in (1, 2):
                x = make_input(family, n, seed)
                qp, st, clip, err, pick = observe_mse(x, symmetric=symmetric, num_bits=bits, run_minmax=state,
                                                      ratios=ratios, qmin=qmin, qmax=qmax)
                mn, mx, has_nan = k2_minmax(st)
                lo, hi, E, k = oracle_search(x.numpy(), mn, mx, has_nan, ratios, symmetric, bits)
                ref.update(lo, hi, has_nan)
                tag = (family, symmetric, bits, n, seed, margin(E))
                assert decidable(E), tag
                assert errors_close(err, E), tag
                assert int(pick) == k, tag
                assert same_bits(clip, np.array([lo, hi], dtype=np.float64)), tag
                assert same_bits(state, np.array([ref.mn, ref.mx], dtype=np.float32)), tag
                assert same_bits(qp, ref.qp_record()), tag
                _, st2 = observe_tensor(x, symmetric=symmetric, num_bits=bits, want_qp=False)
                assert same_bits(st, st2), tag   # the stats record is the whole tensor's: K2's own


def test_families_exercise_what_they_are_for():
    """ongrid: zero errors and exact ties, decided for the smaller k; denormal: candidates go
    invalid as the scale underflows; constant / nan / inf: MinMaxObserver's call."""
    x = make_input("ongrid", 4099, 1)
    *_, err, pick = observe_mse(x, symmetric=False, num_bits=8, ratios=ratios_of("ongrid"), qmin=0, qmax=255)
    e = err.tolist()
    assert e[0] == e[1] == e[2] == 0.0 and min(e[3:]) > 0.0 and int(pick) == 0
    *_, err, pick = observe_mse(x, symmetric=True, num_bits=4, ratios=ratios_of("ongrid"), qmin=-8, qmax=7)
    e = err.tolist()
    assert e[0] == e[1] == e[2] > 0.0
    x = make_input("denormal", 4099, 1)
    *_, err, pick = observe_mse(x, symmetric=True, num_bits=8, ratios=ratios_of("denormal"), qmin=-128, qmax=127)
    e = err.tolist()
    assert math.isfinite(e[0]) and math.isinf(e[-1]) and math.isfinite(e[int(pick)])
    for family in ("constant", "nan", "inf"):
        x = make_input(family, 4099, 1)
        _, _, clip, err, pick = observe_mse(x, symmetric=True, num_bits=4, ratios=mse_ratios(), qmin=-8, qmax=7)
        v = x[~torch.isnan(x)]
        assert all(math.isinf(v) for v in err.tolist()) and int(pick) == 0
        assert clip.tolist() == [v.min().item(), v.max().item()]


def test_host_relu_is_the_loop_on_the_activated_tensor():
    x = make_input("heavy", 4099, 5)
    a, b = torch.zeros(2), torch.zeros(2)
    kw = dict(symmetric=False, num_bits=4, ratios=mse_ratios(), qmin=0, qmax=15)
    ra = observe_mse(x, run_minmax=a, act="relu", **kw)
    rb = observe_mse(torch.relu(x), run_minmax=b, **kw)
    assert same_bits(a, b) and all(same_bits(p, q) for p, q in zip(ra, rb))


# ------------------------------------------------------------------ 4. invariants
@pytest.mark.parametrize("symmetric", [True, False])
def test_one_candidate_is_minmax(symmetric):
    p = V.QuantizationManager("UniformQuantizer", "MSEObserver", 8, symmetric, False)
    m = V.QuantizationManager("UniformQuantizer", "MinMaxObserver", 8, symmetric, False)
    p.observer.ratios = mse_ratios(1)
    for qm in (p, m):
        qm.is_quantize = False
    for family in FAMILIES:
        for n in (5, 1025, 65537):
            x = make_input(family, n, 4)
            for qm in (p, m):
                qm.collect_qparameter(x)
            assert (p.scale, p.zero_point) == (m.scale, m.zero_point)
            assert same_bits(p.observer._state, m.observer._state)
            assert int(p.observer.last_pick) == 0 and all(math.isinf(v) for v in p.observer.last_errors.tolist())
    assert (p.observer.min_val, p.observer.max_val) == (m.observer.min_val, m.observer.max_val)
    for name in ("mean_abs_x", "mean_x", "std"):
        assert same_bits(np.array(getattr(p, name)), np.array(getattr(m, name)))


def test_gauss_at_4_bits_shrinks_the_range():
    x = make_input("gauss", 70001, 1)
    qm = V.QuantizationManager("UniformQuantizer", "MSEObserver", 4, True, False)
    qm.is_quantize = False
    qm.collect_qparameter(x)
    e, k = qm.observer.last_errors.tolist(), int(qm.observer.last_pick)
    assert k > 0 and e[k] < e[0] and e[k] == min(e)
    assert 0.2 * e[0] < e[k] < 0.5 * e[0]        # the search is worth about 3x at 4 bits on a Gaussian
    mm = MinMaxObserver(True, 4)                   # MinMaxObserver on the same grid
    mm.observe(x)
    assert 0 < qm.scale < mm.get_scale_zero_point()[0]
    assert qm.scale == (max(abs(qm.observer.min_val), abs(qm.observer.max_val)) / (7 + 1e-8))


def test_manager_sets_num_bits_for_mse_only():
    for bits in (2, 4, 8):
        qm = V.QuantizationManager("UniformQuantizer", "MSEObserver", bits, True, False)
        assert qm.observer.num_bits == bits and qm.observer.grid() == (qm.quantizer.qmin, qm.quantizer.qmax)
        qa = V.QuantizationManager("UniformQuantizer", "MSEObserver", bits, False, False)
        assert qa.observer.num_bits == bits and qa.observer.grid() == (qa.quantizer.qmin, qa.quantizer.qmax)
        for name in ("MinMaxObserver", "LSQObserver", "PercentileObserver", "PerChannelMinMaxObserver"):
            other = V.QuantizationManager("UniformQuantizer", name, bits, True, False)
            assert other.observer.num_bits == 8, name   # the reference's 8-bit observer (qm.py:42)
    assert PercentileObserver().num_bits == 8 and MSEObserver().num_bits == 8


# ------------------------------------------------------------------ 5. fused-layer flow
def test_fused_layer_calibration_on_cpu_tensors():
    torch.manual_seed(0)
    cv = nn.Conv2d(3, 8, 3, padding=1, bias=False)
    bn = nn.BatchNorm2d(8)
    bn.running_var.uniform_(0.5, 2.0)
    layer = ConvBnReLU(cv, bn, nn.ReLU(), "MinMaxObserver", "UniformQuantizer", "MSEObserver", "UniformQuantizer",
                       True, False, True, 8, 4)
    qa = layer.activation_quantizer
    assert qa.observer.num_bits == 4 and qa.observer.grid() == (0, 15)
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
    ref = OracleObserver(False, 4)
    for y in captured:   # the layer's output in calibration is relu(pre-activation), unquantized
        v = y.reshape(-1).numpy()
        lo, hi, E, k = oracle_search(v, v.min(), v.max(), False, qa.observer.ratios, False, 4)
        assert decidable(E) and k > 0 and hi < v.max()
        ref.update(lo, hi, False)
    s, z = ref.qparams()
    assert (qa.scale, qa.zero_point) == (s, int(z))
    assert (qa.observer.min_val, qa.observer.max_val) == (0, float(ref.mx))
