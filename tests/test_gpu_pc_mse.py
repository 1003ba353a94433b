"""PerChannelMSEObserver on MI355X: the one-launch kernel (csrc/k_pc_mse.hip) against the host
loop and the per-row numpy oracle (tests/pc_mse_common.py) at the kernel's seams -- every E_k
within 1e-9 relative of the fsum oracle; pick, range, running state and qparams bit for bit,
the oracle's margin asserted for every searched row of every case -- mixed rows in one
workgroup, run-to-run determinism, the fake-quantized output and its backward, the manager's
and the fused layer's routing and HIP-graph capture."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests.pc_mse_common import (FAMILIES, ONGRID_RATIOS, OracleState, check_against_oracle, forms, grid_of, mse_ratios,
                                 pick_seed, same_bits, same_result)
from vsiquantization_amd.fakequant import (PerChannelFQFn, per_channel_fake_quant, per_channel_observe_fq,
                                           per_channel_observe_mse)
from vsiquantization_amd.modules.fused import ConvBnReLU
from vsiquantization_amd.observers import PerChannelMSEObserver

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = forms()
WAVE_LENS = (1, 3, 4, 9, 27, 255, 256, 257, F["wave_max"], F["wave_max"] + 1)
BLOCK_LENS = (F["block_max"], F["block_max"] + 1, F["block_max"] + 4, 2 * F["block_max"] + 36)
ROWS = (1, 3, F["rows_per_wg"] + 1, 65)
SEARCHED = ("gauss", "heavy", "relu")
MIXED = FAMILIES + FAMILIES[::-1]   # 16 adjacent rows: every family next to every kind of fallback
TABLES = {"default": mse_ratios(), "denormal": mse_ratios(64, 2.0 ** -24), "ongrid": ONGRID_RATIOS}


def _families(rows):
    return tuple(SEARCHED[c % len(SEARCHED)] for c in range(rows))


def _to_dev(xc, offset):
    if not offset:
        return xc.to(DEV)
    buf = torch.empty(xc.numel() + 1, dtype=torch.float32, device=DEV)   # a view one element into a buffer
    x = buf[1:].view(xc.shape)
    x.copy_(xc)
    assert x.data_ptr() % 16 != 0
    return x


def _check_sequence(families, rowlen, symmetric, bits, ratios, calls=1, offset=False, start=1):
    """Successive calls on one running state: device == host loop == oracle, a repeated call
    the same bits, y / mask the fixed-qparam kernel's for the qparams returned."""
    C = len(families)
    qmin, qmax = grid_of(bits, symmetric)
    state = OracleState(C, symmetric, bits)
    dmn, dmx = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    hmn, hmx = torch.zeros(C), torch.zeros(C)
    kw = dict(symmetric=symmetric, qmin=qmin, qmax=qmax, num_bits=bits, ratios=ratios, want_row_stats=True)
    seed = start
    for _ in range(calls):
        seed, xc, rows = pick_seed(families, rowlen, ratios, symmetric, bits, start=seed)   # on the CPU, oracle alone
        tag = (families[:4], C, rowlen, symmetric, bits, len(ratios), offset, seed)
        seed += 1
        x = _to_dev(xc, offset)
        before = (dmn.clone(), dmx.clone())
        r = per_channel_observe_mse(x, run_min=dmn, run_max=dmx, want_mask=True, **kw)
        again = per_channel_observe_mse(x, run_min=before[0], run_max=before[1], want_mask=True, **kw)
        only = per_channel_observe_mse(x, run_min=None, run_max=None, quantize=False, **kw)
        h = per_channel_observe_mse(xc, run_min=hmn, run_max=hmx, want_mask=True, **kw)
        state.update(rows)
        check_against_oracle(r, rows, state, tag)
        check_against_oracle(h, rows, state, tag)
        assert same_result(r, again) and same_bits(r["y"], again["y"]) and same_bits(r["mask"], again["mask"]), tag
        assert same_bits(r["row_stats"], again["row_stats"]), tag
        assert same_bits(only["err"], r["err"]) and same_bits(only["pick"], r["pick"]) and only["y"] is None, tag
        assert same_bits(only["clip"], r["clip"]), tag
        y, mask, _ = per_channel_fake_quant(x, r["scale"], r["zp"], qmin, qmax, want_mask=True)
        assert same_bits(r["y"], y) and same_bits(r["mask"], mask), tag
        assert same_bits(r["y"], h["y"]), tag
        # the row sums are K3's: the same fp32 sums over each group of 4, added in f64 in another
        # order -- two orders of n <= 6153 f64 additions differ by at most 2 n 2^-53 < 2e-12 of the
        # sum of magnitudes
        k3 = per_channel_observe_fq(x, symmetric=symmetric, qmin=qmin, qmax=qmax, quantize=False,
                                    want_row_stats=True)["row_stats"].cpu().numpy()
        rs = r["row_stats"].cpu().numpy()
        with np.errstate(all="ignore"):
            ok = np.abs(rs - k3) <= 2e-12 * np.abs(k3[:, [0, 0, 2]])
        assert np.all(ok | (np.isnan(rs) & np.isnan(k3)) | (rs == k3)), tag


# ------------------------------------------------------------------ 1. the seams
@pytest.mark.parametrize("rowlen", WAVE_LENS)
def test_wave_form_row_lengths(rowlen):
    _check_sequence(_families(F["rows_per_wg"] + 1), rowlen, True, 4, mse_ratios(), calls=2)
    _check_sequence(_families(3), rowlen, False, 2, mse_ratios())


@pytest.mark.parametrize("rowlen", BLOCK_LENS)
def test_workgroup_form_row_lengths(rowlen):
    _check_sequence(_families(3), rowlen, False, 4, mse_ratios())


@pytest.mark.parametrize("rows", ROWS)
def test_row_counts(rows):
    _check_sequence(_families(rows), 27, True, 4, mse_ratios(), calls=2)
    _check_sequence(_families(rows), F["wave_max"] + 4, False, 4, mse_ratios(16))


def test_ragged_rows_and_offset_views_take_the_scalar_path():
    for rowlen in (27, 257, F["wave_max"] + 3, F["block_max"] + 1):
        _check_sequence(_families(3), rowlen, True, 4, mse_ratios(16), offset=True)
    for rowlen in (256, F["wave_max"] + 4):   # rowlen % 4 == 0 but the base is not 16-byte aligned
        _check_sequence(_families(5), rowlen, False, 4, mse_ratios(16), offset=True)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_mixed_rows_in_one_tensor(table, symmetric):
    """gauss / heavy / relu / constant / nan / inf / denormal / ongrid in adjacent rows: each
    its own oracle and its own fallback, in the waves of one workgroup and in workgroups of
    their own."""
    for bits in (2, 4, 8):
        for rowlen in (27, 257, F["wave_max"] + 4):
            _check_sequence(MIXED, rowlen, symmetric, bits, TABLES[table], calls=2)


@pytest.mark.parametrize("count", [2, 64, 128])
def test_candidate_counts(count):
    for symmetric, bits in ((True, 4), (False, 8)):
        _check_sequence(_families(5), 257, symmetric, bits, mse_ratios(count))
        _check_sequence(_families(2), F["wave_max"] + 4, symmetric, bits, mse_ratios(count))


# ------------------------------------------------------------------ 2. quantize and backward
def _heavy_weight(shape=(32, 16, 3, 3)):
    g = torch.Generator().manual_seed(5)
    w = torch.randn(*shape, generator=g)
    w.view(shape[0], -1)[:, 0] = 8.0   # one outlier per out-channel
    return w


def test_observe_quantize_backward_is_the_fixed_qparam_ste():
    w = _heavy_weight().to(DEV)
    obs = PerChannelMSEObserver(True, 4)
    quantizer = V.PerChannelUniformQuantizer(4, True)
    a = w.clone().requires_grad_(True)
    y, rs = obs.observe_quantize(a, quantizer, want_row_stats=True)
    g = torch.randn_like(y)
    y.backward(g)
    s, z = obs.get_scale_zero_point()
    b = w.clone().requires_grad_(True)
    yb = PerChannelFQFn.apply(b, s, z, quantizer.qmin, quantizer.qmax)
    yb.backward(g)
    assert same_bits(y, yb) and same_bits(a.grad, b.grad)
    assert rs.shape == (32, 3) and bool((obs.last_pick > 0).all())


# ------------------------------------------------------------------ 3. manager and fused layer
def _qm(observer, bits=4, sym=True):
    qm = V.QuantizationManager("PerChannelUniformQuantizer", observer, bits, sym, False)
    qm.is_observer_qparam, qm.is_learning_scale = True, False
    return qm


def test_manager_routes_reach_the_kernel():
    w = _heavy_weight().to(DEV)
    for is_quantize in (False, True):
        qm, mm = _qm("PerChannelMSEObserver"), _qm("PerChannelMinMaxObserver")
        for q in (qm, mm):
            q.is_quantize = is_quantize
        if is_quantize:
            y = qm.quantize(w)             # the fused observe + quantize path
            mm.quantize(w)
            want, _, _ = per_channel_fake_quant(w, qm.scale, qm.zero_point, qm.quantizer.qmin, qm.quantizer.qmax)
            assert same_bits(y, want)
        else:
            qm.collect_qparameter(w)
            mm.collect_qparameter(w)
        obs = qm.observer
        assert obs.last_errors.shape == (32, 64) and bool((obs.last_pick > 0).all())
        assert bool((obs.max_val < mm.observer.max_val).all())
        assert "_op" not in obs.__dict__   # the parent's bound min / max op is never built
        for name in ("mean_abs_x", "mean_x", "std"):
            assert len(getattr(qm, name)) == 1 and getattr(qm, name) == getattr(mm, name)
        h = per_channel_observe_mse(w.cpu(), symmetric=True, qmin=-8, qmax=7, num_bits=4, ratios=obs.ratios,
                                    quantize=False)
        assert same_bits(obs.last_pick, h["pick"]) and same_bits(qm.scale, h["scale"])


def test_conv_bn_relu_weight_observer():
    torch.manual_seed(0)

    def layer(observer_w):
        torch.manual_seed(0)
        cv = nn.Conv2d(16, 32, 3, padding=1, bias=False)
        with torch.no_grad():
            cv.weight.copy_(_heavy_weight())
        bn = nn.BatchNorm2d(32)
        return ConvBnReLU(cv, bn, nn.ReLU(), observer_w, "PerChannelUniformQuantizer", "MinMaxObserver",
                          "UniformQuantizer", True, False, True, 4, 8).to(DEV)

    a, b = layer("PerChannelMSEObserver"), layer("PerChannelMinMaxObserver")
    x = torch.randn(2, 16, 8, 8, device=DEV)
    for m in (a, b):
        for q in (m.weight_quantizer, m.activation_quantizer):
            q.is_learning_scale = False   # calibration: the observers set the qparams
        m(x)
    oa, ob = a.weight_quantizer.observer, b.weight_quantizer.observer
    assert isinstance(oa, PerChannelMSEObserver) and oa.num_bits == 4
    assert oa.last_pick is not None and bool((oa.last_pick > 0).any())
    assert bool((oa.max_val <= ob.max_val).all()) and bool((oa.max_val < ob.max_val).any())


def test_half_tensors_raise():
    x = torch.randn(8, 27, device=DEV)
    qm = _qm("PerChannelMSEObserver")
    qm.is_quantize = False
    with pytest.raises(TypeError, match="bfloat16"):
        qm.collect_qparameter(x.bfloat16())
    with pytest.raises(TypeError, match="float16"):
        per_channel_observe_mse(x.half(), symmetric=True, qmin=-8, qmax=7, ratios=mse_ratios())
    with pytest.raises(TypeError, match="float16"):
        PerChannelMSEObserver(True, 4).observe_quantize(x.half(), V.PerChannelUniformQuantizer(4, True))


# ------------------------------------------------------------------ 4. HIP-graph capture
def test_graph_replay_equals_eager():
    _, x1, _ = pick_seed(_families(9), 576, mse_ratios(), False, 4, start=1)
    _, x2, _ = pick_seed(_families(9), 576, mse_ratios(), False, 4, start=20)
    x1, x2 = x1.to(DEV), x2.to(DEV)
    kw = dict(symmetric=False, qmin=0, qmax=15, num_bits=4, ratios=mse_ratios(), want_mask=True, want_row_stats=True)
    ref_mn, ref_mx = torch.zeros(9, device=DEV), torch.zeros(9, device=DEV)
    want = per_channel_observe_mse(x2, run_min=ref_mn, run_max=ref_mx, **kw)

    xs = x1.clone()
    state = torch.zeros(2, 9, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        per_channel_observe_mse(xs, run_min=state[0], run_max=state[1], **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = per_channel_observe_mse(xs, run_min=state[0], run_max=state[1], **kw)
    xs.copy_(x2)
    for _ in range(2):
        state.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert same_result(got, want) and same_bits(got["y"], want["y"]) and same_bits(got["mask"], want["mask"])
    assert same_bits(got["row_stats"], want["row_stats"])
    assert same_bits(state[0], ref_mn) and same_bits(state[1], ref_mx)
