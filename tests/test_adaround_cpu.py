"""AdaRound on the host: the C ABI's host loops (vsiq_host_adaround_*) against the numpy
restatement of tests/adaround_common.py, the pinned edge inputs, the autograd Function
against a float64 eager composition, AdaRoundWeight's initialisation, the export round
trip and the layer driver.  No GPU."""
import numpy as np
import pytest
import torch

import vsiquantization_amd as V
from tests import adaround_common as A
from vsiquantization_amd import _hip as H
from vsiquantization_amd.fakequant import AdaRoundFn, adaround_backward, adaround_forward, unpack_dequant

F32 = np.float32
NAMES = ("vsiq_adaround_workspace_doubles", "vsiq_adaround_fwd_f32", "vsiq_adaround_bwd_f32",
         "vsiq_host_adaround_fwd_f32", "vsiq_host_adaround_bwd_f32")


def test_entries_and_abi():
    lib = H.lib()
    for name in NAMES:
        assert name in H.EXPORTED and hasattr(lib, name)
    assert lib.vsiq_abi_version() == 13   # additive


def _host_mask(w, V_, sc, zp, lo, hi, per_row):
    """m of the host forward (its optional mask output)."""
    rows, rowlen = w.shape
    wt, vt = torch.from_numpy(w), torch.from_numpy(V_)
    y = torch.empty_like(wt)
    mask = torch.empty(w.shape, dtype=torch.uint8)
    s = torch.from_numpy(sc)
    z = None if zp is None else torch.from_numpy(zp)
    rc = H.lib().vsiq_host_adaround_fwd_f32(H.ptr(wt), H.ptr(vt), H.ptr(y), H.ptr(mask), H.c_i64(rows),
                                            H.c_i64(rowlen), H.ptr(s), H.ptr(z), H.c_i64(rows if per_row else 1), 0,
                                            lo, hi, 0, 1.0, None)
    assert rc == 0
    return y.numpy(), mask.numpy().astype(bool)


@pytest.mark.parametrize("tag,rows,rowlen,per_row", A.all_cases())
def test_host_against_oracle(tag, rows, rowlen, per_row):
    """y soft and hard and m bit for bit given h; grad_V with lambda = 0 bit for bit."""
    for k, (bits, sym) in enumerate(A.GRIDS):
        w, Vv, g, sc, zp, lo, hi = A.make_case(rows, rowlen, bits, sym, per_row, seed=17 * k + rowlen)
        h, hp = A.lib_h(Vv), A.lib_hp(Vv)
        yo, mo, _ = A.oracle_forward(w, Vv, sc, zp, lo, hi, h=h)
        y, _ = A.run(w, Vv, sc, zp, lo, hi, per_row)
        assert A.bits_equal(y, yo), (tag, bits, sym)
        ym, m = _host_mask(w, Vv, sc, zp, lo, hi, per_row)
        assert A.bits_equal(ym, yo) and np.array_equal(m, mo), (tag, bits, sym)
        yh, _ = A.run(w, Vv, sc, zp, lo, hi, per_row, hard=True)
        assert A.bits_equal(yh, A.oracle_forward(w, Vv, sc, zp, lo, hi, hard=True)[0]), (tag, bits, sym)
        gv = A.run_bwd(g, w, Vv, sc, zp, lo, hi, per_row, lam=0.0, beta=2.0)
        assert A.bits_equal(gv, A.oracle_grad(g, w, Vv, sc, zp, lo, hi, 0.0, 2.0, h=h, hp=hp)), (tag, bits, sym)


def test_h_against_f64_closed_form():
    """|h - h64| <= 1e-6 (and h' likewise): sleef_expf_u10 is a 1-ulp exponential, the
    division, the fma and the clamp add a few ulps of 1.0, the fp32 constants 1.2f / 0.1f
    are within 5e-8 of 1.2 / 0.1; 1e-6 is about 8 ulps of 1.0 -- derived, not measured.  A
    wrong zeta, gamma or sign misses by 1e-2 or more."""
    v = np.concatenate([np.linspace(-40, 40, 200001), [0.0, -0.0, 30.0, -30.0, 2.3978953, -2.3978953]]).astype(F32)
    h, hp = A.lib_h(v), A.lib_hp(v)
    h6, hp6 = A.h64(v)
    eh, ep = np.abs(h - h6).max(), np.abs(hp - hp6).max()
    print("max |h - h64|", eh, "max |h' - h'64|", ep)
    # h' is discontinuous where hr crosses 0 / 1: fp32 and f64 may sit on different sides
    # within 1e-6 of the crossing, so compare away from it
    away = (np.abs(h6) > 1e-5) & (np.abs(1 - h6) > 1e-5) | (h6 == 0) & (h == 0) | (h6 == 1) & (h == 1)
    assert eh <= 1e-6
    assert np.abs(hp - hp6)[away].max() <= 1e-6
    assert ((h >= 0) & (h <= 1)).all()


@pytest.mark.parametrize("beta", A.BETAS)
def test_regulariser_host(beta):
    """grad_V with lambda != 0 within 1 fp32 ulp of the oracle, R within 1e-9 relative."""
    for rows, rowlen, per_row in ((1, 1023, False), (64, 27, True), (3, 1030, True), (130, 5, True)):
        w, Vv, g, sc, zp, lo, hi = A.make_case(rows, rowlen, 4, False, per_row, seed=rowlen)
        h = A.lib_h(Vv)
        _, R = A.run(w, Vv, sc, zp, lo, hi, per_row, beta=beta)
        Ro = A.oracle_reg(h, beta)
        print(rows, rowlen, beta, "R", float(R), Ro)
        assert abs(float(R) - Ro) <= 1e-9 * abs(Ro)
        _, R2 = A.run(w, Vv, sc, zp, lo, hi, per_row, beta=beta, want_y=False)
        assert float(R2) == float(R)
        gv = A.run_bwd(g, w, Vv, sc, zp, lo, hi, per_row, lam=0.01, beta=beta).numpy()
        go = A.oracle_grad(g, w, Vv, sc, zp, lo, hi, 0.01, beta, h=h)
        d = A.ulp_distance(gv, go).max()
        print("max ulp", d)
        assert d <= 1


def edge_case():
    """Pinned edge inputs on the 4-bit grid [-8, 7], s = 0.25, z = 0 (w/s exact)."""
    s = 0.25
    nan, inf = float("nan"), float("inf")
    #        w            V      what
    rows = [(0.30, 0.0),          # V = 0: hard up, soft h = 0.5
            (0.30, 30.0),         # h == 1, grad 0
            (0.30, -30.0),        # h == 0, grad 0
            (0.30, nan),          # NaN V: h = 0 (soft and hard), grad 0
            (7 * s, 0.5),         # w/s exact integer at hi: b = 7, r = 7 + h > hi -> outside
            (6.5 * s, 30.0),      # b = 6, h = 1: r = 7 == hi, just inside
            (7.2 * s, 0.5),       # b = 7, h > 0: r just outside hi
            (-8 * s, -30.0),      # b = -8, h = 0: r == lo, just inside
            (-8.5 * s, 0.5),      # b = -9, h < 1: r < lo, outside
            (-8.5 * s, 30.0),     # b = -9, h = 1: r == lo, inside
            (2 * s, 1.0),         # w/s an exact integer
            (inf, 0.5), (-inf, 0.5), (nan, 0.5)]
    w = np.array([[r[0] for r in rows]], F32)
    v = np.array([[r[1] for r in rows]], F32)
    return w, v, np.ones_like(w), np.array([s]), None, -8, 7


def check_edges(device):
    w, v, g, sc, zp, lo, hi = edge_case()
    s = F32(0.25)
    y = A.run(w, v, sc, zp, lo, hi, False, device)[0].cpu().numpy()[0]
    yh = A.run(w, v, sc, zp, lo, hi, False, device, hard=True)[0].cpu().numpy()[0]
    gv = A.run_bwd(g, w, v, sc, zp, lo, hi, False, device, lam=0.0, beta=2.0).cpu().numpy()[0]
    gl = A.run_bwd(g, w, v, sc, zp, lo, hi, False, device, lam=0.01, beta=2.0).cpu().numpy()[0]
    hp05 = A.lib_hp(np.array([0.5], F32))[0]
    h05 = A.lib_h(np.array([0.5], F32))[0]
    assert y[0] == F32(1.5) * s and yh[0] == 2 * s and gv[0] == F32(np.float64(s) * A.lib_hp(np.zeros(1, F32))[0])
    assert y[1] == 2 * s and yh[1] == 2 * s and gv[1] == 0 and gl[1] == 0
    assert y[2] == 1 * s and yh[2] == 1 * s and gv[2] == 0 and gl[2] == 0
    assert y[3] == 1 * s and yh[3] == 1 * s and gv[3] == 0 and gl[3] == 0
    assert y[4] == 7 * s and gv[4] == 0 and gl[4] != 0            # outside: clamped, no output gradient (the regulariser still acts)
    assert y[5] == 7 * s and yh[5] == 7 * s
    assert y[6] == 7 * s and gv[6] == 0
    assert y[7] == -8 * s and yh[7] == -8 * s
    assert y[8] == -8 * s and gv[8] == 0 and gl[8] != 0
    assert y[9] == -8 * s and yh[9] == -8 * s
    assert y[10] == (F32(2) + A.lib_h(np.ones(1, F32))[0]) * s and yh[10] == 3 * s and gv[10] > 0
    assert y[11] == 7 * s and yh[11] == 7 * s and gv[11] == 0
    assert y[12] == -8 * s and yh[12] == -8 * s and gv[12] == 0
    assert np.isnan(y[13]) and np.isnan(yh[13]) and gv[13] == 0
    # inside with V = 0.5: the gradient is s * h'(0.5), rounded once
    w2 = np.array([[0.3]], F32)
    g2 = A.run_bwd(np.ones_like(w2), w2, np.array([[0.5]], F32), sc, zp, lo, hi, False, device, lam=0.0,
                   beta=2.0).cpu().numpy()[0, 0]
    assert g2 == F32(np.float64(s) * np.float64(hp05)) and 0 < h05 < 1
    # the whole vector against the oracle too (bit for bit, lambda = 0)
    assert A.bits_equal(gv.reshape(1, -1), A.oracle_grad(g, w, v, sc, zp, lo, hi, 0.0, 2.0))
    assert A.bits_equal(y.reshape(1, -1), A.oracle_forward(w, v, sc, zp, lo, hi)[0])


def test_edges_host():
    check_edges("cpu")


def eager64(w, v, g, s, z, lo, hi, lam, beta):
    """float64 eager-torch composition of the same formulas; returns grad_V and its two
    summands' magnitudes (for the tolerance)."""
    w, g, s, z = (torch.as_tensor(a, dtype=torch.float64) for a in (w, g, s, z))
    v = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    sig = torch.sigmoid(v)
    h = torch.clamp(1.2 * sig - 0.1, 0, 1)
    r = torch.floor(w / s + z) + h
    y = (torch.clamp(r, lo, hi) - z) * s
    reg = torch.sum(1 - torch.abs(2 * h - 1) ** beta)
    (gy,) = torch.autograd.grad(torch.sum(y * g), v, retain_graph=True)
    (gr,) = torch.autograd.grad(lam * reg, v)
    return (gy + gr).numpy(), (gy.abs() + gr.abs()).numpy()


def check_function_gradient(device):
    """AdaRoundFn's grad_V on [4, 27] against the f64 composition to 1e-5 relative (relative
    to the summands' magnitude where lambda != 0: the two terms may cancel)."""
    w, _, g, sc, zp, lo, hi = A.make_case(4, 27, 4, False, True, seed=5)
    v = np.random.default_rng(6).uniform(-2, 2, w.shape).astype(F32)   # inside the rectified range
    s32, z32 = A.qp32(sc, zp, 4)
    for lam, beta in ((0.0, 2.0), (0.01, 2.0), (0.01, 3.7), (0.01, 20.0)):
        Vp = torch.from_numpy(v).to(device).requires_grad_(True)
        y, reg = AdaRoundFn.apply(Vp, torch.from_numpy(w).to(device), torch.from_numpy(sc), torch.from_numpy(zp), lo,
                                  hi, 0, lam, beta, False)
        y.backward(torch.from_numpy(g).to(device))
        ref, mag = eager64(w, v, g, s32, z32, lo, hi, lam, beta)
        err = np.abs(Vp.grad.cpu().numpy() - ref)
        print(lam, beta, "max rel err", (err / np.maximum(mag, 1e-300)).max())
        assert (err <= 1e-5 * mag).all()
        assert not reg.requires_grad and reg.dtype == torch.float64


def test_function_gradient_host():
    check_function_gradient("cpu")


def check_init_and_round_trip(device):
    layer, _ = A.build_layer(3, device)
    w = layer.get_weight_bias()[0].detach().clone()
    wq = layer.weight_quantizer
    s, z, lo, hi, axis, _ = wq.current_grid(w)
    ada = V.AdaRoundWeight().init_from(w, s, z, lo, hi)
    s32 = s.detach().to(torch.float32).reshape(-1, 1, 1, 1)
    t = (w / s32 + 0.0).double()
    frac = t - torch.floor(t)
    assert not bool((frac == 0.5).any())
    rtn = layer.quantize_weights(w)
    hard = ada.harden(w)
    # floor + 1 cannot produce the -0.0 that rint gives for t in (-0.5, 0): +0.0 there
    assert A.bits_equal(hard, rtn + 0.0)
    inside = (t >= 0) | (t <= -0.5)
    assert A.bits_equal(hard[inside], rtn[inside])
    ada.eval()
    assert A.bits_equal(ada(w), hard)
    # learned rounding: flip some V, harden, write into the layer, export, unpack
    with torch.no_grad():
        ada.V.mul_(torch.where(torch.rand(ada.V.shape, generator=torch.Generator().manual_seed(1)).to(device) < 0.3,
                               -1.0, 1.0))
    hard = ada.harden(w)
    with torch.no_grad():
        layer.get_weight_bias()[0].copy_(hard)
    packed, _ = layer.export_packed_weight()
    y, codes = unpack_dequant(packed, want_codes=True)
    assert A.bits_equal(y, hard + 0.0) and A.bits_equal(y[hard != 0], hard[hard != 0])
    b = torch.floor((w.double() / s32.double()).float())
    want = torch.clamp(b + (ada.V.detach() >= 0).float(), lo, hi)
    assert torch.equal(codes.to(torch.float32), want)
    assert A.bits_equal(layer.quantize_weights(layer.get_weight_bias()[0].detach()) + 0.0, hard + 0.0)


def test_init_and_round_trip_host():
    check_init_and_round_trip("cpu")


def check_end_to_end(device):
    layer, x = A.build_layer(0, device)
    rec = V.adaround_layer(layer, x, iters=200)
    print(rec)
    assert rec["mse_adaround"] < rec["mse_nearest"]
    w = layer.get_weight_bias()[0].detach()
    s, z, lo, hi, _, _ = layer.weight_quantizer.current_grid(w)
    s32 = s.to(torch.float32).reshape(-1, 1, 1, 1)
    c = torch.round(w / s32)
    # every h is exactly 0 or 1: each weight is an integer code of the grid times its scale
    assert torch.equal(w, c * s32) and float(c.min()) >= lo and float(c.max()) <= hi
    assert rec["flipped"] > 0


def test_end_to_end_host():
    check_end_to_end("cpu")


def test_model_driver_host():
    """adaround_model: forward order, input captured from the model as quantized so far, an
    unfolded-BN layer skipped and named."""
    import torch.nn as nn

    from vsiquantization_amd.modules.fused import ConvBnReLU
    l1, x = A.build_layer(1)
    l2, _ = A.build_layer(2)
    l2.conv_fuse = nn.Conv2d(8, 8, 3, padding=1)
    l2.weight_quantizer.observer = type(l2.weight_quantizer.observer)(True)
    l2.weight_quantizer.observer.num_bits = 4
    l2.weight_quantizer.quantize(l2.conv_fuse.weight.detach())
    cv, bn = nn.Conv2d(8, 4, 1), nn.BatchNorm2d(4)
    l3 = ConvBnReLU(cv, bn, nn.ReLU(), "PerChannelMSEObserver", "PerChannelUniformQuantizer", "MinMaxObserver",
                    "UniformQuantizer", True, True, False, 4, 8)
    l3.weight_quantizer.is_learning_scale = False
    l3.weight_quantizer.quantize(l3.conv_fuse.weight.detach())
    for l in (l1, l2, l3):
        l.quantize_out = False
    model = nn.Sequential(l1, l2, l3)
    with pytest.warns(RuntimeWarning, match="unfolded BatchNorm"):
        out = V.adaround_model(model, [x[:2], x[2:]], iters=20)
    assert list(out["layers"]) == ["0", "1"] and list(out["skipped"]) == ["2"]
    assert "is_fuse_bn=False" in out["skipped"]["2"]


def test_errors_host():
    w = torch.zeros(4, 8)
    v = torch.zeros(4, 8)
    for bad in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match=str(bad)):
            adaround_forward(w.to(bad), v, 0.1, 0, -8, 7)
        with pytest.raises(TypeError, match=str(bad)):
            adaround_backward(w, w, v.to(bad), 0.1, 0, -8, 7)
    with pytest.raises(ValueError, match="like w"):
        adaround_forward(w, torch.zeros(4, 9), 0.1, 0, -8, 7)
    with pytest.raises(RuntimeError, match="per-channel scale has 3 entries, the tensor has 4 channels"):
        adaround_forward(w, v, torch.ones(3), None, -8, 7, axis=0)
    with pytest.raises(ValueError, match="expected a scalar"):
        adaround_forward(w, v, torch.ones(4), None, -8, 7)
    lib = H.lib()
    one = torch.ones(1, dtype=torch.float64)
    y = torch.empty_like(w)
    args = (H.ptr(w), H.ptr(v), H.ptr(y), None, H.c_i64(4), H.c_i64(8), H.ptr(one), None)
    assert lib.vsiq_host_adaround_fwd_f32(*args, H.c_i64(3), 0, -8, 7, 0, 2.0, None) == -1     # nq
    assert lib.vsiq_host_adaround_fwd_f32(*args, H.c_i64(1), 0, 7, -8, 0, 2.0, None) == -1     # qmin > qmax
    assert lib.vsiq_adaround_fwd_f32(None, None, None, H.c_i64(4), H.c_i64(0), None, None, H.c_i64(1), 0, -8, 7, 0,
                                     2.0, None, None, H.c_i64(0), None, None) == -1            # before any pointer
    assert lib.vsiq_adaround_bwd_f32(None, None, None, None, H.c_i64(4), H.c_i64(8), None, None, H.c_i64(2), 0, -8, 7,
                                     0.0, 2.0, None) == -1
    assert lib.vsiq_adaround_workspace_doubles(H.c_i64(64), H.c_i64(27)) >= 64 * 8
    layer, x = A.build_layer(0)
    layer.weight_quantizer.scale = 1
    with pytest.raises(RuntimeError, match="neither observed nor learned"):
        V.adaround_layer(layer, x, iters=1)
