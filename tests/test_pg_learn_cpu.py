"""Learnable group scales (PerGroupLSQQuantizer) on CPU tensors: the host loop
(vsiq_host_pg_lsq_bwd_f32) against oracle/fakequant_np.py group by group and against the route that
existed before (PerChannelLearnFn on x.view(-1, G)), the argument errors of both C entry points, then
the Python layers: the autograd Function, the quantizer, the manager (calibrate, activate, one SGD
step), the state-dict round trip on a fused layer, what stays refused, and a short training loop."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests import pg_common as P
from tests import pg_learn_common as L
from vsiquantization_amd import _hip as H
from vsiquantization_amd.fakequant import PerGroupLearnFn, per_group_fake_quant, pg_lsq_backward
from vsiquantization_amd.modules.fused import ConvBnReLU, LinearBnReLU
from vsiquantization_amd.utils.quantize_manager import activate_learning_qparam

LEARN_ZP = (0, 1)


def _case(rows, rowlen, G, symmetric, nbits, learn_zp):
    x = P.weights(rows, rowlen, rows + rowlen)
    g = P.weights(rows, rowlen, 7) * 20
    qmin, qmax = P.grid(symmetric, nbits)
    s, z = L.make_qparams(x, G, symmetric, qmin, qmax, learn_zp)
    return x, g, s, z, qmin, qmax


def test_registry_and_exports():
    assert V.CLASS_REGISTRY["PerGroupLSQQuantizer"] is V.PerGroupLSQQuantizer
    from vsiquantization_amd.quantizers import PerGroupLSQQuantizer
    q = PerGroupLSQQuantizer(4, False, group_size=64)
    assert isinstance(q, V.PerGroupUniformQuantizer) and type(q) is not V.PerGroupUniformQuantizer
    assert not isinstance(q, (V.UniformQuantizer, V.PerChannelUniformQuantizer))
    assert q.learns_zero_point and not V.PerGroupLSQQuantizer(4, True).learns_zero_point
    assert not V.PerGroupUniformQuantizer(4, False).learns_zero_point
    assert q.group_size == 64 and (q.qmin, q.qmax) == (0, 15) and "PerGroupLSQQuantizer" in repr(q)
    assert V.pg_lsq_backward is pg_lsq_backward and V.PerGroupLearnFn is PerGroupLearnFn
    assert "vsiq_pg_lsq_bwd_f32" in H.EXPORTED and "vsiq_host_pg_lsq_bwd_f32" in H.EXPORTED
    assert H.lib().vsiq_abi_version() == 13


def test_entry_points_validate_on_host():
    """Argument errors are decided before any launch (no GPU needed), as vsiq_pg_fq_fwd_f32's."""
    lib, null = H.lib(), None
    dev, host = lib.vsiq_pg_lsq_bwd_f32, lib.vsiq_host_pg_lsq_bwd_f32

    def both(g=16, x=16, gx=16, rows=2, rowlen=64, group=32, s=16, z=16, zpl=0, qmin=-8, qmax=7, gs=16, gz=16):
        a = dev(g, x, gx, rows, rowlen, group, s, z, zpl, qmin, qmax, 0.1, gs, gz, null)
        b = host(g, x, gx, rows, rowlen, group, s, z, zpl, qmin, qmax, 0.1, gs, gz)
        assert a == b
        return a

    for group in (0, 16, 48, 100, 512, -32):
        assert both(group=group) == -1
        assert both(null, null, null, 0, 9, group, null, null, 0, -8, 7, null, null) == -1
    assert both(null, null, null, 0, 9, 32, null, null, 0, -8, 7, null, null) == 0      # rows == 0
    assert both(rows=-1) == -1 and both(rowlen=0) == -1 and both(qmin=7, qmax=-8) == -1
    for zpl in (2, -1, 3):                                                             # mode 2 is not offered
        assert both(zpl=zpl) == -1
    for missing in ("g", "x", "gx", "s", "z", "gs"):
        assert both(**{missing: null}) == -1, missing
    assert dev(16, 16, 16, 1 << 31, 64, 32, 16, 16, 0, -8, 7, 0.1, 16, 16, null) == -1   # too many row chunks


@pytest.mark.parametrize("learn_zp", LEARN_ZP)
@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
@pytest.mark.parametrize("rows,rowlen,G", P.SHAPES, ids=P.ids(P.SHAPES))
def test_host_loop_equals_the_oracle_and_the_parent_route(rows, rowlen, G, symmetric, nbits, learn_zp):
    x, g, s, z, qmin, qmax = _case(rows, rowlen, G, symmetric, nbits, learn_zp)
    tag = (rows, rowlen, G, symmetric, nbits, learn_zp)
    got = L.run(x, g, s, z, qmin, qmax, L.GSCALE, learn_zp, G)
    L.check_against_oracle(got, x, g, s, z, qmin, qmax, L.GSCALE, learn_zp, G, tag)
    if learn_zp and z.numel() >= 12:   # both kinds of zero point are present (make_qparams)
        out = ~L.zp_in_range(z, qmin, qmax)
        assert bool(out.any()) and bool((~out).any())
        assert bool((got["gz"][~out] != 0).any())
    if rowlen % G == 0:
        L.check_against_parent_route(got, x, g, s, z, qmin, qmax, L.GSCALE, learn_zp, G, tag)
    again = L.run(x, g, s, z, qmin, qmax, L.GSCALE, learn_zp, G)
    assert all(P.same_bits(again[k], got[k]) for k in got), tag


def test_nullable_zero_point_gradient():
    x, g, s, z, qmin, qmax = _case(3, 160, 64, False, 8, 1)
    _, gs, gz = pg_lsq_backward(g, x, s, z, qmin, qmax, 0.5, True, 64)
    gx2, gs2 = torch.empty_like(g), torch.empty_like(s)
    rc = H.lib().vsiq_host_pg_lsq_bwd_f32(H.ptr(g), H.ptr(x), H.ptr(gx2), 3, 160, 64, H.ptr(s), H.ptr(z), 1, qmin, qmax,
                                          0.5, H.ptr(gs2), None)
    assert rc == 0 and P.same_bits(gs2, gs) and bool((gz != 0).any())
    gz0 = torch.full_like(s, 7.0)
    rc = H.lib().vsiq_host_pg_lsq_bwd_f32(H.ptr(g), H.ptr(x), H.ptr(gx2), 3, 160, 64, H.ptr(s), H.ptr(z), 0, qmin, qmax,
                                          0.5, H.ptr(gs2), H.ptr(gz0))
    assert rc == 0 and bool((gz0 == 0).all())   # given with zp_learn == 0: written 0


@pytest.mark.parametrize("learn_zp", LEARN_ZP)
@pytest.mark.parametrize("G", [32, 128])
def test_special_groups_stay_in_their_group(G, learn_zp):
    """NaN / Inf in x or g: the group's grad_scale is non-finite, its neighbours' sums are the
    oracle's (vector-length and odd row lengths)."""
    for extra in (40, 41):
        x, g = L.special_case(G, extra)
        for symmetric, nbits in P.GRIDS:
            qmin, qmax = P.grid(symmetric, nbits)
            s, z = L.make_qparams(x, G, symmetric, qmin, qmax, learn_zp)
            got = L.run(x, g, s, z, qmin, qmax, L.GSCALE, learn_zp, G)
            L.check_special(got, got, x, g, s, z, qmin, qmax, L.GSCALE, learn_zp, G, (G, extra, symmetric, nbits))


def test_function_returns_gradients_in_the_parameters_shape_and_dtype():
    x, g, s, z, qmin, qmax = _case(4, 160, 64, False, 2, 1)
    want = L.run(x, g, s, z, qmin, qmax, 0.25, 1, 64)
    a = x.clone().requires_grad_(True)
    sp = s.float().reshape(-1).clone().requires_grad_(True)          # fp32, flat: any shape of rows * ngr entries
    zp = z.clone().requires_grad_(True)
    y = PerGroupLearnFn.apply(a, sp, zp, qmin, qmax, 0.25, True, 64)
    y.backward(g)
    ref = L.run(x, g, sp.detach(), z, qmin, qmax, 0.25, 1, 64)       # the scale as the fp32 Parameter holds it
    assert P.same_bits(y.detach(), ref["y"]) and P.same_bits(a.grad, ref["gx"])
    assert sp.grad.shape == sp.shape and sp.grad.dtype == torch.float32
    assert P.same_bits(sp.grad, ref["gs"].float().reshape(-1))
    assert zp.grad.shape == z.shape and zp.grad.dtype == torch.float64 and P.same_bits(zp.grad, ref["gz"])
    assert want["gs"].shape == (4, 3)
    b = x.clone().requires_grad_(True)                               # a zero point that is not learned: no gradient
    z0 = z.clone().requires_grad_(True)
    PerGroupLearnFn.apply(b, s, z0, qmin, qmax, 0.25, False, 64).backward(g)
    assert z0.grad is None and b.grad is not None


def test_type_and_size_checks():
    x, g, s, z, qmin, qmax = _case(4, 64, 32, True, 4, 0)
    for bad in (x.bfloat16(), x.half(), x.double()):
        with pytest.raises(TypeError):
            pg_lsq_backward(bad, x, s, z, qmin, qmax, 0.1, False, 32)
        with pytest.raises(TypeError):
            pg_lsq_backward(g, bad, s, z, qmin, qmax, 0.1, False, 32)
        with pytest.raises(TypeError):
            PerGroupLearnFn.apply(bad, s, z, qmin, qmax, 0.1, False, 32)
        with pytest.raises(TypeError):
            V.PerGroupLSQQuantizer(4, True, 32).quantize(bad, s, z, True)
    with pytest.raises(ValueError):
        pg_lsq_backward(g, x, s.reshape(-1)[1:], z, qmin, qmax, 0.1, False, 32)
    with pytest.raises(ValueError):
        pg_lsq_backward(g, x, s, z.reshape(-1)[1:], qmin, qmax, 0.1, False, 32)
    with pytest.raises(ValueError):
        pg_lsq_backward(g[:2], x, s, z, qmin, qmax, 0.1, False, 32)
    with pytest.raises(ValueError):
        pg_lsq_backward(g, x, s, z, qmin, qmax, 0.1, False, 48)
    with pytest.raises(TypeError):
        pg_lsq_backward(g, x, 0.1, z, qmin, qmax, 0.1, False, 32)


# ------------------------------------------------------------------ quantizer and manager
def test_quantizer_paths():
    x, g, s, z, qmin, qmax = _case(5, 200, 64, False, 4, 1)
    q = V.PerGroupLSQQuantizer(4, False, group_size=64)
    gscale = (q.qmax * 64) ** -0.5                       # the nominal count, also for the short last group (8 of 64)
    ref = L.run(x, g, s, z, qmin, qmax, gscale, 1, 64)
    a, sp, zp = x.clone().requires_grad_(True), s.clone().requires_grad_(True), z.clone().requires_grad_(True)
    y = q.quantize(a, sp, zp, True)
    y.backward(g)
    assert P.same_bits(y.detach(), ref["y"]) and P.same_bits(a.grad, ref["gx"])
    assert P.same_bits(sp.grad, ref["gs"]) and P.same_bits(zp.grad, ref["gz"])
    with torch.no_grad():                                # the same forward without the Function
        yn = q.quantize(a, sp, zp, True)
    assert yn.grad_fn is None and P.same_bits(yn, ref["y"])
    yx = q.quantize(x, s, z, True)                       # nothing requires grad
    assert yx.grad_fn is None and P.same_bits(yx, ref["y"])
    frozen = q.quantize(x, sp, zp, True)                 # a frozen x still trains its qparams
    sp.grad = None
    frozen.backward(g)
    assert P.same_bits(sp.grad, ref["gs"])
    # is_learning_scale False: the base class (zero point as given, STE backward)
    base = V.PerGroupUniformQuantizer(4, False, group_size=64)
    assert P.same_bits(q.quantize(x, s, z, False), base.quantize(x, s, z, False))
    with pytest.raises(NotImplementedError, match="PerGroup"):
        q.quantize(x, s, z, True, act="relu")
    with pytest.raises(RuntimeError, match="PerGroupLSQQuantizer"):
        q.quantize(x, 1, 0, True)
    # symmetric: the manager's scalar 0 is expanded to zeros, and no zero-point gradient comes back
    qs = V.PerGroupLSQQuantizer(4, True, group_size=64)
    ss, _ = L.make_qparams(x, 64, True, -8, 7, 0)
    b, sq = x.clone().requires_grad_(True), ss.clone().requires_grad_(True)
    ys = qs.quantize(b, sq, 0, True)
    ys.backward(g)
    refs = L.run(x, g, ss, torch.zeros_like(ss), -8, 7, (7 * 64) ** -0.5, 0, 64)
    assert P.same_bits(ys.detach(), refs["y"]) and P.same_bits(b.grad, refs["gx"]) and P.same_bits(sq.grad, refs["gs"])


def _manager(bits=4, sym=True, G=64, learn=False):
    qm = V.QuantizationManager("PerGroupLSQQuantizer", "PerGroupMinMaxObserver", bits, sym, learn)
    qm.quantizer.group_size = G
    return qm


@pytest.mark.parametrize("sym", [True, False])
def test_manager_calibrate_then_learn(sym):
    x, g = P.weights(6, 200, 4), P.weights(6, 200, 5) * 20
    qm = _manager(bits=4 if sym else 8, sym=sym)          # the manager's observer is 8-bit: zero points on uint8
    qmin, qmax = qm.quantizer.qmin, qm.quantizer.qmax
    want = P.expected(x, 64, sym, qmin, qmax)
    assert P.same_bits(qm.quantize(x), want["y"]) and qm.observer.group_size == 64   # observing: as the base class
    with pytest.raises(RuntimeError, match="PerGroupLSQQuantizer"):
        _manager(learn=True).quantize(x)                  # learning before anything was observed
    state = (qm.observer.run_min.clone(), qm.observer.run_max.clone())
    qm.is_learning_scale = True
    qm.init_scaling_factor_for_learning()                 # leaves the observed group qparams in place
    assert P.same_bits(qm.scale, want["scale"]) and not qm.mean_abs_x
    qm.make_learn_qparameter()
    assert isinstance(qm.scale, nn.Parameter) and qm.scale.dtype == torch.float64 and qm.scale.shape == (6, 4)
    assert P.same_bits(qm.scale.detach(), want["scale"])
    if sym:
        assert qm.zero_point == 0 and [n for n, _ in qm.named_parameters()] == ["scale"]
    else:
        assert isinstance(qm.zero_point, nn.Parameter) and P.same_bits(qm.zero_point.detach(), want["zp"] + 1e-9)
    a = x.clone().requires_grad_(True)
    y = qm.quantize(a)
    y.backward(g)
    z = qm.zero_point.detach() if not sym else torch.zeros(6, 4, dtype=torch.float64)
    ref = L.run(x, g, want["scale"], z, qmin, qmax, (qmax * 64) ** -0.5, int(not sym), 64)
    assert P.same_bits(y.detach(), ref["y"]) and P.same_bits(a.grad, ref["gx"]) and P.same_bits(qm.scale.grad, ref["gs"])
    if not sym:
        assert P.same_bits(qm.zero_point.grad, ref["gz"])   # zeros: the observed range clamps nothing
    before = qm.scale.detach().clone()
    torch.optim.SGD(qm.parameters(), lr=1e-3).step()
    assert bool((qm.scale.detach() != before).any()) and qm.scale.shape == (6, 4)
    assert torch.equal(qm.observer.run_min, state[0]) and torch.equal(qm.observer.run_max, state[1])
    assert not qm.mean_abs_x                              # no observer call, no stats record while learning
    qm.is_quantize = False
    assert qm.quantize(x) is x


def _layer(seed, qname="PerGroupLSQQuantizer", G=64):
    torch.manual_seed(seed)
    layer = LinearBnReLU(nn.Linear(200, 5), nn.BatchNorm1d(5), nn.ReLU(), "PerGroupMinMaxObserver", qname,
                         "MinMaxObserver", "UniformQuantizer", True, True, True, 4, 8)
    layer.weight_quantizer.quantizer.group_size = G
    return layer


def _calibrated_learning_layer(seed, x):
    layer = _layer(seed)
    for q in (layer.weight_quantizer, layer.activation_quantizer):
        q.is_learning_scale = False
    layer(x)                                              # calibration: observed qparams, activation stats
    model = nn.Sequential(layer)
    activate_learning_qparam(model)                       # the default use_init=True
    return model, layer


def test_fused_layer_trains_its_group_scales_and_round_trips():
    x = torch.randn(3, 200, generator=torch.Generator().manual_seed(3))
    model, layer = _calibrated_learning_layer(1, x)
    wq = layer.weight_quantizer
    w = layer.get_weight_bias()[0].detach()
    observed = P.expected(w, 64, True, -8, 7)
    assert isinstance(wq.scale, nn.Parameter) and P.same_bits(wq.scale.detach(), observed["scale"])
    assert "0.weight_quantizer.scale" in dict(model.named_parameters())
    state = wq.observer.run_max.clone()
    opt = torch.optim.SGD(model.parameters(), lr=1e-2)
    model(x).square().mean().backward()
    assert wq.scale.grad.shape == (5, 4) and bool((wq.scale.grad != 0).any())
    assert bool(torch.isfinite(wq.scale.grad).all())
    opt.step()
    assert bool((wq.scale.detach() != observed["scale"]).any()) and torch.equal(wq.observer.run_max, state)
    # state dict: the trained [rows, groups] Parameter comes back bit for bit in a second layer
    other_model, other = _calibrated_learning_layer(2, x * 2)
    assert not P.same_bits(other.weight_quantizer.scale.detach(), wq.scale.detach())
    sd = model.state_dict()
    assert sd["0.weight_quantizer.scale"].shape == (5, 4) and sd["0.weight_quantizer.scale"].dtype == torch.float64
    other_model.load_state_dict(sd)
    assert P.same_bits(other.weight_quantizer.scale.detach(), wq.scale.detach())
    model.eval(), other_model.eval()
    with torch.no_grad():
        assert P.same_bits(other_model(x), model(x))


def test_asymmetric_layer_round_trips_its_zero_points():
    x = torch.randn(3, 200, generator=torch.Generator().manual_seed(3))

    def build(seed, inp):
        torch.manual_seed(seed)
        layer = LinearBnReLU(nn.Linear(200, 5), nn.BatchNorm1d(5), nn.ReLU(), "PerGroupMinMaxObserver",
                             "PerGroupLSQQuantizer", "MinMaxObserver", "UniformQuantizer", False, True, True, 4, 8)
        for q in (layer.weight_quantizer, layer.activation_quantizer):
            q.is_learning_scale = False
        layer(inp)
        model = nn.Sequential(layer)
        activate_learning_qparam(model)
        return model, layer.weight_quantizer

    model, wq = build(1, x)
    assert isinstance(wq.zero_point, nn.Parameter) and wq.zero_point.shape == (5, 2)
    model(x).square().mean().backward()
    assert wq.zero_point.grad.shape == (5, 2) and wq.scale.grad.shape == (5, 2)
    torch.optim.SGD(model.parameters(), lr=1e-2).step()
    other_model, owq = build(2, x * 3)
    other_model.load_state_dict(model.state_dict())
    assert P.same_bits(owq.zero_point.detach(), wq.zero_point.detach()) and P.same_bits(owq.scale.detach(), wq.scale.detach())


def test_what_stays_refused_names_the_class():
    x = P.weights(4, 64, 1)
    qm = _manager(G=32)
    with pytest.raises(RuntimeError, match="PerGroupLSQQuantizer"):
        qm.make_learn_qparameter()                        # nothing observed yet
    with pytest.raises(NotImplementedError, match="PerGroup"):
        qm.quantize(x, act="relu")
    qm.quantize(x)
    for call in (qm.export_packed, qm.current_grid):
        with pytest.raises(NotImplementedError, match="PerGroupLSQQuantizer"):
            call(x)
    qm.is_learning_scale = True
    qm.make_learn_qparameter()
    for call in (qm.export_packed, qm.current_grid):
        with pytest.raises(NotImplementedError, match="PerGroupLSQQuantizer"):
            call(x)
    layer = _layer(0, G=32)
    layer.weight_quantizer.is_learning_scale = False
    layer.weight_quantizer.quantize(layer.get_weight_bias()[0].detach())
    with pytest.raises(NotImplementedError, match="PerGroupLSQQuantizer"):
        V.adaround_layer(layer, torch.randn(8, 200))
    with pytest.raises(NotImplementedError, match="PerGroupLSQQuantizer"):
        layer.export_packed_weight()
    for obs, q in (("MinMaxObserver", "PerGroupLSQQuantizer"), ("PerChannelMinMaxObserver", "PerGroupLSQQuantizer")):
        mixed = V.QuantizationManager(q, obs, 4, True, False)
        with pytest.raises(NotImplementedError, match="PerGroup"):
            mixed.quantize(x)
        with pytest.raises(NotImplementedError, match="PerGroup"):
            mixed.make_learn_qparameter()
    with pytest.raises(NotImplementedError, match="PerGroup"):   # as an activation quantizer
        ConvBnReLU(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.ReLU(), "MinMaxObserver", "UniformQuantizer",
                   "MinMaxObserver", "PerGroupLSQQuantizer", True, True, True, 4, 8)
    dist = _manager(G=32)
    dist.dist_group = object()
    with pytest.raises(NotImplementedError, match="PerGroupMinMaxObserver"):
        dist.quantize(x)
    for bad in (x.bfloat16(), x.half(), x.double()):
        with pytest.raises(TypeError):
            _manager(G=32).quantize(bad)
    # the base class keeps every refusal it had
    base = V.QuantizationManager("PerGroupUniformQuantizer", "PerGroupMinMaxObserver", 4, True, False)
    base.quantize(x)
    with pytest.raises(NotImplementedError, match="PerGroup"):
        base.make_learn_qparameter()
    base.is_learning_scale = True
    with pytest.raises(NotImplementedError, match="PerGroup"):
        base.quantize(x)


def test_twenty_steps_on_the_scales_lower_the_quantization_error():
    """Symmetric 3-bit, G = 64, a 4 x 256 weight: gradient descent on the [4, 4] scales alone, from
    the observed (min / max) scales, lowers ||fq(w) - w||^2."""
    w = torch.randn(4, 256, generator=torch.Generator().manual_seed(0))
    qm = _manager(bits=3, G=64)
    qm.quantize(w)
    qm.is_learning_scale = True
    qm.make_learn_qparameter()
    start = qm.scale.detach().clone()
    opt = torch.optim.SGD([qm.scale], lr=2e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = (qm.quantize(w) - w).square().sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses
    assert bool((qm.scale.detach() != start).all()) and bool((qm.scale.detach() > 0).all())
