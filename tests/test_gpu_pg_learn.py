"""Learnable group scales on MI355X (csrc/k_pg.hip k_pg_lsq_bwd): the one-launch backward against
oracle/fakequant_np.py group by group, the host loops and the route that existed before
(PerChannelLearnFn / K6 on x.view(-1, G)), at the smallest shapes at which each mechanism of the
kernel can fail (tests/pg_common.py's table); then an offset view, both tasks-per-wave arms, zero
points outside the grid and at ties (every case: pg_learn_common.make_qparams), non-finite groups,
a fused layer's training step against the CPU's, and HIP-graph capture.

y and grad_x are compared bit for bit; the f64 gradients with the bar of pg_learn_common (their
addition order is the kernel's own)."""
import copy

import pytest
import torch
import torch.nn as nn

from tests import pg_common as P
from tests import pg_learn_common as L
from vsiquantization_amd.fakequant import per_group_fake_quant, pg_lsq_backward
from vsiquantization_amd.modules.fused import LinearBnReLU
from vsiquantization_amd.utils.quantize_manager import activate_learning_qparam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEARN_ZP = (0, 1)


def _offset_view(xc):
    buf = torch.empty(xc.numel() + 1, dtype=torch.float32, device=DEV)   # a view one element into a buffer
    x = buf[1:].view(xc.shape)
    x.copy_(xc)
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    return x


def _device_and_host(xc, gc, s, z, qmin, qmax, learn_zp, G, tag, x=None, g=None):
    """The device route and the host loops on the same data: y and gx bit for bit, and the device
    twice gives the same bits everywhere."""
    x = xc.to(DEV) if x is None else x
    g = gc.to(DEV) if g is None else g
    got = L.run(x, g, s.to(DEV), z.to(DEV), qmin, qmax, L.GSCALE, learn_zp, G)
    host = L.run(xc, gc, s, z, qmin, qmax, L.GSCALE, learn_zp, G)
    assert P.same_bits(got["y"].cpu(), host["y"]) and P.same_bits(got["gx"].cpu(), host["gx"]), (tag, "host")
    again = L.run(x, g, s.to(DEV), z.to(DEV), qmin, qmax, L.GSCALE, learn_zp, G)
    assert all(P.same_bits(again[k], got[k]) for k in got), (tag, "run to run")
    return got, host


def _check_finite(xc, gc, G, symmetric, nbits, learn_zp, tag, offset=False, oracle=True):
    qmin, qmax = P.grid(symmetric, nbits)
    s, z = L.make_qparams(xc, G, symmetric, qmin, qmax, learn_zp)
    x, g = (_offset_view(xc), _offset_view(gc)) if offset else (xc.to(DEV), gc.to(DEV))
    got, host = _device_and_host(xc, gc, s, z, qmin, qmax, learn_zp, G, tag, x=x, g=g)
    Ts, Tz, fin_s, fin_z = L.terms(xc, gc, s, z, qmin, qmax, learn_zp, G)
    assert fin_s.all() and fin_z.all(), tag
    assert not len(L.within_bar(got["gs"], host["gs"].numpy(), Ts, L.GSCALE)), (tag, "grad_scale against the host loop")
    assert not len(L.within_bar(got["gz"], host["gz"].numpy(), Tz, L.GSCALE)), (tag, "grad_zp against the host loop")
    out = ~L.zp_in_range(z, qmin, qmax) if learn_zp else torch.ones_like(z, dtype=torch.bool)
    assert bool((got["gz"].cpu()[out] == 0).all()), (tag, "grad_zp exactly 0")
    if oracle:
        L.check_against_oracle(got, xc, gc, s, z, qmin, qmax, L.GSCALE, learn_zp, G, tag)
    rowlen = xc.numel() // xc.shape[0]
    if rowlen % G == 0 and not offset:
        L.check_against_parent_route(got, x, g, s, z, qmin, qmax, L.GSCALE, learn_zp, G, tag)
    return got


@pytest.mark.parametrize("learn_zp", LEARN_ZP)
@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
@pytest.mark.parametrize("rows,rowlen,G", P.SHAPES, ids=P.ids(P.SHAPES))
def test_kernel_equals_the_oracle_the_host_loops_and_the_parent_route(rows, rowlen, G, symmetric, nbits, learn_zp):
    xc, gc = P.weights(rows, rowlen, rows + rowlen), P.weights(rows, rowlen, 7) * 20
    _check_finite(xc, gc, G, symmetric, nbits, learn_zp, (rows, rowlen, G, symmetric, nbits, learn_zp))


@pytest.mark.parametrize("learn_zp", LEARN_ZP)
@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
def test_view_offset_by_one_element_takes_the_scalar_path(symmetric, nbits, learn_zp):
    xc, gc = P.weights(5, 96, 13), P.weights(5, 96, 14) * 20
    _check_finite(xc, gc, 32, symmetric, nbits, learn_zp, ("offset", symmetric, nbits, learn_zp), offset=True)


@pytest.mark.parametrize("learn_zp", LEARN_ZP)
def test_four_tasks_per_wave_from_the_grid_size_threshold_on(learn_zp):
    """pg_per_wave's threshold (64 wave tasks per CU): the smallest tensor over it, with a 4-element
    last chunk per row (rowlen 3076 = 12 * 256 + 4: 63 padding lanes that must add zero) and a last
    workgroup that is not full, and the largest one under it.  Against the host loops (the
    definition); the oracle loop over these 16 000 groups is left to the small shapes."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for rows in (-(-64 * cus // 13) + 1, 64 * cus // 13 - 1):
        assert (rows * 13 >= 64 * cus) == (rows > 64 * cus // 13)
        xc, gc = P.weights(rows, 3076, rows), P.weights(rows, 3076, 7) * 20
        _check_finite(xc, gc, 128, False, 2, learn_zp, ("tasks per wave", rows, learn_zp), oracle=False)


@pytest.mark.parametrize("learn_zp", LEARN_ZP)
@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
@pytest.mark.parametrize("G", [32, 128])
def test_non_finite_groups_stay_in_their_group(G, symmetric, nbits, learn_zp):
    """NaN / Inf in x or g in the waves that also hold ordinary groups, vector and scalar path: gx
    is the host loop's, the group's grad_scale non-finite in the host loop's way, and the
    neighbouring groups' sums meet the finite bar."""
    qmin, qmax = P.grid(symmetric, nbits)
    for extra in (40, 41):
        xc, gc = L.special_case(G, extra)
        s, z = L.make_qparams(xc, G, symmetric, qmin, qmax, learn_zp)
        tag = ("special", G, extra, symmetric, nbits, learn_zp)
        got, host = _device_and_host(xc, gc, s, z, qmin, qmax, learn_zp, G, tag)
        L.check_special(got, host, xc, gc, s, z, qmin, qmax, L.GSCALE, learn_zp, G, tag)


def _learning_layer(symmetric, bits, x):
    torch.manual_seed(1)
    layer = LinearBnReLU(nn.Linear(200, 5), nn.BatchNorm1d(5), nn.ReLU(), "PerGroupMinMaxObserver",
                         "PerGroupLSQQuantizer", "MinMaxObserver", "UniformQuantizer", symmetric, True, True, bits, 8)
    layer.weight_quantizer.quantizer.group_size = 64
    for q in (layer.weight_quantizer, layer.activation_quantizer):
        q.is_learning_scale = False
    layer(x)                                              # calibration
    model = nn.Sequential(layer)
    activate_learning_qparam(model)
    return model, layer


@pytest.mark.parametrize("symmetric,bits", [(True, 4), (False, 8)])
def test_fused_layer_training_step_equals_the_cpu_step(symmetric, bits):
    xc = torch.randn(3, 200, generator=torch.Generator().manual_seed(3))
    model_c, layer_c = _learning_layer(symmetric, bits, xc)
    model_g = copy.deepcopy(model_c).to(DEV)
    layer_g = model_g[0]
    wq_c, wq_g = layer_c.weight_quantizer, layer_g.weight_quantizer
    assert wq_g.scale.is_cuda and P.same_bits(wq_g.scale.detach().cpu(), wq_c.scale.detach())
    # the weight quantizer's step on the same weight and grad_output: y and w.grad bit for bit
    wc = (layer_c.get_weight_bias()[0].detach() * 1.3).requires_grad_(True)   # 1.3: the learned scales clamp some
    wg = wc.detach().to(DEV).requires_grad_(True)
    gc = P.weights(5, 200, 9) * 20
    yc, yg = wq_c.quantize(wc), wq_g.quantize(wg)
    yc.backward(gc)
    yg.backward(gc.to(DEV))
    assert P.same_bits(yg.detach().cpu(), yc.detach()) and P.same_bits(wg.grad.cpu(), wc.grad)
    q = wq_c.quantizer
    gscale = (q.qmax * 64) ** -0.5
    z = wq_c.zero_point.detach() if not symmetric else torch.zeros(5, 4, dtype=torch.float64)
    Ts, Tz, fin_s, fin_z = L.terms(wc, gc, wq_c.scale.detach(), z, q.qmin, q.qmax, int(not symmetric), 64)
    assert fin_s.all() and fin_z.all() and bool((wq_c.scale.grad != 0).any())
    assert wq_g.scale.grad.shape == (5, 4) and wq_g.scale.grad.dtype == torch.float64
    assert not len(L.within_bar(wq_g.scale.grad, wq_c.scale.grad.numpy(), Ts, gscale))
    if not symmetric:
        assert not len(L.within_bar(wq_g.zero_point.grad, wq_c.zero_point.grad.numpy(), Tz, gscale))
    # and the whole layer trains on the device: finite gradients, the scales move, nothing observed
    before = wq_g.scale.detach().clone()
    wq_g.scale.grad = None
    opt = torch.optim.SGD(model_g.parameters(), lr=1e-2)
    model_g(xc.to(DEV)).square().mean().backward()
    assert bool(torch.isfinite(wq_g.scale.grad).all()) and bool((wq_g.scale.grad != 0).any())
    opt.step()
    assert bool((wq_g.scale.detach() != before).any())
    sd = model_g.state_dict()
    assert sd["0.weight_quantizer.scale"].shape == (5, 4)
    model_c.load_state_dict(sd)
    assert P.same_bits(wq_c.scale.detach(), wq_g.scale.detach().cpu())


# ------------------------------------------------------------------ HIP-graph capture
def _captured(fn, warm):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_graph_replay_equals_eager():
    rows, rowlen, G = 9, 576, 64
    x1, x2 = P.weights(rows, rowlen, 1).to(DEV), (P.weights(rows, rowlen, 20) * 2).to(DEV)
    g1, g2 = P.weights(rows, rowlen, 3).to(DEV), (P.weights(rows, rowlen, 4) * 30).to(DEV)
    s, z = L.make_qparams(x2, G, False, 0, 15, 1)
    s, z = s.to(DEV), z.to(DEV)
    want_y = per_group_fake_quant(x2, s, z, 0, 15, group_size=G, zp_round=True)[0]
    want = pg_lsq_backward(g2, x2, s, z, 0, 15, 0.05, True, G)
    assert bool((want[1] != 0).any()) and bool((want[2] != 0).any())

    xs = x1.clone()
    fwd = lambda: per_group_fake_quant(xs, s, z, 0, 15, group_size=G, zp_round=True)[0]   # noqa: E731
    graph, y = _captured(fwd, fwd)
    xs.copy_(x2)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(y, want_y)

    # the backward in a capture of its own (never autograd.backward inside a capture)
    gs = g1.clone()
    bwd = lambda: pg_lsq_backward(gs, xs, s, z, 0, 15, 0.05, True, G)   # noqa: E731
    bgraph, got = _captured(bwd, bwd)
    gs.copy_(g2)
    for _ in range(2):
        bgraph.replay()
    torch.cuda.synchronize()
    for a, b, name in zip(got, want, ("gx", "grad_scale", "grad_zp")):
        assert P.same_bits(a, b), name
