"""Group-wise (per-group) weight quantization on MI355X (csrc/k_pg.hip): the one-launch observe +
fake quant, the fixed forward and the STE backward against the code that existed before them --
K3 (per_channel_observe_fq) on the tensor cut into rows of one group each, tests/pg_common.py --
and against the host loops, bit for bit, at the smallest shapes at which each mechanism of the
kernel can fail; then an offset view, special groups, the manager, and HIP-graph capture."""
import pytest
import torch

import vsiquantization_amd as V
from tests import pg_common as P
from vsiquantization_amd.fakequant import (PerGroupFQFn, PerGroupObserveFQFn, per_group_fake_quant,
                                           per_group_observe_fq, pg_ste_backward)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# rows x rowlen, G                       what it exercises
#    3 x 32     32     one group per row, 8 lanes
#    5 x 96     32     several groups per wave, rows not wave-aligned
#    4 x 160    64     short last group (32 of 64)
#    7 x 27     32     scalar path, one short group
#    2 x 1000   128    crosses mask words, last group 104
#    3 x 1027   128    scalar path across words
#    2 x 300    256    whole-wave group + tail of 44
#   64 x 4608   128    many workgroups, a real layer's row
#    1 x 20480  64     a row split over workgroups
SHAPES = P.SHAPES


def _run(x, G, symmetric, nbits, **kw):
    qmin, qmax = P.grid(symmetric, nbits)
    return per_group_observe_fq(x, group_size=G, symmetric=symmetric, qmin=qmin, qmax=qmax, **kw)


def _offset_view(xc):
    buf = torch.empty(xc.numel() + 1, dtype=torch.float32, device=DEV)   # a view one element into a buffer
    x = buf[1:].view(xc.shape)
    x.copy_(xc)
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    return x


def _check_all(xc, G, symmetric, nbits, tag, x=None):
    """Device == K3 on the reshaped pieces == host loops: y, codes, scale, zp, run_min, run_max, the
    unpacked mask and grad_x; the fixed forward and observe-only agree with the fused call."""
    rows, rowlen = xc.shape[0], xc.numel() // xc.shape[0]
    qmin, qmax = P.grid(symmetric, nbits)
    x = xc.to(DEV) if x is None else x
    gc = P.weights(rows, rowlen, 77) * 20
    g = gc.to(DEV)
    want = P.expected(x, G, symmetric, qmin, qmax, want_codes=True, g=g)
    got = _run(x, G, symmetric, nbits, want_mask=True, want_codes=True)
    P.check(got, want, rows, rowlen, tag, codes=True)
    gx = pg_ste_backward(g, got["mask"], got["scale"], G)
    assert P.same_bits(gx, want["gx"]), tag
    host = _run(xc, G, symmetric, nbits, want_mask=True)
    for k in ("y", "scale", "zp", "run_min", "run_max"):
        assert P.same_bits(got[k].cpu(), host[k]), (tag, "host", k)
    assert torch.equal(P.unpack_mask(got["mask"], rows, rowlen), P.unpack_mask(host["mask"], rows, rowlen)), tag
    assert P.same_bits(gx.cpu(), pg_ste_backward(gc, host["mask"], host["scale"], G)), tag
    y, mask, codes = per_group_fake_quant(x, got["scale"], got["zp"], qmin, qmax, group_size=G, want_mask=True,
                                          want_codes=True)
    assert P.same_bits(y, got["y"]) and torch.equal(codes, got["codes"]), tag
    assert torch.equal(P.unpack_mask(mask, rows, rowlen), want["mask"]), tag
    plain = _run(x, G, symmetric, nbits)                       # no mask, no codes: another instantiation
    only = _run(x, G, symmetric, nbits, quantize=False)
    assert P.same_bits(plain["y"], got["y"]) and only["y"] is None, tag
    for k in ("scale", "zp", "run_min", "run_max"):
        assert P.same_bits(only[k], got[k]) and P.same_bits(plain[k], got[k]), (tag, k)


@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
@pytest.mark.parametrize("rows,rowlen,G", SHAPES, ids=P.ids(SHAPES))
def test_kernels_equal_the_reshaped_k3_route_and_the_host_loops(rows, rowlen, G, symmetric, nbits):
    _check_all(P.weights(rows, rowlen, rows + rowlen), G, symmetric, nbits, (rows, rowlen, G, symmetric, nbits))


def test_four_tasks_per_wave_from_the_grid_size_threshold_on():
    """From 64 wave tasks (256-element row chunks) per CU on, a wave takes 4 tasks instead of 1
    (k_pg.hip pg_per_wave): the smallest tensor over that threshold, with a 4-element last chunk
    per row (rowlen 3076 = 12 * 256 + 4) and a last workgroup that is not full, and the
    largest one still under it."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for rows in (-(-64 * cus // 13) + 1, 64 * cus // 13 - 1):
        assert (rows * 13 >= 64 * cus) == (rows > 64 * cus // 13)
        _check_all(P.weights(rows, 3076, rows), 128, False, 2, ("tasks per wave", rows))


@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
def test_view_offset_by_one_element_takes_the_scalar_path(symmetric, nbits):
    xc = P.weights(5, 96, 13)
    _check_all(xc, 32, symmetric, nbits, ("offset", symmetric, nbits), x=_offset_view(xc))


@pytest.mark.parametrize("symmetric,nbits", P.GRIDS, ids=P.ids(P.GRIDS))
@pytest.mark.parametrize("G", [32, 128])
def test_special_groups_next_to_ordinary_ones(G, symmetric, nbits):
    """NaN, +Inf, all-zero and constant groups in the waves that also hold ordinary groups (G = 32:
    all in one wave; G = 128: two groups per wave), vector and scalar path."""
    for extra in (40, 41):
        xc = P.with_special_groups(P.weights(2, 8 * G + extra, 11), G)
        _check_all(xc, G, symmetric, nbits, ("special", G, extra, symmetric, nbits))


def test_state_carried_over_two_calls():
    rows, rowlen, G = 4, 160, 64
    a, b = P.weights(rows, rowlen, 1).to(DEV), (P.weights(rows, rowlen, 2) * 3).to(DEV)
    mn, mx = torch.zeros(rows, 3, device=DEV), torch.zeros(rows, 3, device=DEV)
    _run(a, G, False, 8, run_min=mn, run_max=mx)
    state = (mn.clone(), mx.clone())
    want = P.expected(b, G, False, 0, 255, run_min=state[0], run_max=state[1], want_codes=True)
    got = _run(b, G, False, 8, run_min=mn, run_max=mx, want_mask=True, want_codes=True)
    P.check(got, want, rows, rowlen, "second call", codes=True)
    assert got["run_min"] is mn and bool((mn < state[0]).any())


def test_autograd_and_manager():
    rows, rowlen, G = 6, 200, 64
    xc, gc = P.weights(rows, rowlen, 9), P.weights(rows, rowlen, 10) * 50
    x, g = xc.to(DEV), gc.to(DEV)
    want = P.expected(x, G, True, -8, 7, g=g)
    a = x.clone().requires_grad_(True)
    y, s, z = PerGroupObserveFQFn.apply(a, G, True, -8, 7, 8, 1e-8, None, None)
    y.backward(g)
    assert P.same_bits(y, want["y"]) and P.same_bits(a.grad.reshape(rows, rowlen), want["gx"])
    b = x.clone().requires_grad_(True)
    PerGroupFQFn.apply(b, s, z, -8, 7, G).backward(g)
    assert P.same_bits(b.grad, a.grad)
    qm = V.QuantizationManager("PerGroupUniformQuantizer", "PerGroupMinMaxObserver", 4, True, False)
    qm.quantizer.group_size = G
    c = x.clone().requires_grad_(True)
    yq = qm.quantize(c)
    yq.backward(g)
    assert P.same_bits(yq, want["y"]) and P.same_bits(c.grad, a.grad) and P.same_bits(qm.scale, want["scale"])
    qm.is_observer_qparam = False
    assert P.same_bits(qm.quantize(x), want["y"])
    with pytest.raises(TypeError, match="bfloat16"):
        qm.quantize(x.bfloat16())
    with pytest.raises(TypeError, match="float16"):
        per_group_observe_fq(x.half(), group_size=G, symmetric=True, qmin=-8, qmax=7)


def test_calibrate_qat_model_with_default_arguments():
    """The documented calibration call defers the per-tensor observers by default; a group-wise
    weight manager observes per call under it."""
    import torch.nn as nn

    from vsiquantization_amd.modules.fused import LinearBnReLU
    from vsiquantization_amd.utils.quantize_manager import calibrate_qat_model
    torch.manual_seed(2)
    layer = LinearBnReLU(nn.Linear(200, 5), nn.BatchNorm1d(5), nn.ReLU(), "PerGroupMinMaxObserver",
                         "PerGroupUniformQuantizer", "MinMaxObserver", "UniformQuantizer", True, True, True, 4, 8)
    layer.weight_quantizer.quantizer.group_size = 64
    model = nn.Sequential(layer).to(DEV)
    batches = [torch.randn(3, 200, device=DEV), torch.randn(3, 200, device=DEV)]
    calibrate_qat_model(model, batches, lambda m, loader, dev: [m(b) for b in loader])
    wq, aq = layer.weight_quantizer, layer.activation_quantizer
    w = layer.get_weight_bias()[0].detach()
    first = P.expected(w, 64, True, -8, 7)
    want = P.expected(w, 64, True, -8, 7, run_min=first["run_min"], run_max=first["run_max"])   # two calls
    assert P.same_bits(wq.scale, want["scale"]) and P.same_bits(wq.zero_point, want["zp"])
    assert P.same_bits(wq.observer.run_max, want["run_max"]) and wq.scale.shape == (5, 4)
    assert len(aq.mean_abs_x) == 2 and float(aq.scale) > 0   # the activation side was deferred and folded


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
    kw = dict(group_size=G, symmetric=False, qmin=0, qmax=15, want_mask=True, want_codes=True)
    ref_mn, ref_mx = torch.zeros(rows, 9, device=DEV), torch.zeros(rows, 9, device=DEV)
    want = per_group_observe_fq(x2, run_min=ref_mn, run_max=ref_mx, **kw)
    want_gx = pg_ste_backward(g2, want["mask"], want["scale"], G)

    xs = x1.clone()
    state = torch.zeros(2, rows, 9, device=DEV)
    fwd = lambda: per_group_observe_fq(xs, run_min=state[0], run_max=state[1], **kw)   # noqa: E731
    graph, got = _captured(fwd, fwd)
    xs.copy_(x2)
    for _ in range(2):
        state.zero_()
        graph.replay()
    torch.cuda.synchronize()
    for k in ("y", "scale", "zp", "codes", "mask"):
        assert P.same_bits(got[k], want[k]), k
    assert P.same_bits(state[0], ref_mn) and P.same_bits(state[1], ref_mx)

    # the backward in a capture of its own (never autograd.backward inside a capture)
    gs, mask, scale = g1.clone(), want["mask"].clone(), want["scale"].clone()
    bwd = lambda: pg_ste_backward(gs, mask, scale, G)   # noqa: E731
    bgraph, gx = _captured(bwd, bwd)
    gs.copy_(g2)
    for _ in range(2):
        bgraph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(gx, want_gx)
