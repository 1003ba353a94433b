"""PerGroupMSEObserver on MI355X (csrc/k_pg_mse.hip) against the host loop and tests/pg_mse_common.py's oracle."""
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests import pg_common as P
from tests import pg_mse_common as M
from vsiquantization_amd.fakequant import per_group_fake_quant, per_group_observe_mse
from vsiquantization_amd.modules.fused import LinearBnReLU
from vsiquantization_amd.utils.quantize_manager import activate_learning_qparam

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = M.mse_ratios()
FAMS = ("gauss", "heavy", "relu", "gauss", "heavy")
OUT = dict(want_mask=True, want_codes=True)
_run = M.run


def _check(x, groups, G, symmetric, bits, tag, ratios=RATIOS, xd=None):
    """Device == oracle (E within REL, the rest bit for bit) == host loop; y / mask / codes are
    per_group_fake_quant's; a repeated call repeats the bits; asking for the errors changes nothing else."""
    xd = x.to(DEV) if xd is None else xd
    qmin, qmax = M.grid_of(bits, symmetric)
    got = _run(xd, G, symmetric, bits, ratios, **OUT)
    state = M.OracleState(len(groups), symmetric, bits)
    state.update(groups)
    M.check_against_oracle(M.flat(got), groups, state, tag)
    host = _run(x, G, symmetric, bits, ratios, want_mask=True)
    assert M.same_but_errors(got, host, ("y",)), tag
    assert torch.equal(P.unpack_mask(got["mask"], *x.shape), P.unpack_mask(host["mask"], *x.shape)), tag
    y, mask, codes = per_group_fake_quant(xd, got["scale"], got["zp"], qmin, qmax, group_size=G, **OUT)
    assert M.same_bits(y, got["y"]) and torch.equal(mask, got["mask"]) and torch.equal(codes, got["codes"]), tag
    again, bare = _run(xd, G, symmetric, bits, ratios, **OUT), _run(xd, G, symmetric, bits, ratios, False, **OUT)
    assert M.same_but_errors(again, got, ("err", "y", "mask", "codes")) and bare["err"] is None and \
        M.same_but_errors(bare, got, ("y", "mask", "codes")), tag
    return got


@pytest.mark.parametrize("rows", [1, 3, 5])   # 5: more than a workgroup's waves
@pytest.mark.parametrize("rowlen", [1, 27, 32, 33, 100, 256, 257, 260, 516])
@pytest.mark.parametrize("G", M.GROUPS)
def test_device_equals_host_loop_equals_oracle(G, rowlen, rows):
    symmetric, bits = M.GRIDS[(rowlen + rows) % 3]
    _, x, groups = M.case(FAMS[:rows], rowlen, G, RATIOS, symmetric, bits)
    _check(x, groups, G, symmetric, bits, (G, rowlen, rows))


@pytest.mark.parametrize("symmetric,bits", M.GRIDS)
@pytest.mark.parametrize("G", M.GROUPS)
def test_mixed_families_in_the_groups_of_one_wave(G, symmetric, bits):
    _, x, groups = M.case("mixed", 0, G, RATIOS, symmetric, bits)
    got = _check(x, groups, G, symmetric, bits, ("mixed", G, symmetric, bits))
    assert bool(got["pick"].any()) and bool(torch.isinf(got["err"][0, 3]).all())   # "constant" fell back


@pytest.mark.parametrize("count", [1, 2, 64, 128, "ongrid"])   # no search, a partial batch, 1 and 2 passes, exact ties
def test_candidate_counts_and_exact_ties(count):
    if count == "ongrid":
        ratios, fams, grid = M.ONGRID_RATIOS, ("ongrid",) * 3, (False, 8)
    else:
        ratios, fams, grid = M.mse_ratios(count), FAMS[:3], (True, 4)
    _, x, groups = M.case(fams, 100, 32, ratios, *grid)
    _check(x, groups, 32, *grid, ("count", count), ratios=ratios)


def test_view_offset_by_one_element_and_two_calls_carrying_state():
    _, a, ga = M.case(FAMS, 96, 32, RATIOS, False, 4)
    buf = torch.empty(a.numel() + 1, dtype=torch.float32, device=DEV)   # a view one element into a buffer
    xd = buf[1:].view(a.shape)
    xd.copy_(a)
    _check(a, ga, 32, False, 4, "offset", xd=xd)
    b = M.case(FAMS, 96, 32, RATIOS, False, 4, 20)[1] * 2   # (a power of two: as decidable as the case)
    state = M.OracleState(len(ga), False, 4)
    mn, mx = torch.zeros(5, 3, device=DEV), torch.zeros(5, 3, device=DEV)
    for x, groups in ((a, ga), (b, M.oracle_groups(b, 32, RATIOS, False, 4))):
        r = _run(x.to(DEV), 32, False, 4, run_min=mn, run_max=mx)
        state.update(groups)
        M.check_against_oracle(M.flat(r), groups, state, "state")


@pytest.mark.parametrize("rowlen", [256, 258])   # the vector and the per-element path
def test_every_output_arm(rowlen):
    xd = M.case(FAMS[:2], rowlen, 64, RATIOS, True, 4)[1].to(DEV)
    full = _run(xd, 64, True, 4, **OUT)
    for kw in (dict(quantize=False), dict(), dict(want_mask=True), dict(want_codes=True)):
        r = _run(xd, 64, True, 4, **kw)
        assert M.same_but_errors(r, full, ("err",) + tuple(k for k in ("y", "mask", "codes") if r[k] is not None)), kw
        assert (r["y"] is None) == ("quantize" in kw) and (r["mask"] is None) == ("want_mask" not in kw)


def test_manager_with_both_group_quantizers_and_the_lsq_step():
    torch.manual_seed(1)
    w = torch.randn(5, 200, device=DEV)
    w[:, ::37] *= 8.0   # a heavy weight: outliers in most groups
    sums = {}
    for name in ("PerGroupMSEObserver", "PerGroupMinMaxObserver"):   # fresh states, 4-bit symmetric, g64
        qm = V.QuantizationManager("PerGroupUniformQuantizer", name, 4, True, False)
        qm.quantizer.group_size = 64
        d = (qm.quantize(w).double() - w.double()) ** 2
        sums[name] = nn.functional.pad(d, (0, 56)).reshape(5, 4, 64).sum(-1)
    a, b = sums["PerGroupMSEObserver"], sums["PerGroupMinMaxObserver"]
    assert bool((a <= b).all()) and bool((a < b).any())
    layer = LinearBnReLU(nn.Linear(200, 5), nn.BatchNorm1d(5), nn.ReLU(), "PerGroupMSEObserver", "PerGroupLSQQuantizer",
                         "MinMaxObserver", "UniformQuantizer", True, True, True, 4, 8).to(DEV)
    layer.weight_quantizer.quantizer.group_size = 64
    with torch.no_grad():
        layer.linear_fuse.weight[:, ::37] *= 8.0
    for q in (layer.weight_quantizer, layer.activation_quantizer):
        q.is_learning_scale = False
    x = torch.randn(3, 200, device=DEV)
    layer(x)                                              # calibration
    wq = layer.weight_quantizer
    assert isinstance(wq.observer, V.PerGroupMSEObserver) and bool((wq.observer.last_pick > 0).any())
    assert wq.observer.last_errors is None and wq.observer.num_bits == 4 and wq.scale.shape == (5, 4)
    model = nn.Sequential(layer)
    activate_learning_qparam(model)
    before = wq.scale.detach().clone()
    model(x).square().mean().backward()
    torch.optim.SGD(model.parameters(), lr=1e-2).step()
    assert bool(torch.isfinite(wq.scale.grad).all()) and bool((wq.scale.detach() != before).any())
    with pytest.raises(TypeError, match="float16"):
        per_group_observe_mse(w.half(), group_size=64, symmetric=True, qmin=-8, qmax=7, ratios=RATIOS)


def test_graph_replay_equals_eager():
    rows, rowlen, G = 9, 576, 64
    x1, x2 = (P.weights(rows, rowlen, 1) * 60).to(DEV), (P.weights(rows, rowlen, 20) * 90).to(DEV)
    kw = dict(group_size=G, symmetric=False, qmin=0, qmax=15, num_bits=4, ratios=RATIOS, want_errors=True, **OUT)
    ref = torch.zeros(2, rows, 9, device=DEV)
    want = per_group_observe_mse(x2, run_min=ref[0], run_max=ref[1], **kw)
    xs, state = x1.clone(), torch.zeros(2, rows, 9, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = per_group_observe_mse(xs, run_min=state[0], run_max=state[1], **kw)
    xs.copy_(x2)
    for _ in range(2):
        state.zero_()
        graph.replay()
    torch.cuda.synchronize()
    assert M.same_but_errors(got, want, ("err", "y", "mask", "codes")) and bool(want["pick"].any())
    assert M.same_bits(state, ref)
