"""The learnable backward at non-finite, tie and clamp-edge inputs, without a GPU:
the oracle against the reference fixtures of those inputs (tests/golden/gen_goldens.py
section 10), and the native host loops (vsiq_host_lsq_bwd_f32, vsiq_host_pc_lsq_bwd_f32 /
vsiq_host_pcm_lsq_bwd_f32 through vsiquantization_amd/host.py) against the oracle.
tests/lsq_edges_common.py holds the inputs and the comparison; tests/test_gpu_lsq_edges.py
runs the same inputs through every device form."""
import numpy as np
import pytest
import torch

from vsiquantization_amd import _hip as H
from vsiquantization_amd import fakequant as FQ
from vsiquantization_amd import host
from oracle import fakequant_np as O
from tests import goldens as G
from tests import lsq_edges_common as EC

SILU = H.SiluAct(*O.SILU_REF_DEFAULT)   # the host layout the oracle's SiLU names
SHORT, LONG = 203, 70001                # below the host loops' SIMD / chunk sizes, and two chunks


def t(a, grad=False):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.requires_grad_(True) if grad else x


def qcase_of(case):
    return EC.QCase(case["qcase"], case["sym"], case["bits"], case["learn_zp"], float(case["scale"]), case["zp"])


# --------------------------------------------------------------------------- oracle == fixtures
@pytest.mark.parametrize("case", G.cases("learnable_fq_edges"), ids=lambda c: f"{c['key']}-{c['qcase']}-{c['variant']}")
def test_oracle_equals_reference_learnable_edges(case):
    qc = qcase_of(case)
    x, g = G.arr(case["x"]), G.arr(case["g"])
    bx, bg = EC.build_inputs(qc, case["variant"], x.size, seed=1000 + int(case["key"][4:]))
    G.assert_bitwise_f32(bx, x, "the builder gives the fixture's x")
    G.assert_bitwise_f32(bg, g, "the builder gives the fixture's g")
    exp = EC.oracle(x, g, qc, O.grad_scale(EC.qrange(qc)[1], x.size))
    EC.check_golden(exp.y, exp.gx, exp.gs, exp.gz if qc.learn_zp else None, case, case["key"])


def test_reference_edge_fixtures_cover_every_class():
    """What the fixtures pin: every planted variant, finite gradients (values) and NaN,
    +inf and -inf ones (classes), and the reference's NaN zero-point gradient for an
    in-range NaN or inf incoming gradient."""
    cs = G.cases("learnable_fq_edges")
    assert {c["variant"] for c in cs} == set(EC.VARIANTS)
    assert {c["qcase"] for c in cs} == {q.name for q in EC.QCASES}
    classes = {EC.grad_class(float(c[k])) for c in cs for k in ("scale_grad", "zp_grad") if k in c}
    assert classes == {"nan", "+inf", "-inf", "finite"}
    for variant in ("g_nan_in_range", "g_inf_in_range"):
        zs = [float(c["zp_grad"]) for c in cs if c["variant"] == variant and c["learn_zp"] == 1
              and 0 <= round(c["zp"]) <= 15 and float(c["scale"]) > 0]
        assert zs and all(np.isnan(z) for z in zs), (variant, zs)


@pytest.mark.parametrize("case", G.cases("per_channel_learnable_edges"), ids=lambda c: c["key"])
def test_oracle_equals_reference_per_channel_edges(case):
    w, g = G.arr(case["x"]), G.arr(case["g"])
    sym = case["sym"]
    qmin, qmax = O.qrange(case["bits"], sym)
    exp = EC.pc_oracle(w, g, G.arr(case["scale"]), G.arr(case["zp"]), qmin, qmax,
                       O.grad_scale(qmax, w[0].size), 0, not sym)
    EC.check_golden(exp.y, exp.gx, exp.gs, None if sym else exp.gz, case, case["key"])
    assert np.isnan(exp.gs[1]) and (sym or np.isnan(exp.gz[1]))        # the NaN-gradient channel
    assert np.isfinite(np.delete(exp.gs, 1)).all()                      # stays in its channel


def _lsqm_edge_case():
    (case,) = [c for c in G.cases("lsq_fake_quantize") if c.get("edges")]
    return case


def test_oracle_equals_reference_lsq_fake_quantize_edges():
    case = _lsqm_edge_case()
    x, g = G.arr(case["x"]), G.arr(case["g"])
    s, z = G.arr(case["scale"]).reshape(-1), G.arr(case["zp"]).reshape(-1)
    gsc = O.lsq_module_grad_scale(x.shape, case["qmax"], True, case["config_act"])
    exp = EC.pc_oracle(x, g, s, z, case["qmin"], case["qmax"], gsc, 1, True)
    EC.check_golden(exp.y, exp.gx, exp.gs, exp.gz, case, case["key"])
    assert np.isnan(exp.gz[1]) and np.isnan(exp.gs[1]) and np.isnan(exp.gs[4])
    assert np.isfinite(exp.gz[[0, 2, 3, 4, 5]]).all()


# --------------------------------------------------------------------------- host loops == oracle
def host_run(x, g, qc, gscale, act):
    qmin, qmax = EC.qrange(qc)
    s = torch.tensor(float(qc.scale), dtype=torch.float64, requires_grad=True)
    z = torch.tensor(float(qc.zp), dtype=torch.float64, requires_grad=True) if qc.learn_zp else 0.0
    xg = t(x, grad=True)
    assert host.is_host(xg)
    y = FQ.fake_quant_learn(xg, s, z, qmin, qmax, gscale, qc.learn_zp, act)
    y.backward(t(g))
    return (y.detach().numpy(), xg.grad.numpy(), float(s.grad), float(z.grad) if qc.learn_zp else 0.0)


@pytest.mark.parametrize("qc", EC.QCASES, ids=lambda q: q.name)
def test_host_loop_equals_oracle(qc):
    """vsiq_host_lsq_bwd_f32 on every variant: plain and fused ReLU at both lengths, fused
    SiLU at the short one."""
    gscale = 0.37
    for vi, variant in enumerate(EC.VARIANTS):
        for n, acts in ((SHORT, (None, "relu", SILU)), (LONG, (None, "relu"))):
            x, g = EC.build_inputs(qc, variant, n, seed=7 * vi + n % 5)
            for act in acts:
                exp = EC.oracle(x, g, qc, gscale, act)
                y, gx, gs, gz = host_run(x, g, qc, gscale, act)
                EC.check(y, gx, gs, gz, exp, f"{qc.name} {variant} n={n} act={act}", zp_grad=bool(qc.learn_zp))


@pytest.mark.parametrize("shape,axis", [((6, 5, 3, 3), 0), ((4, LONG), 0), ((3, 7, 4), 1), ((2, 4, LONG), 1)])
@pytest.mark.parametrize("learn_zp", [False, True])
def test_host_per_channel_loops_equal_oracle(shape, axis, learn_zp):
    """vsiq_host_pc_lsq_bwd_f32 / vsiq_host_pcm_lsq_bwd_f32 (PerChannelLearnFn on CPU, axis 0 / 1) with
    the three special channels, rows below and above the host loops' chunk."""
    sym = not learn_zp
    qmin, qmax = O.qrange(4, sym)
    x, g, s, z = EC.pc_build(shape, axis, sym, 4, seed=sum(shape) + axis, learn_zp=learn_zp)
    gscale = (qmax * x.size / shape[axis]) ** -0.5
    exp = EC.pc_oracle(x, g, s, z, qmin, qmax, gscale, axis, learn_zp)
    sp, zp = t(s, grad=True), t(z, grad=learn_zp)
    xg = t(x, grad=True)
    y = FQ.PerChannelLearnFn.apply(xg, sp, zp, qmin, qmax, gscale, learn_zp, axis)
    y.backward(t(g))
    EC.check(y.detach().numpy(), xg.grad.numpy(), sp.grad.numpy(), zp.grad.numpy() if learn_zp else None, exp,
             f"{shape} axis {axis}", zp_grad=learn_zp)
    assert np.isnan(exp.gs[1]) and np.isfinite(np.delete(exp.gs, 1)).all()
    if learn_zp:
        assert np.isnan(exp.gz[1]) and np.isfinite(np.delete(exp.gz, 1)).all()


def test_host_lsq_fake_quantize_edge_fixture():
    """The new LSQFakeQuantize fixture through the host path (axis 1)."""
    case = _lsqm_edge_case()
    x, g = G.arr(case["x"]), G.arr(case["g"])
    sp, zp = t(G.arr(case["scale"]).copy(), grad=True), t(G.arr(case["zp"]).copy(), grad=True)
    gsc = O.lsq_module_grad_scale(x.shape, case["qmax"], True, case["config_act"])
    xg = t(x, grad=True)
    y = FQ.PerChannelLearnFn.apply(xg, sp, zp, case["qmin"], case["qmax"], gsc, True, 1)
    y.backward(t(g))
    EC.check_golden(y.detach().numpy(), xg.grad.numpy(), sp.grad.numpy(), zp.grad.numpy(), case, case["key"])
