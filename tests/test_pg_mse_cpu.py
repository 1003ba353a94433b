"""PerGroupMSEObserver without a GPU: the host loop against tests/pg_mse_common.py's oracle, and the arguments."""
import pytest
import torch

import vsiquantization_amd as V
from tests import pg_mse_common as M
from vsiquantization_amd import _hip as H
from vsiquantization_amd import host
from vsiquantization_amd.fakequant import per_group_observe_fq, per_group_observe_mse
from vsiquantization_amd.observers import PerGroupMinMaxObserver

RATIOS = M.mse_ratios()
_run = M.run


@pytest.mark.parametrize("symmetric,bits", M.GRIDS)
@pytest.mark.parametrize("G", M.GROUPS)
def test_host_loop_equals_oracle_on_ragged_rows_over_two_calls(G, symmetric, bits):
    qmin, qmax = M.grid_of(bits, symmetric)
    for rowlen in (1, 27, 33, 100, 257):
        ngr = -(-rowlen // G)
        state = M.OracleState(3 * ngr, symmetric, bits)
        mn, mx = torch.zeros(3, ngr), torch.zeros(3, ngr)
        seed = 1
        for _ in range(2):   # two successive calls on one running state
            seed, x, groups = M.case(("gauss", "heavy", "relu"), rowlen, G, RATIOS, symmetric, bits, seed)
            seed += 1
            r = _run(x, G, symmetric, bits, run_min=mn, run_max=mx, want_mask=True)
            state.update(groups)
            M.check_against_oracle(M.flat(r), groups, state, (G, symmetric, bits, rowlen, seed))
            y, mask = host.pg_fake_quant(x, r["scale"], r["zp"], G, qmin, qmax, want_mask=True)
            assert M.same_bits(r["y"], y) and torch.equal(r["mask"], mask) and r["run_min"] is mn


@pytest.mark.parametrize("symmetric,bits", M.GRIDS)
@pytest.mark.parametrize("G", M.GROUPS)
def test_host_loop_equals_oracle_on_mixed_families_as_adjacent_groups(G, symmetric, bits):
    """constant / nan / inf groups are PerGroupMinMaxObserver's, their neighbours still search."""
    _, x, groups = M.case("mixed", 0, G, RATIOS, symmetric, bits)
    r = _run(x, G, symmetric, bits)
    state = M.OracleState(len(groups), symmetric, bits)
    state.update(groups)
    M.check_against_oracle(M.flat(r), groups, state, (G, symmetric, bits))
    fell = [i for i, f in enumerate(M.MIXED[:8]) if f in ("constant", "nan", "inf")]   # in row 0
    assert not r["pick"][0, fell].any() and torch.isinf(r["err"][0, fell]).all() and bool(r["pick"].any())
    assert _run(x, G, symmetric, bits, quantize=False, want_errors=False)["err"] is None


@pytest.mark.parametrize("symmetric,bits", M.GRIDS)
def test_one_candidate_is_per_group_observe_fq(symmetric, bits):
    qmin, qmax = M.grid_of(bits, symmetric)
    _, x, _ = M.case("mixed", 0, 64, RATIOS, symmetric, bits)
    a = _run(x, 64, symmetric, bits, ratios=(1.0,), want_mask=True)
    b = per_group_observe_fq(x, group_size=64, symmetric=symmetric, qmin=qmin, qmax=qmax, obs_bits=bits, want_mask=True)
    assert all(M.same_bits(a[k], b[k]) for k in ("y", "scale", "zp", "run_min", "run_max", "mask"))
    assert not a["pick"].any() and torch.isinf(a["err"]).all()


def test_registry_abi_and_bad_arguments():
    obs = V.CLASS_REGISTRY["PerGroupMSEObserver"](True)
    assert isinstance(obs, V.PerGroupMSEObserver) and isinstance(obs, PerGroupMinMaxObserver) and not obs.want_errors
    assert (obs.candidates, obs.min_ratio, obs.ratios, obs.last_pick, obs.last_errors) == (64, 2 ** -8, RATIOS, None, None)
    qm = V.QuantizationManager("PerGroupLSQQuantizer", "PerGroupMSEObserver", 4, True, False)
    assert qm.observer.num_bits == 4 and qm.observer.grid() == (qm.quantizer.qmin, qm.quantizer.qmax)
    lib = H.lib()
    assert all(n in H.EXPORTED and hasattr(lib, n) for n in ("vsiq_pg_observe_mse_f32", "vsiq_host_pg_observe_mse_f32"))
    assert H.ABI_VERSION == 13 and lib.vsiq_abi_version() == 13
    x = torch.randn(2, 40)
    kw = dict(group_size=32, symmetric=True, qmin=-8, qmax=7, ratios=RATIOS)
    for bad in (dict(group_size=48), dict(ratios=[0.5, 1.0]), dict(ratios=[1.0] * 129), dict(qmin=3, qmax=3),
                dict(run_min=torch.zeros(2, 3))):   # the last: the state of another group count
        with pytest.raises(ValueError):
            per_group_observe_mse(x, **{**kw, **bad})
    with pytest.raises(TypeError, match="float16"):
        per_group_observe_mse(x.half(), **kw)
    with pytest.raises(NotImplementedError):
        per_group_observe_mse(x, want_codes=True, **kw)
    bufs = [x] + [torch.zeros(8, dtype=d) for d in (torch.float32,) * 2 + (torch.float64,) * 3 + (torch.int32,)]
    b = [H.ptr(x), None, None, H.c_i64(2), H.c_i64(40), H.c_i64(32), (H.c_d * 2)(1.0, 0.5), 2] + \
        [H.ptr(v) for v in bufs[1:6]] + [None, H.ptr(bufs[6]), 1, -8, 7, 7.0, 1e-8]
    call = lib.vsiq_host_pg_observe_mse_f32
    assert call(*b) == 0 and call(*b[:3], H.c_i64(0), *b[4:]) == 0   # err_out is nullable; rows == 0 returns 0
    for i, v in ((0, None), (5, H.c_i64(48)), (6, None), (7, 0), (7, 129), (12, None), (14, None), (4, H.c_i64(0)),
                 (3, H.c_i64(-1)), (16, 7)):
        assert call(*b[:i], v, *b[i + 1:]) == -1, i
