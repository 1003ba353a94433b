"""PerChannelMSEObserver without a GPU: registry and ABI, argument checks of both entry
points, the native host loop against the per-row numpy oracle (tests/pc_mse_common.py), its
fake quant against host.pc_fake_quant, one candidate against PerChannelMinMaxObserver, and the
manager's routing on CPU tensors."""
import math

import numpy as np
import pytest
import torch

import vsiquantization_amd as V
from tests.pc_mse_common import (FAMILIES, ONGRID_RATIOS, OracleState, check_against_oracle, mse_ratios, pick_seed,
                                 same_bits)
from vsiquantization_amd import _hip as H
from vsiquantization_amd import host
from vsiquantization_amd.fakequant import PerChannelFQFn, per_channel_observe_mse
from vsiquantization_amd.observers import PerChannelMinMaxObserver, PerChannelMSEObserver
from vsiquantization_amd.utils.registry import CLASS_REGISTRY

ENTRIES = ("vsiq_pc_observe_mse_f32", "vsiq_host_pc_observe_mse_f32")


# ------------------------------------------------------------------ 1. registry, ABI
def test_registry_and_construction():
    obs = CLASS_REGISTRY["PerChannelMSEObserver"](True)
    assert isinstance(obs, PerChannelMSEObserver) and isinstance(obs, PerChannelMinMaxObserver)
    assert V.PerChannelMSEObserver is PerChannelMSEObserver
    assert (obs.symmetric, obs.num_bits, obs.eps, obs.candidates, obs.min_ratio) == (True, 8, 1e-8, 64, 2 ** -8)
    assert obs.follows_bits_width and obs.ratios == mse_ratios() and obs.last_errors is None and obs.last_pick is None
    assert PerChannelMSEObserver(candidates=1).ratios == (1.0,)
    assert PerChannelMSEObserver(ratios=[1.0, 0.5]).candidates == 2
    assert (PerChannelMSEObserver(True, 2).grid(), PerChannelMSEObserver(False, 2).grid()) == ((-2, 1), (0, 3))
    with pytest.raises(ValueError):
        PerChannelMSEObserver(ratios=[0.5, 1.0])
    for bits in (2, 4, 8):
        qm = V.QuantizationManager("PerChannelUniformQuantizer", "PerChannelMSEObserver", bits, True, False)
        assert isinstance(qm.observer, PerChannelMSEObserver) and qm.observer.num_bits == bits
        assert qm.observer.grid() == (qm.quantizer.qmin, qm.quantizer.qmax)


def test_symbols_bound_and_abi_unchanged():
    lib = H.lib()
    for name in ENTRIES:
        assert name in H.EXPORTED and hasattr(lib, name)
    assert H.ABI_VERSION == 13 and lib.vsiq_abi_version() == 13


# ------------------------------------------------------------------ 2. argument checks
def test_argument_checks_without_a_launch():
    lib = H.lib()
    rows, rowlen = 2, 8
    bufs = dict(x=torch.zeros(rows, rowlen), y=torch.zeros(rows, rowlen), mn=torch.zeros(rows), mx=torch.zeros(rows),
                s=torch.zeros(rows, dtype=torch.float64), z=torch.zeros(rows, dtype=torch.float64),
                clip=torch.zeros(rows, 2, dtype=torch.float64), err=torch.zeros(rows, 128, dtype=torch.float64),
                pick=torch.zeros(rows, dtype=torch.int32), mask8=torch.zeros(rows, rowlen, dtype=torch.uint8),
                mask64=torch.zeros(8, dtype=torch.int64))
    p = {k: H.ptr(v) for k, v in bufs.items()}
    good = (H.c_d * 2)(1.0, 0.5)

    def table(vals):
        return (H.c_d * len(vals))(*vals)

    def dev(x=p["x"], y=None, codes=None, mask=None, rows=rows, rowlen=rowlen, ratios=good, count=2, mn=p["mn"],
            mx=p["mx"], s=p["s"], z=p["z"], clip=p["clip"], pick=p["pick"], qmin=-8, qmax=7):
        return lib.vsiq_pc_observe_mse_f32(x, y, codes, mask, H.c_i64(rows), H.c_i64(rowlen), ratios, count, mn, mx, s,
                                           z, clip, p["err"], pick, None, 1, qmin, qmax, 7.0, 1e-8, None)

    def hst(x=p["x"], y=None, codes=None, mask=None, rows=rows, rowlen=rowlen, ratios=good, count=2, mn=p["mn"],
            mx=p["mx"], s=p["s"], z=p["z"], clip=p["clip"], pick=p["pick"], qmin=-8, qmax=7):
        return lib.vsiq_host_pc_observe_mse_f32(x, y, mask, H.c_i64(rows), H.c_i64(rowlen), ratios, count, mn, mx, s,
                                                z, clip, p["err"], pick, None, 1, qmin, qmax, 7.0, 1e-8)

    E_ARG = -1
    for f, mask in ((dev, p["mask64"]), (hst, p["mask8"])):
        for null in ("x", "ratios", "mn", "mx", "s", "z", "clip", "pick"):
            assert f(**{null: None}) == E_ARG, null
        assert f(rows=0) == E_ARG and f(rows=-1) == E_ARG and f(rowlen=0) == E_ARG and f(rowlen=-4) == E_ARG
        assert f(mask=mask) == E_ARG                      # a mask without y
        for count in (0, -1, 129, 1 << 20):
            assert f(ratios=table([1.0] * 130), count=count) == E_ARG, count
        for bad in ([0.5, 1.0], [1.0, 0.0], [1.0, -0.5], [1.0, 1.5], [1.0, float("nan")], [float("nan"), 0.5]):
            assert f(ratios=table(bad)) == E_ARG, bad
        assert f(qmin=7, qmax=7) == E_ARG and f(qmin=8, qmax=7) == E_ARG
    assert dev(codes=p["mask8"]) == E_ARG                 # codes without y
    assert not bufs["err"].any() and not bufs["s"].any() and not bufs["pick"].any()
    assert hst() == 0 and bufs["pick"].tolist() == [0, 0] and math.isinf(float(bufs["err"].reshape(-1)[0]))


def test_python_validates_ratios_and_grid():
    x = torch.randn(4, 9)
    for bad in ([0.5, 1.0], [1.0, 0.0], [], [1.0] * 129):
        with pytest.raises(ValueError):
            per_channel_observe_mse(x, symmetric=True, qmin=-8, qmax=7, ratios=bad)
    with pytest.raises(ValueError):
        per_channel_observe_mse(x, symmetric=True, qmin=3, qmax=3, ratios=[1.0, 0.5])


# ------------------------------------------------------------------ 3. host loop == oracle
MIXED = FAMILIES + FAMILIES[::-1]
TABLES = {"default": mse_ratios(), "denormal": mse_ratios(64, 2.0 ** -24), "ongrid": ONGRID_RATIOS}


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_host_loop_equals_oracle_row_by_row(table, symmetric):
    ratios = TABLES[table]
    for bits in (2, 4, 8):
        qmin, qmax = (-(2 ** (bits - 1)), 2 ** (bits - 1) - 1) if symmetric else (0, 2 ** bits - 1)
        for rowlen in (1, 3, 9, 27, 257):
            state = OracleState(len(MIXED), symmetric, bits)
            mn, mx = torch.zeros(len(MIXED)), torch.zeros(len(MIXED))
            seed = 1
            for _ in range(2):   # two successive calls on one running state
                seed, x, rows = pick_seed(MIXED, rowlen, ratios, symmetric, bits, start=seed)
                seed += 1
                r = per_channel_observe_mse(x, symmetric=symmetric, qmin=qmin, qmax=qmax, num_bits=bits, run_min=mn,
                                            run_max=mx, ratios=ratios, want_mask=True, want_row_stats=True)
                state.update(rows)
                check_against_oracle(r, rows, state, (table, symmetric, bits, rowlen, seed))
                y, mask = host.pc_fake_quant(x, r["scale"], r["zp"], qmin, qmax, want_mask=True)
                assert same_bits(r["y"], y) and same_bits(r["mask"], mask)
                ref = host.pc_observe_fq(x, symmetric=symmetric, qmin=qmin, qmax=qmax, quantize=False,
                                         want_row_stats=True)
                assert same_bits(r["row_stats"], ref["row_stats"])


def test_fallback_is_per_row():
    """constant / nan / inf rows are PerChannelMinMaxObserver's; their neighbours still search."""
    torch.manual_seed(0)
    x = torch.stack([torch.full((64,), 2.5), torch.randn(64) * 3, torch.randn(64) * 3, torch.randn(64) * 3])
    x[1, 5] = float("nan")
    x[2, 7] = float("inf")
    r = per_channel_observe_mse(x, symmetric=True, qmin=-8, qmax=7, num_bits=4, ratios=mse_ratios(), quantize=False)
    m = host.pc_observe_fq(x, symmetric=True, qmin=-8, qmax=7, obs_bits=4, quantize=False)
    err = r["err"]
    assert all(torch.isinf(err[c]).all() and int(r["pick"][c]) == 0 for c in (0, 1, 2))
    assert torch.isfinite(err[3]).all() and int(r["pick"][3]) > 0
    for c in (0, 1, 2):
        assert same_bits(r["scale"][c], m["scale"][c]) and same_bits(r["run_max"][c], m["run_max"][c])
    assert float(r["run_max"][3]) < float(m["run_max"][3])


# ------------------------------------------------------------------ 4. one candidate == min / max
@pytest.mark.parametrize("symmetric", [True, False])
def test_one_candidate_is_per_channel_minmax(symmetric):
    p = V.QuantizationManager("PerChannelUniformQuantizer", "PerChannelMSEObserver", 4, symmetric, False)
    m = V.QuantizationManager("PerChannelUniformQuantizer", "PerChannelMinMaxObserver", 4, symmetric, False)
    p.observer.ratios = mse_ratios(1)
    m.observer.num_bits = 4   # the same observer width on both sides
    for seed in (1, 2):       # two successive calls on one running state
        x = torch.stack([torch.randn(27, generator=torch.Generator().manual_seed(seed + c)) * (c + 1)
                         for c in range(6)])
        x[2] = 1.5
        x[3, 4] = float("nan")
        yp, ym = p.quantize(x), m.quantize(x)
        assert same_bits(yp, ym)
        assert same_bits(p.scale, m.scale) and same_bits(p.zero_point, m.zero_point)
        assert same_bits(p.observer.run_min, m.observer.run_min) and same_bits(p.observer.run_max, m.observer.run_max)
        assert not p.observer.last_pick.any() and torch.isinf(p.observer.last_errors).all()
    for name in ("mean_abs_x", "mean_x", "std"):
        assert same_bits(np.array(getattr(p, name)), np.array(getattr(m, name)))


# ------------------------------------------------------------------ 5. manager, autograd, state
def test_manager_routes_and_observer_state():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(8, 64, 3, 3, generator=g)
    w[:, 0, 0, 0] = 8.0   # one outlier per out-channel: a heavy-tailed weight
    qm = V.QuantizationManager("PerChannelUniformQuantizer", "PerChannelMSEObserver", 4, True, False)
    mm = V.QuantizationManager("PerChannelUniformQuantizer", "PerChannelMinMaxObserver", 4, True, False)
    for q in (qm, mm):
        q.is_quantize = False
        q.collect_qparameter(w)
    obs = qm.observer
    assert obs.last_errors.shape == (8, 64) and obs.last_pick.shape == (8,) and bool((obs.last_pick > 0).all())
    assert bool((obs.max_val < mm.observer.max_val).all())
    assert len(qm.mean_abs_x) == 1 and qm.mean_abs_x == mm.mean_abs_x and qm.std == mm.std
    qm.is_quantize = True
    wg = w.clone().requires_grad_(True)
    y = qm.quantize(wg)
    y.backward(torch.ones_like(y))
    s, z = qm.observer.get_scale_zero_point()
    ref = w.clone().requires_grad_(True)
    yr = PerChannelFQFn.apply(ref, s, z, qm.quantizer.qmin, qm.quantizer.qmax)
    yr.backward(torch.ones_like(yr))
    assert same_bits(y, yr) and same_bits(wg.grad, ref.grad)
    import copy
    import pickle
    clone = copy.deepcopy(obs)
    assert same_bits(clone.run_min, obs.run_min) and clone.run_min is not obs.run_min and clone.ratios == obs.ratios
    assert pickle.loads(pickle.dumps(obs)).candidates == 64
    obs.reset()
    assert obs.run_min is None and obs.last_errors is None
    with pytest.raises(RuntimeError, match="PerChannelMSEObserver"):
        obs.get_scale_zero_point()
