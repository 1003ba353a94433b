"""Every arm of the launch dispatch of the kernels merged after tests/test_gpu_dispatch.py, once,
through the public entry points (MI355X only): the MSE and percentile observers, the
per-channel MSE observer, pack / unpack, AdaRound, the multi-tensor LSQ launch and the 16-bit
kernels -- and the fixed-qparam per-channel forward, which the older file never ran with the
knob off.

Their own suites never set the non-temporal knob, so each of them runs one (VEC, NT) pair per
shape.  Each test here crosses the knob (NT) with the layouts for one entry point, at the
smallest shape that selects the arm (thresholds read from the launch code's constants), and
compares with the references and bars of that kernel's own suite -- never with the device's
other arm alone: the library's host entry points (vsiq_host_*, pinned by the CPU suite) and
the numpy restatements of tests/{mse,percentile,pc_mse,pack,adaround}_common.py and
oracle/fakequant_np.py.  y / codes / packed bytes / masks / grad_x / grad_V (lambda = 0) bit
for bit, min / max / qparams / clips / picks exact, every E_k and R <= 1e-9 relative, grad_V
(lambda != 0) <= 1 fp32 ulp, scale / zero-point gradients <= 1e-9.

Layouts: "vec" = row length % 4 == 0 on a 16-byte-aligned tensor; "tail" = row length % 4 != 0;
"offset" = the vec shape on a view one element into the allocation.  The two observers take
their NT arm only from 256 MB (kObsTemporalMB) with the knob on: their tests share one tensor
of 2^26 + 4 elements (n % 4 == 0, a ragged last grid-stride step), the only large one here.
The knob is process-global: it is set only inside ``with tuned(...)``.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import fakequant_np as O
from tests import adaround_common as A
from tests import goldens as G
from tests import mse_common as M
from tests import pack_common as P
from tests import pc_mse_common as PC
from tests import test_gpu_half as TH
from tests import test_gpu_multi as TM
from tests.percentile_common import tail_of
from tests.test_gpu_percentile import _host_hist
from tests.tuning_common import tuned
from vsiquantization_amd import _hip as H
from vsiquantization_amd import fakequant as FQ
from vsiquantization_amd import host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACTS = (None, "relu", "silu")
NTS = (1, 0)


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    H.lib()
    yield
    _big.clear()
    _host.clear()


def _const(text, name):
    return int(re.search(r"constexpr (?:int|int64_t) %s = (\d+);" % name, text).group(1))


def _src(name):
    return open(os.path.join(PC.CSRC, name)).read()


# --------------------------------------------------------------------------- 1. the two observers' NT arm
BIG_N = (1 << 26) + 4
BIG_SEED = 26
_big = {}
_host = {}


def _obs_sizes():
    """(NT threshold in MB, groups of one workgroup step, grid limit), read from the source."""
    common, k2 = _src("vsiq_common.cuh"), _src("k_observe_k2.cuh")
    mb = _const(common + k2, "kObsTemporalMB")
    grid = _const(common + k2, "kObsGrid")
    return mb, _const(common, "kBlock") * _const(common, "kObsU"), grid


def big():
    """(CPU tensor, device tensor) of BIG_N gauss elements, made once."""
    if not _big:
        xc = M.make_input("gauss", BIG_N, BIG_SEED)
        _big["x"] = (xc, xc.to(DEV))
    return _big["x"]


def host_once(key, fn):
    if key not in _host:
        _host[key] = fn()
    return _host[key]


def test_big_tensor_selects_the_nt_arm_with_a_ragged_last_step():
    """The facts the size is chosen for, from the launch code's constants."""
    mb, step, grid = _obs_sizes()
    for f in ("k_observe_mse.hip", "k_observe_hist.hip"):
        assert "g_tune.nontemporal != 0 && !((n * (int64_t)sizeof(float)) >> 20 < kObsTemporalMB)" in _src(f)
    assert (BIG_N * 4) >> 20 >= mb and ((BIG_N - 4) * 4) >> 20 >= mb   # NT with the knob on
    assert BIG_N % 4 == 0                                              # VEC
    ng = BIG_N // 4
    assert ng > grid * step and ng % step != 0                         # the full grid; the last step is ragged


def _counter_words():
    return int(H.workspace(torch.device(DEV)).counter.ne(0).sum())


def _stats_words():
    w = H.workspace(torch.device(DEV))
    return int(w.histogram().ne(0).sum()) + int(w.counter.ne(0).sum())


MSE_KW = dict(symmetric=False, num_bits=4, qmin=0, qmax=15)


def _mse_device(act, ratios, nt):
    state = torch.zeros(2, dtype=torch.float32, device=DEV)
    with tuned(NONTEMPORAL=nt):
        r = FQ.observe_mse(big()[1], run_minmax=state, ratios=ratios, act=act, **MSE_KW)
    torch.cuda.synchronize()
    assert _counter_words() == 0, (act, nt)
    return list(r) + [state]


def _same_all(a, b, skip=1):
    """Two result lists bit for bit, but for entry ``skip``: the stats record, which is K2's output
    (its own NT arm: test_gpu_dispatch.py::test_observe_nontemporal), not the second pass's."""
    assert len(a) == len(b)
    return all(M.same_bits(p, q) for i, (p, q) in enumerate(zip(a, b)) if i != skip)


@pytest.mark.parametrize("act", ACTS)
def test_mse_observer_nt_arm_equals_host(act):
    """k_observe_mse<1, 1, ACT>: ld4<true> in the whole steps, load_group_c<true, true> in the ragged last
    one.  Two candidates (the smallest count that reads x) against the host loop on the CPU copy."""
    ratios = FQ.mse_ratios(2)

    def host():
        state = torch.zeros(2, dtype=torch.float32)
        return list(FQ.observe_mse(big()[0], run_minmax=state, ratios=ratios, act=act, **MSE_KW)) + [state]
    hqp, hst, hclip, herr, hpick, hstate = host_once(("mse", act), host)
    qp, st, clip, err, pick, state = _mse_device(act, ratios, 1)
    E = [float(e) for e in herr]
    print("mse big", act, "pick", int(pick), int(hpick), "E", err.tolist(), E, "margin", M.margin(E))
    assert M.decidable(E), (act, M.margin(E))
    assert M.errors_close(err, E), act
    assert int(pick) == int(hpick), act
    for k in (H.ST_MIN, H.ST_MAX, H.ST_NAN, H.ST_N):
        assert float(st[k]) == float(hst[k]), (act, k)
    assert M.same_bits(clip, hclip) and M.same_bits(qp, hqp) and M.same_bits(state, hstate), act


def test_mse_observer_nt_arm_all_candidates():
    """The default 64-candidate table: every sum, the pick, the clip and the qparams of the NT arm are
    the cached arm's bit for bit (the summation order is fixed and does not depend on NT)."""
    on = _mse_device(None, FQ.mse_ratios(), 1)
    off = _mse_device(None, FQ.mse_ratios(), 0)
    assert on[3].numel() == 64 and bool(torch.isfinite(on[3]).all()) and 0 < int(on[4]) < 63
    assert _same_all(on, off)


@pytest.mark.parametrize("act", ACTS)
def test_mse_observer_cached_arm_at_the_full_grid(act):
    """k_observe_mse<1, 0, ACT> on the same tensor (512 workgroups, ragged last step): the NT arm's
    result, which test_mse_observer_nt_arm_equals_host holds to the host's."""
    assert _same_all(_mse_device(act, FQ.mse_ratios(2), 1), _mse_device(act, FQ.mse_ratios(2), 0))


PCT_KW = dict(symmetric=False)


def _pct_device(act, bins, pct, nt):
    out = []
    with tuned(NONTEMPORAL=nt):
        for _ in range(2):   # the second, stream-ordered call finds the histogram and the counter zeroed
            state = torch.zeros(2, dtype=torch.float32, device=DEV)
            r = FQ.observe_percentile(big()[1], run_minmax=state, tail=tail_of(pct), bins=bins, act=act, **PCT_KW)
            out.append(list(r) + [state])
    torch.cuda.synchronize()
    assert _stats_words() == 0, (act, bins, nt)
    assert _same_all(out[0], out[1]), (act, bins, nt)
    return out[0]


def _pct_host(act):
    def host():
        state = torch.zeros(2, dtype=torch.float32)
        return list(FQ.observe_percentile(big()[0], run_minmax=state, tail=tail_of(99.99), bins=2048, act=act,
                                          **PCT_KW)) + [state]
    return host_once(("pct", act), host)


@pytest.mark.parametrize("act", ACTS)
def test_percentile_observer_nt_arm_equals_host(act):
    """k_observe_hist<1, 1, ACT> at 2048 bins / 99.99 against the host loop on the CPU copy."""
    hqp, hst, hclip, hstate = _pct_host(act)
    qp, st, clip, state = _pct_device(act, 2048, 99.99, 1)
    for k in (H.ST_MIN, H.ST_MAX, H.ST_NAN, H.ST_N):
        assert float(st[k]) == float(hst[k]), (act, k)
    assert M.same_bits(clip, hclip) and M.same_bits(qp, hqp) and M.same_bits(state, hstate), act
    assert float(clip[0]) < float(clip[1]) < float(hst[H.ST_MAX])   # the histogram was used: the top was clipped


@pytest.mark.parametrize("bins", [256, 4096])
def test_percentile_observer_nt_arm_other_bin_counts(bins):
    """The same arm at the smallest and the largest histogram: the host histogram loop on the host
    observer's record of the CPU copy."""
    hst = _pct_host(None)[1]
    hstate = torch.zeros(2, dtype=torch.float32)
    hqp, hclip = _host_hist(big()[0], hst, bins, tail_of(99.99), hstate, False)
    qp, st, clip, state = _pct_device(None, bins, 99.99, 1)
    assert float(st[H.ST_MIN]) == float(hst[H.ST_MIN]) and float(st[H.ST_MAX]) == float(hst[H.ST_MAX])
    assert M.same_bits(clip, hclip) and M.same_bits(qp, hqp) and M.same_bits(state, hstate), bins


@pytest.mark.parametrize("act", ACTS)
def test_percentile_observer_cached_arm_at_the_full_grid(act):
    """k_observe_hist<1, 0, ACT> on the same tensor: the NT arm's result."""
    assert _same_all(_pct_device(act, 2048, 99.99, 1), _pct_device(act, 2048, 99.99, 0))


# --------------------------------------------------------------------------- 2. PerChannelMSEObserver
F = PC.forms()


def _pc_block_steps():
    """(elements of one block-form step per row, the NC values the launch instantiates)."""
    src = _src("k_pc_mse.hip")
    chunks = _const(src, "kPcMseBlockChunks")
    assert "with_int_le<1, 2, 3, kPcMseBlockChunks>(cdiv(a.rowlen, 4 * kBlock * kPcMseU)" in src
    assert "with_int_le<1, kPcMseWaveChunks>(cdiv(a.rowlen, 4 * kWave * kPcMseU)" in src
    assert "if (a.rowlen <= kPcMseWaveShort)" in src
    assert F["block_max"] % chunks == 0
    return F["block_max"] // chunks, sorted({1, 2, 3, chunks})


def pc_form(rowlen):
    """(form, NC) the launch code selects for a row length: with_int_le takes the first listed NC that
    holds cdiv(rowlen, step)."""
    bstep, ncs = _pc_block_steps()
    wstep = F["wave_max"] // _const(_src("k_pc_mse.hip"), "kPcMseWaveChunks")
    if rowlen <= F["wave_short"]:
        return "wave-short", 1
    if rowlen <= F["wave_max"]:
        return "wave", min(nc for nc in (1, F["wave_max"] // wstep) if nc >= -(-rowlen // wstep))
    if rowlen <= F["block_max"]:
        return "block", min(nc for nc in ncs if nc >= -(-rowlen // bstep))
    return "long", 0


BSTEP, BNCS = _pc_block_steps()
# vec: one length per instantiation; tail: one length per form (the scalar path has no NT instance)
PC_VEC = [256, F["wave_max"] // 2, F["wave_max"]] + [BSTEP * k for k in BNCS] + [F["block_max"] + 4]
PC_TAIL = [257, BSTEP * 2 + 3, F["block_max"] + 5]
PC_FAMILIES = ("gauss", "heavy", "relu")


def test_pc_mse_lengths_select_every_instantiation():
    assert [pc_form(n) for n in PC_VEC] == [("wave-short", 1), ("wave", 1), ("wave", 2)] + \
        [("block", k) for k in BNCS] + [("long", 0)]
    assert BNCS == [1, 2, 3, 4] and [BSTEP * k for k in BNCS] == [3072 * k for k in (1, 2, 3, 4)]
    assert [pc_form(n)[0] for n in PC_TAIL] == ["wave", "block", "long"]
    assert all(n % 4 == 0 for n in PC_VEC) and all(n % 4 != 0 for n in PC_TAIL)


@functools.lru_cache(maxsize=None)
def _pc_case(rowlen):
    """(CPU tensor, oracle rows, the host entry point's result with and without y), once per length."""
    _, xc, rows = PC.pick_seed(PC_FAMILIES, rowlen, PC.mse_ratios(), False, 4)
    kw = _pc_kw()
    hq = FQ.per_channel_observe_mse(xc, run_min=torch.zeros(3), run_max=torch.zeros(3), want_mask=True, **kw)
    ho = FQ.per_channel_observe_mse(xc, run_min=torch.zeros(3), run_max=torch.zeros(3), quantize=False, **kw)
    return xc, rows, hq, ho


def _pc_kw():
    qmin, qmax = PC.grid_of(4, False)
    return dict(symmetric=False, qmin=qmin, qmax=qmax, num_bits=4, ratios=PC.mse_ratios(), want_row_stats=True)


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("rowlen", PC_VEC + PC_TAIL)
def test_pc_mse_observer(rowlen, nt):
    """launch_pc_mse: the wave form (one group per lane; NC 1, 2), the workgroup form (NC 1..4) and the
    long-row form x three (VEC, NT) pairs x y wanted or not, 3 rows: the oracle's rows, then the host
    entry point's pick, clip, running state, qparams and y bit for bit."""
    xc, rows, hq, ho = _pc_case(rowlen)
    kw = _pc_kw()
    tag = (rowlen, pc_form(rowlen), nt)
    x = xc.to(DEV)
    assert x.data_ptr() % 16 == 0
    with tuned(NONTEMPORAL=nt):
        rq = FQ.per_channel_observe_mse(x, run_min=torch.zeros(3, device=DEV), run_max=torch.zeros(3, device=DEV),
                                        want_mask=True, **kw)
        ro = FQ.per_channel_observe_mse(x, run_min=torch.zeros(3, device=DEV), run_max=torch.zeros(3, device=DEV),
                                        quantize=False, **kw)
    for r, h in ((rq, hq), (ro, ho)):
        state = PC.OracleState(3, False, 4)
        state.update(rows)
        PC.check_against_oracle(r, rows, state, tag)
        PC.check_against_oracle(h, rows, state, tag)
        # (the host adds a row's f64 terms in another order: its E_k are held to the oracle above)
        assert PC.same_result(r, h, keys=("pick", "clip", "scale", "zp", "run_min", "run_max")), tag
    assert PC.same_result(rq, ro), tag   # with and without y: one search, the same bits
    assert ro["y"] is None and PC.same_bits(rq["y"], hq["y"]), tag
    # the mask in the device's 1-bit layout: the fixed-qparam kernel's (default knob) for the qparams returned
    y, mask, _ = FQ.per_channel_fake_quant(x, rq["scale"], rq["zp"], kw["qmin"], kw["qmax"], want_mask=True)
    assert PC.same_bits(rq["y"], y) and PC.same_bits(rq["mask"], mask), tag


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("lay,rowlen", [("vec", 64), ("vec", 2052), ("tail", 61), ("offset", 64)])
def test_pc_fixed_fake_quant(lay, rowlen, nt):
    """vsiq_pcm_fq_fwd_f32 (the fixed-qparam per-channel forward the observer tests above lean on): the
    packed-rows form (no mask, short rows) and the per-row form (mask; rows of more than one workgroup) x
    three (VEC, NT) pairs: y and the mask of the host entry point, the codes of the numpy restatement."""
    x = P.make_x(3, rowlen, seed=rowlen)
    s, z = P.make_qparams(3, 4, False, True, seed=rowlen)
    yh, mh = host.pc_fake_quant(x, s, z, 0, 15, zp_round=True, want_mask=True)
    codes = P.codes_np(x.numpy(), P.f32_qparams(s.numpy(), z.numpy(), 3, 0, 15, True), 0, 15)
    xd = _offset(x) if lay == "offset" else x.to(DEV)
    assert (rowlen % 4 != 0) == (lay == "tail")
    for mask in (False, True):
        with tuned(NONTEMPORAL=nt):
            y, m, c = FQ.per_channel_fake_quant(xd, s.to(DEV), z.to(DEV), 0, 15, zp_round=True, want_mask=mask,
                                                want_codes=True)
        assert P.same_bits(y, yh), (lay, rowlen, nt, mask)
        assert np.array_equal(c.cpu().numpy().astype(np.int64), codes), (lay, rowlen, nt, mask)
        if mask:
            assert np.array_equal(G.unpack_mask(m.cpu().numpy(), 3, rowlen), mh.numpy().astype(bool)), (lay, rowlen, nt)


# --------------------------------------------------------------------------- 3. pack / unpack
PACK_ROWS = 3
PACK_LENS = (64, 20, 17)   # vec and wide (% 16 == 0); vec, not wide; scalar
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _offset(t):
    """t's values on a view one element into a fresh allocation (not 16-byte aligned)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _pack_case(x, scale, zp, qmin, qmax, bits, per_row, lay, nt, tag):
    dev = (lambda v: v.to(DEV) if isinstance(v, torch.Tensor) else v)
    xd = _offset(x) if lay == "offset" else x.to(DEV)
    axis = 0 if per_row else None
    x2 = x if per_row else x.reshape(1, -1)
    rows, rowlen = x2.shape
    ph = FQ.quantize_pack(x, scale, zp, qmin, qmax, bits=bits, axis=axis, zp_round=True)   # the host loop
    with tuned(NONTEMPORAL=nt):
        p = FQ.quantize_pack(xd, dev(scale), dev(zp), qmin, qmax, bits=bits, axis=axis, zp_round=True)
        outs = {(dt, wc): FQ.unpack_dequant(p, dt, want_codes=wc) for dt in DTYPES for wc in (False, True)}
        only = torch.empty(p.shape, dtype=torch.uint8, device=DEV)   # codes alone: no y
        rc = H.lib().vsiq_unpack_dequant(H.ptr(p.data), None, H.ptr(only), H.c_i64(rows), H.c_i64(rowlen),
                                         H.ptr(p.qparams), H.c_i64(p.qparams.shape[0]), p.qmin, p.bits, H.DT_F32,
                                         H.stream_of(torch.device(DEV)))
    assert rc == 0, tag
    codes_ref, y_ref = P.check_packed(p, x2, scale, zp, qmin, qmax, bits, per_row, True, tag)
    assert not (p.data.cpu().numpy() & P.padding_mask(rowlen, bits)[None, :]).any(), tag
    assert P.same_bits(p.data, ph.data) and P.same_bits(p.qparams, ph.qparams), tag
    yh, ch = FQ.unpack_dequant(ph, want_codes=True)
    want_c = torch.from_numpy(codes_ref.astype(np.uint8)).reshape(p.shape)
    assert P.same_bits(ch, want_c) and P.same_bits(yh.reshape(x2.shape), y_ref), tag
    assert P.same_bits(only, want_c), tag
    for (dt, wc), out in outs.items():
        y, c = out if wc else (out, None)
        want_y = torch.from_numpy(y_ref).to(dt).reshape(p.shape)   # rounded once to dt
        raw = torch.int32 if dt == torch.float32 else torch.int16
        assert y.dtype == dt and P.same_bits(y.view(raw), want_y.view(raw)), (tag, dt)
        if wc:
            assert P.same_bits(c, want_c), (tag, dt)


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("bits", P.BITS)
def test_pack_unpack(bits, nt, monkeypatch):
    """vsiq_quantize_pack_f32 (bits x three (VEC, NT) pairs x per-row x wide) and vsiq_unpack_dequant
    (bits x element type x the pairs; y and codes, y alone, codes alone) on buffers that held 0xFF:
    packed bytes, recorded qparams and zero padding bits of the numpy restatement and the host loop,
    y of the restatement rounded once to the element type."""
    real_empty = torch.empty

    def dirty_empty(*a, **k):
        t = real_empty(*a, **k)
        if t.dtype == torch.uint8:
            t.fill_(0xFF)
        return t
    monkeypatch.setattr(FQ.torch, "empty", dirty_empty)
    qmin, qmax = P.grid(bits, False)
    for i, rowlen in enumerate(PACK_LENS):
        x = P.make_x(PACK_ROWS, rowlen, seed=10 * bits + i)
        for per_row in (True, False):
            s, z = P.make_qparams(PACK_ROWS, bits, False, per_row, seed=i)
            _pack_case(x if per_row else x.reshape(-1), s, z, qmin, qmax, bits, per_row, "aligned", nt,
                       (bits, rowlen, per_row, nt))
        if rowlen % 4 == 0:   # the vec shapes one element into an allocation: the scalar path
            s, z = P.make_qparams(PACK_ROWS, bits, False, True, seed=i)
            _pack_case(x, s, z, qmin, qmax, bits, True, "offset", nt, (bits, rowlen, "offset", nt))


# --------------------------------------------------------------------------- 4. AdaRound
# vec shapes (row length % 4 == 0): one row (per tensor) of two workgroups, rows of two workgroups, and
# the regulariser's folds above 128 and above 2048 workgroups
ADA_VEC = (("vec1x2052", 1, A.WG_SPAN + 4, False), ("vec3x1032", 3, 1032, True), ("vec130x8", 130, 8, True),
           ("vec2050x4", 2050, 4, True))
ADA_OLD = tuple(A.all_cases()) + tuple((f"fold{r}x{c}", r, c, True) for r, c in A.SHAPES_FOLD)


def _ada_check(tag, rows, rowlen, per_row, nt):
    """soft, hard, soft + R, R alone and the backward on one shape: tests/test_gpu_adaround.py's bars."""
    with tuned(NONTEMPORAL=nt):
        for k, (bits, sym) in enumerate(A.GRIDS):
            w, Vv, g, sc, zp, lo, hi = A.make_case(rows, rowlen, bits, sym, per_row, seed=31 * k + rowlen)
            for hard in (False, True):
                yd, _ = A.run(w, Vv, sc, zp, lo, hi, per_row, DEV, hard=hard)
                yh, _ = A.run(w, Vv, sc, zp, lo, hi, per_row, hard=hard)
                assert A.bits_equal(yd, yh), (tag, bits, sym, hard, nt)
            gd = A.run_bwd(g, w, Vv, sc, zp, lo, hi, per_row, DEV, lam=0.0, beta=2.0)
            gh = A.run_bwd(g, w, Vv, sc, zp, lo, hi, per_row, lam=0.0, beta=2.0)
            assert A.bits_equal(gd, gh), (tag, bits, sym, nt)
        beta = 3.7
        w, Vv, g, sc, zp, lo, hi = A.make_case(rows, rowlen, 4, False, per_row, seed=rowlen + 1)
        h = A.lib_h(Vv)
        yd, R = A.run(w, Vv, sc, zp, lo, hi, per_row, DEV, beta=beta)
        Ro = A.oracle_reg(h, beta)
        print(tag, nt, "R", float(R), Ro)
        assert abs(float(R) - Ro) <= 1e-9 * abs(Ro), (tag, nt)
        assert A.bits_equal(yd, A.run(w, Vv, sc, zp, lo, hi, per_row)[0]), (tag, nt)   # y is the same with R asked
        _, R2 = A.run(w, Vv, sc, zp, lo, hi, per_row, DEV, beta=beta, want_y=False)
        _, R3 = A.run(w, Vv, sc, zp, lo, hi, per_row, DEV, beta=beta)
        assert float(R2) == float(R) == float(R3), (tag, nt)   # fixed order; the counter was left at 0
        gd = A.run_bwd(g, w, Vv, sc, zp, lo, hi, per_row, DEV, lam=0.01, beta=beta).cpu().numpy()
        go = A.oracle_grad(g, w, Vv, sc, zp, lo, hi, 0.01, beta, h=h)
        d = A.ulp_distance(gd, go).max()
        print(tag, nt, "max ulp", d)
        assert d <= 1, (tag, nt)


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("tag,rows,rowlen,per_row", ADA_VEC)
def test_adaround_vector_shapes(tag, rows, rowlen, per_row, nt):
    """k_adaround_fwd<1, NT, MODE> (four modes) and k_adaround_bwd<1, NT> with every fold of the regulariser."""
    assert rowlen % 4 == 0
    _ada_check(tag, rows, rowlen, per_row, nt)


@pytest.mark.parametrize("tag,rows,rowlen,per_row", ADA_OLD)
def test_adaround_cached_arm(tag, rows, rowlen, per_row):
    """Every shape of tests/test_gpu_adaround.py with the knob off."""
    _ada_check(tag, rows, rowlen, per_row, 0)


# --------------------------------------------------------------------------- 5. multi-tensor LSQ
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("count", [len(TM.SIZES), 40])
def test_lsq_multi_cached_arm(asym, count):
    """k_lsq_fwd_multi<false> / k_lsq_bwd_multi<false>: per tensor the per-tensor path's bits (default
    knob) and the oracle's closed form."""
    sizes = (TM.SIZES * 3)[:count]
    cases = [TM._case(n, i, asym) for i, n in enumerate(sizes)]
    xs = [c[0].clone().requires_grad_(True) for c in cases]
    specs = [FQ.LsqSpec(c[2], c[3], c[4], c[5], c[6], asym) for c in cases]
    with tuned(NONTEMPORAL=0):
        ys = FQ.lsq_fake_quant_multi(xs, specs)
        torch.autograd.backward(ys, [c[1] for c in cases])
        torch.cuda.synchronize()
    got = [(y.detach().clone(), x.grad.clone(), c[2].grad.clone(), c[3].grad.clone() if asym else None)
           for x, y, c in zip(xs, ys, cases)]
    for c in cases:
        c[2].grad = None
        if asym:
            c[3].grad = None
    for (x0, gy, s, zp, qmin, qmax, gscale), (y, gx, gs, gz) in zip(cases, got):
        x = x0.clone().requires_grad_(True)
        yr = FQ.FakeQuantLearnFn.apply(x, s, zp, qmin, qmax, gscale, asym, None)
        yr.backward(gy)
        G.assert_bitwise_f32(y.cpu().numpy(), yr.detach().cpu().numpy(), "y")
        G.assert_bitwise_f32(gx.cpu().numpy(), x.grad.cpu().numpy(), "grad_x")
        assert torch.equal(gs, s.grad), (gs, s.grad)
        if asym:
            assert torch.equal(gz, zp.grad), (gz, zp.grad)
        s.grad = None
        if asym:
            zp.grad = None
        yo, gxo, gso, gzo = O.lsq_forward_backward(x0.cpu().numpy(), gy.cpu().numpy(), float(s), float(zp), qmin, qmax,
                                                   gscale, learn_zp=asym)
        G.assert_bitwise_f32(y.cpu().numpy(), yo, "y (oracle)")
        G.assert_bitwise_f32(gx.cpu().numpy(), gxo, "grad_x (oracle)")
        assert float(gs) == pytest.approx(gso, rel=1e-9, abs=1e-12)
        if asym:
            assert float(gz) == pytest.approx(gzo, rel=1e-9, abs=1e-12)


# --------------------------------------------------------------------------- 6. 16-bit kernels
# The reference is tests/test_gpu_half.py's: the fp32 entry point (default knob: the arm the fp32 suites
# hold to the oracle) on the widened tensor, rounded once to the element type.
def _off(fn, *a, **k):
    with tuned(NONTEMPORAL=0):
        return fn(*a, **k)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", TH.DTYPES)
def test_half_forward_every_input_value_cached_arm(dtype, act):
    x = TH.all_patterns(dtype)
    xf = x.float()
    for qmin, qmax, s, zp in TH.CONFIGS:
        y, m, c = _off(FQ.fake_quant, x, s, zp, qmin, qmax, want_mask=True, want_codes=True, act=act)
        yo, mo, co = FQ.fake_quant(xf, s, zp, qmin, qmax, want_mask=True, want_codes=True, act=act)
        assert y.dtype == dtype and y.shape == x.shape
        TH.assert_bits(y, yo, f"y {qmin}..{qmax}")
        assert c.dtype == co.dtype and torch.equal(c, co)
        assert torch.equal(m, mo)


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("dtype", TH.DTYPES)
def test_half_ste_backward_cached_arm(dtype, act):
    g = TH.all_patterns(dtype)
    x = TH.permuted(g)
    _, mask, _ = FQ.fake_quant(x.float(), 0.05, 0, -128, 127, want_mask=True, act=act)
    gx = _off(FQ.ste_backward, g, mask, 0.05, pre=x if act else None, act=act)
    gxo = FQ.ste_backward(g.float(), mask, 0.05, pre=x.float() if act else None, act=act)
    assert gx.dtype == dtype
    TH.assert_bits(gx, gxo, "gx")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("zp_learn", [0, 1])
@pytest.mark.parametrize("dtype", TH.DTYPES)
def test_half_lsq_backward_cached_arm(dtype, zp_learn, act):
    torch.manual_seed(3)
    qmin, qmax, zp = (0, 255, 37.0) if zp_learn else (-128, 127, 0.0)
    cases = [(TH.all_patterns(dtype), TH.permuted(TH.all_patterns(dtype)))]
    for n in (4099, 3 * 4 * TH.KBLOCK * TH.LSQ_G[0] + 5):
        cases.append((torch.randn(n, device=DEV).to(dtype), (torch.randn(n, device=DEV) * 4).to(dtype)))
    for g, x in cases:
        gx, grads = _off(FQ.lsq_backward, g, x, 0.05, zp, qmin, qmax, 0.02, zp_learn, act=act)
        gxo, gradso = FQ.lsq_backward(g.float(), x.float(), 0.05, zp, qmin, qmax, 0.02, zp_learn, act=act)
        assert gx.dtype == dtype
        TH.assert_bits(gx, gxo, f"gx n={g.numel()}")
        assert TH.same_bits(grads, gradso), (g.numel(), grads.tolist(), gradso.tolist())
    assert torch.isfinite(grads).all() and float(grads[0]) != 0.0


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("dtype", TH.DTYPES)
def test_half_edges_cached_arm(dtype, aligned):
    """Forward, STE backward and K4 at tests/test_gpu_half.py's edge sizes, 8-byte aligned and one element off."""
    torch.manual_seed(11)
    place = (lambda t: t) if aligned else TH.offset_view
    for n in TH.EDGE_N:
        x0 = (torch.randn(n, device=DEV) * 3).to(dtype)
        g0 = torch.randn(n, device=DEV).to(dtype)
        x, g = place(x0), place(g0)
        xf, gf = x0.float(), g0.float()
        for act in (None, "relu"):
            y, m, c = _off(FQ.fake_quant, x, 0.05, 0, -128, 127, want_mask=True, want_codes=True, act=act)
            yo, mo, co = FQ.fake_quant(xf, 0.05, 0, -128, 127, want_mask=True, want_codes=True, act=act)
            TH.assert_bits(y, yo, f"fwd n={n}")
            assert torch.equal(c, co) and torch.equal(m, mo), n
            gx = _off(FQ.ste_backward, g, mo, 0.05, pre=x if act else None, act=act)
            gxo = FQ.ste_backward(gf, mo, 0.05, pre=xf if act else None, act=act)
            TH.assert_bits(gx, gxo, f"ste n={n}")
            kx, kg = _off(FQ.lsq_backward, g, x, 0.05, 3.0, 0, 255, 0.01, 1, act=act)
            kxo, kgo = FQ.lsq_backward(gf, xf, 0.05, 3.0, 0, 255, 0.01, 1, act=act)
            TH.assert_bits(kx, kxo, f"k4 n={n}")
            assert TH.same_bits(kg, kgo), (n, kg.tolist(), kgo.tolist())
