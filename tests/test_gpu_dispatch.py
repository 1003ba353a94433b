"""Every arm of the launch dispatch in csrc/ once, through the C ABI (MI355X only).

The launch code turns runtime facts into kernel template arguments: 16-byte alignment and
n % 4 (VEC), the non-temporal knob (NT), the activation (ACT), codes / mask wanted, and a
groups-per-lane count or workgroup size (G / U / NV / BS / S).  Each test crosses those
for one entry point at the smallest shape that selects the arm (thresholds read from the
launch code's constants) and compares with the oracle (oracle/fakequant_np.py) or the
library's host entry points (vsiq_host_*, pinned bitwise to the reference by the CPU
suite), with the assertions of the parity tests: y / codes / mask / grad_x bit for bit,
min / max / NaN count / qparams exact, sums <= 1e-6, scale / zero-point gradients <= 1e-9.

Layouts: "vec" = n % 4 == 0 on a 16-byte-aligned tensor; "tail" = n % 4 != 0; "offset" =
the vec n on a view one element into the allocation.  Forms chosen by CU count and
occupancy (the one-round gated grids) are covered by size without asserting which ran.
"""
import numpy as np
import pytest
import torch

from vsiquantization_amd import _hip as H
from vsiquantization_amd import fakequant as FQ
from vsiquantization_amd.quantizers.deferred import lsq_backward_part
from oracle import fakequant_np as O
from tests import goldens as G
from tests.tuning_common import tuned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYS = ("vec", "tail", "offset")
ACTS = (None, "relu", "silu")
NMAX = 13_107_200          # the largest one-round gated size (9 groups per lane of 256 lanes)
ONE_ROUND = (3_276_800, 13_107_200)   # 2 / 9 groups per lane are one round at 256 CUs
S, Z, QMIN, QMAX = 0.021, 3, 0, 255
_base = {}
_want = {}


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    H.lib()
    H.set_silu_reference(*G.GOLDEN_SILU_REF)
    gen = torch.Generator().manual_seed(20)
    for k, scale in (("x", 2.0), ("g", 1.0)):
        c = torch.randn(NMAX + 8, generator=gen) * scale
        _base[k] = (c, c.to(DEV))
    yield
    H.set_silu_reference()
    _base.clear()
    _want.clear()


def REF():
    return H.silu_reference()


def view(k, n, lay):
    """(CPU tensor, device tensor) of n elements of base k in layout lay."""
    assert (n % 4 != 0) == (lay == "tail")
    o = 1 if lay == "offset" else 0
    c, d = _base[k]
    return c[o:o + n], d[o:o + n]


def sized(n4, lay, delta=3):
    return n4 + delta if lay == "tail" else n4


def npy(t):
    return t.detach().cpu().numpy()


def cached(key, fn):
    if key not in _want:
        _want[key] = fn()
    return _want[key]


def host_observe(n, lay, act):
    """(qp, stats) of act(x) from the host entry point (vsiq_host_observe_f32)."""
    def run():
        qp, st = FQ.observe_tensor(view("x", n, lay)[0], symmetric=False, act=act)
        return npy(qp), npy(st)
    return cached(("obs", n, lay, act), run)


def check_stats(st, want, what):
    for k in (H.ST_MIN, H.ST_MAX, H.ST_NAN, H.ST_N):
        assert st[k] == want[k], (what, k)
    assert st[H.ST_SUMABS] == pytest.approx(want[H.ST_SUMABS], rel=1e-6), what
    assert st[H.ST_SUM] == pytest.approx(want[H.ST_SUM], rel=1e-6, abs=1e-6 * want[H.ST_SUMABS]), what
    assert st[H.ST_SUMSQ] == pytest.approx(want[H.ST_SUMSQ], rel=1e-6), what


def check_qp(qp, want, what):
    for k in (H.QP_SCALE, H.QP_ZP, H.QP_MIN, H.QP_MAX):
        assert qp[k] == want[k], (what, k)


def act_fwd(n, lay, act):
    return cached(("act", n, lay, act), lambda: O.act_forward(npy(view("x", n, lay)[0]), act, REF()))


# --------------------------------------------------------------------------- K1 / K5 forward, STE backward
def _fq_ste(n, lay, act, codes, mask):
    what = (n, lay, act, codes, mask)
    xc, xd = view("x", n, lay)
    gc, gd = view("g", n, lay)
    y, m, c = FQ.fake_quant(xd, S, Z, QMIN, QMAX, want_mask=mask, want_codes=codes, act=act)
    yo, qo, mo = cached(("fq", n, lay, act), lambda: O.fq_forward(act_fwd(n, lay, act), S, Z, QMIN, QMAX))
    G.assert_bitwise_f32(npy(y), yo, f"y {what}")
    if codes:
        assert np.array_equal(npy(c).astype(np.int64), qo.astype(np.int64)), what
    if mask:
        assert np.array_equal(G.unpack_mask(npy(m), 1, n)[0], mo), what
        gx = FQ.ste_backward(gd, m, S, pre=xd if act else None, act=act)
        go = cached(("ste", n, lay, act), lambda: O.act_backward(O.fq_backward_fixed(npy(gc), mo, S), npy(xc), act,
                                                                 REF()))
        G.assert_bitwise_f32(npy(gx), go, f"grad_x {what}")


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("lay", LAYS)
def test_fq_fwd_and_ste_bwd(lay, nt):
    """launch_fq (four (VEC, NT) pairs x act x codes x mask) and launch_ste (four pairs x act), 3 workgroups."""
    n = sized(5000, lay)
    with tuned(NONTEMPORAL=nt):
        for act in ACTS:
            for codes in (False, True):
                for mask in (False, True):
                    _fq_ste(n, lay, act, codes, mask)


@pytest.mark.parametrize("n", ONE_ROUND)
def test_fq_fwd_and_ste_bwd_one_round_sizes(n):
    """The sizes whose grids are one round at 256 CUs (store gate; K1's and the STE's 9 groups per lane)."""
    _fq_ste(n, "vec", "relu", False, True)


# --------------------------------------------------------------------------- K2
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("lay", LAYS)
def test_observe(lay, act):
    """launch_observe: the grid-stride kernel (one workgroup up to 8192 elements, several above) and the
    one-shot kernel at 2 / 4 / 16 groups per lane (K4's 8 runs as 4).  Under 256 MB the loads are cached
    whatever the knob says, so NT is off here; test_observe_nontemporal has the NT arm."""
    for n4 in (5000, 40_000):
        n = sized(n4, lay)
        xd = view("x", n, lay)[1]
        wq, ws = host_observe(n, lay, act)
        for kernel, groups in ((0, 0), (1, 2), (1, 0), (1, 8), (1, 16)):
            with tuned(OBS_KERNEL=kernel, LSQ_GROUPS=groups):
                qp, st = FQ.observe_tensor(xd, symmetric=False, act=act)
            check_stats(npy(st), ws, (n, lay, act, kernel, groups))
            check_qp(npy(qp), wq, (n, lay, act, kernel, groups))


def test_observe_nontemporal():
    """K2's NT arm: taken from 256 MB (kObsTemporalMB) with the knob on, on the vector path only."""
    n = 1 << 26
    xc = torch.randn(n, generator=torch.Generator().manual_seed(26))
    xd = xc.to(DEV)
    for act in ACTS:
        wq, ws = (npy(t) for t in FQ.observe_tensor(xc, symmetric=False, act=act))
        for kernel, groups in ((0, 0), (1, 2), (1, 0), (1, 16)):
            with tuned(OBS_KERNEL=kernel, LSQ_GROUPS=groups):
                qp, st = FQ.observe_tensor(xd, symmetric=False, act=act)
            check_stats(npy(st), ws, (act, kernel, groups))
            check_qp(npy(qp), wq, (act, kernel, groups))


# --------------------------------------------------------------------------- K2p / K2m / K2o
# observe_part_u: units = cdiv(cdiv(n, 4), 256) >= 512 * 8 -> 8 groups per lane per step, >= 512 * 4 -> 4,
# else 2.  The first n % 4 == 0 size of each, the last below each threshold, and a small one.
PART_SIZES = {2: (4096, 2_096_128), 4: (2_096_132, 4_193_280), 8: (4_193_284,)}


def part_sizes(lay):
    """[(n, U)]: both sides of each threshold; the tail layout's n - 3 has the same group count."""
    return [(n - 3 if lay == "tail" else n, u) for u, ns in PART_SIZES.items() for n in ns]


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("lay", LAYS)
def test_observe_parts(lay, nt):
    """launch_observe_part (U 2 / 4 / 8 x three (VEC, NT) pairs x act) and K2m (NT x all-vector x act):
    the folded records against the host observer, K2m's records bit for bit K2p's."""
    with tuned(NONTEMPORAL=nt):
        for act in ACTS:
            xs, singles = [], []
            for n, u in part_sizes(lay):
                xd = view("x", n, lay)[1]
                parts = FQ.observe_parts(xd, act=act)
                assert parts.numel() == FQ.part_slot_doubles(n)
                check_stats(npy(FQ.fold_parts(parts.view(1, -1)))[0], host_observe(n, lay, act)[1], (n, u, lay, act))
                xs.append(xd)
                singles.append(parts)
            for mixed in (False, True):   # all tensors on the vector path, or not
                if mixed:
                    xs.append(view("x", 4099, "tail")[1])
                    singles.append(FQ.observe_parts(xs[-1], act=act))
                multi = FQ.observe_parts_multi(xs, None, act=act)
                for a, b in zip(multi, singles):
                    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (lay, act, mixed)


def _parts_out(n, lay, act, what):
    xd = view("x", n, lay)[1]
    y, parts = FQ.observe_parts_out(xd, act)
    G.assert_bitwise_f32(npy(y), act_fwd(n, lay, act), f"y {what}")
    check_stats(npy(FQ.fold_parts(parts.view(1, -1)))[0], host_observe(n, lay, act)[1], what)


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("lay", LAYS)
def test_observe_parts_out(lay, nt):
    """K2o: the grid-stride form (U 2 / 4 / 8), the one-shot form at every (groups, block) the knobs can
    select, and the default knobs (small: 2 x 256 ungated; the one-round sizes: the gated forms where the
    device's CU count and the occupancy allow them)."""
    with tuned(NONTEMPORAL=nt):
        for act in ACTS:
            with tuned(K2O_FORM=1):
                for n, u in part_sizes(lay):
                    _parts_out(n, lay, act, (n, u, lay, act, "grid-stride"))
            n = sized(20_480, lay)
            for g in (1, 2, 4, 8, 16):
                for bs in (256, 512, 1024):
                    with tuned(K2O_GROUPS=g, K2O_BLOCK=bs):
                        _parts_out(n, lay, act, (n, lay, act, g, bs))
            for n4 in (20_480,) + ONE_ROUND:
                _parts_out(sized(n4, lay), lay, act, (n4, lay, act, "default"))


# --------------------------------------------------------------------------- K8 / K9 / K10 / K1r
# K8: 2 groups per lane of its 1024 lanes up to kSmallBlock * 2 * 4 = 8192 elements, else 16.
# K10: fold_fq_part_grid(n) <= 32 workgroups x 256 lanes x 4 groups hold n in one step up to 131072 elements.
def _observe_fq_forms(lay):
    t = lay == "tail"
    return [("k8", False, 8191 if t else 8192), ("k8", False, 8193 if t else 8196),
            ("k9", True, sized(20_000, lay)), ("k10", "k10", 131_071 if t else 131_072),
            ("k10", "k10", 131_073 if t else 131_076), ("k1r", None, sized(20_000, lay))]


def _ranks_fq(xd, act, mask, codes):
    n = xd.numel()
    _, local = FQ.observe_tensor(xd, symmetric=False, want_qp=False, act=act)
    y = torch.empty_like(xd)
    qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=DEV)
    st = torch.empty(H.ST_LEN, dtype=torch.float64, device=DEV)
    m = H.mask_buffer(1, n, xd.device) if mask else None
    c = torch.empty(n, dtype=torch.uint8, device=DEV) if codes else None
    rc = H.lib().vsiq_act_fq_fwd_ranks_f32(H.ptr(xd), H.ptr(y), H.ptr(c), H.ptr(m), H.c_i64(n), H.act_code(act),
                                           H.ptr(local), 1, H.ptr(st), None, H.ptr(qp), 0, FQ.qden(False, 8, 1e-8),
                                           1e-8, QMIN, QMAX, H.stream_of(xd.device))
    H.check(rc, "vsiq_act_fq_fwd_ranks_f32")
    return y, qp, st, m, c


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("lay", LAYS)
def test_observe_fq(lay, nt):
    """K8 (U 2 / 16), K9 (K2p at 4 groups per lane + the fold in every workgroup), K10 (1 / 2 steps) and
    K1r, each over three (VEC, NT) pairs x act x codes x mask: the host observer's record, then y / codes /
    mask of the host fake quant at that record's qparams."""
    with tuned(NONTEMPORAL=nt):
        for act in ACTS:
            for form, parts, n in _observe_fq_forms(lay):
                xc, xd = view("x", n, lay)
                wq, ws = host_observe(n, lay, act)
                yo, mo, co = cached(("ofq", n, lay, act), lambda: [npy(t) for t in FQ.fake_quant(
                    xc, None, None, QMIN, QMAX, qp=torch.from_numpy(wq), want_mask=True, want_codes=True, act=act)])
                for codes in (False, True):
                    for mask in (False, True):
                        what = (form, n, lay, act, codes, mask)
                        if form == "k1r":
                            y, qp, st, m, c = _ranks_fq(xd, act, mask, codes)
                        else:
                            y, qp, st, m, c = FQ.observe_fake_quant(xd, symmetric=False, qmin=QMIN, qmax=QMAX, act=act,
                                                                    want_mask=mask, want_codes=codes, parts=parts)
                        check_qp(npy(qp), wq, what)
                        check_stats(npy(st), ws, what)
                        G.assert_bitwise_f32(npy(y), yo, f"y {what}")
                        if codes:
                            assert np.array_equal(npy(c), co), what
                        if mask:
                            assert np.array_equal(G.unpack_mask(npy(m), 1, n)[0], mo.astype(bool)), what


# --------------------------------------------------------------------------- K4 / K4d
@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("lay", LAYS)
def test_lsq_bwd(lay, nt):
    """launch_lsq: four (VEC, NT) pairs x act x 2 / 4 / 8 / 16 groups per lane x learnable zero point, with
    the arrival fold (K4) and records only (K4d + vsiq_lsq_fold_multi)."""
    n = sized(40_000, lay)
    xc, xd = view("x", n, lay)
    gc, gd = view("g", n, lay)
    gscale = O.grad_scale(QMAX, n)
    with tuned(NONTEMPORAL=nt):
        for act in ACTS:
            for zpl in (False, True):
                z = 3.2 if zpl else 3

                def want():
                    _, gxo, gso, gzo = O.lsq_forward_backward(act_fwd(n, lay, act), npy(gc), S, z, QMIN, QMAX, gscale,
                                                              learn_zp=zpl)
                    return O.act_backward(gxo, npy(xc), act, REF()), gso, gzo
                gxo, gso, gzo = cached(("lsq", n, lay, act, zpl), want)
                for groups in (2, 4, 8, 16):
                    what = (n, lay, act, zpl, groups)
                    with tuned(LSQ_GROUPS=groups):
                        gx, grads = FQ.lsq_backward(gd, xd, S, z, QMIN, QMAX, gscale, zpl, act=act)
                        nrec = int(H.lib().vsiq_lsq_part_records(H.c_i64(n)))
                        rec = torch.empty(2 * nrec, dtype=torch.float64, device=DEV)
                        gxp, _, zh = lsq_backward_part(gd, xd, S, z, QMIN, QMAX, zpl, act, rec)
                    out = torch.empty(2, dtype=torch.float64, device=DEV)
                    fold = (H.LsqFold * 1)(H.LsqFold(rec.data_ptr(), nrec, None, zh, gscale, out.data_ptr(), QMIN, QMAX,
                                                     int(zpl), 0))
                    H.check(H.lib().vsiq_lsq_fold_multi(fold, 1, H.stream_of(torch.device(DEV))), "vsiq_lsq_fold_multi")
                    G.assert_bitwise_f32(npy(gx), gxo, f"grad_x {what}")
                    G.assert_bitwise_f32(npy(gxp), gxo, f"grad_x (records only) {what}")
                    for got in (npy(grads), npy(out)):
                        assert got[0] == pytest.approx(gso, rel=1e-9, abs=1e-12), what
                        if zpl:
                            assert got[1] == pytest.approx(gzo, rel=1e-9, abs=1e-12), what


def test_lsq_bwd_part_one_round_sizes():
    """K4d's gated one-round grids (2 groups per lane up to 48M elements), by size."""
    for n in ONE_ROUND:
        xc, xd = view("x", n, "vec")
        gc, gd = view("g", n, "vec")
        _, gxo, _, _ = O.lsq_forward_backward(npy(xc), npy(gc), S, Z, QMIN, QMAX, 1.0)
        rec = torch.empty(2 * int(H.lib().vsiq_lsq_part_records(H.c_i64(n))), dtype=torch.float64, device=DEV)
        G.assert_bitwise_f32(npy(lsq_backward_part(gd, xd, S, Z, QMIN, QMAX, False, None, rec)[0]), gxo, f"grad_x {n}")


# --------------------------------------------------------------------------- K6
# Axis 0, rows in registers: NV = 1 / 2 / 3 / 5 / 9 groups per lane by cdiv(cdiv(rowlen, 4), 256) <= NV;
# both ends of each range (rows of 256 .. 2304 groups take this form).
PCR_GROUPS = (256, 257, 512, 513, 768, 769, 1280, 1281, 2304)


def _pc_lsq(shape, axis, zpl, what):
    rng = np.random.default_rng(sum(shape))
    x = (rng.standard_normal(shape) * 2).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    C = shape[axis]
    s = rng.uniform(0.01, 0.1, C)
    z = np.rint(rng.uniform(0, 255, C)) + 0.2 if zpl else np.zeros(C)
    gscale = (255 * x.size / C) ** -0.5
    sd = torch.tensor(s, dtype=torch.float64, device=DEV)
    zd = torch.tensor(z, dtype=torch.float64, device=DEV)
    want = O.pc_lsq_forward_backward(x, g, s, z, 0, 255, gscale, axis=axis, learn_zp=zpl)
    for nt in (1, 0):
        with tuned(NONTEMPORAL=nt):
            gx, gs, gz = FQ.pc_lsq_backward(torch.from_numpy(g).to(DEV), torch.from_numpy(x).to(DEV), sd, zd, 0, 255,
                                            gscale, zpl, axis)
        G.assert_bitwise_f32(npy(gx), want[1], f"grad_x {what} nt={nt}")
        np.testing.assert_allclose(npy(gs), want[2], rtol=1e-9, atol=1e-12)
        if zpl:
            np.testing.assert_allclose(npy(gz), want[3], rtol=1e-9, atol=1e-12)
    return torch.from_numpy(g).to(DEV), torch.from_numpy(x).to(DEV), sd, zd, gscale, (npy(gx), npy(gs), npy(gz))


@pytest.mark.parametrize("zpl", [False, True])
@pytest.mark.parametrize("vec", [True, False])
def test_pc_lsq_bwd_rows_in_registers(vec, zpl):
    """launch_pcr_lsq: NV x learnable zero point x four (VEC, NT) pairs; 3 rows each."""
    for ng in PCR_GROUPS:
        _pc_lsq((3, 4 * ng if vec else 4 * ng - 1), 0, zpl, (ng, vec, zpl))


@pytest.mark.parametrize("zpl", [False, True])
def test_pc_lsq_bwd_channel_columns(zpl):
    """launch_pcc_lsq (NT x learnable zero point, the fold in the launch), the packed-rows form and the
    per-row form (four (VEC, NT) pairs x learnable zero point each)."""
    g, x, s, z, gscale, one = _pc_lsq((100, 8, 10, 10), 1, zpl, ("columns", zpl))
    # the same with the separate fold launch (vsiq_pcm_lsq_bwd_f32: no counters): every output bit for bit
    gx, gs, gz = torch.empty_like(g), torch.empty_like(s), torch.empty_like(z)
    ws = torch.empty(int(H.lib().vsiq_pcm_workspace_doubles(800, 100)), dtype=torch.float64, device=DEV)
    for nt in (1, 0):
        with tuned(NONTEMPORAL=nt):
            rc = H.lib().vsiq_pcm_lsq_bwd_f32(H.ptr(g), H.ptr(x), H.ptr(gx), H.c_i64(800), H.c_i64(100), H.c_i64(8),
                                              H.ptr(s), H.ptr(z), int(zpl), 0, 255, gscale, H.ptr(gs), H.ptr(gz),
                                              H.ptr(ws), H.c_i64(ws.numel()), H.stream_of(torch.device(DEV)))
        assert rc == 0
        for a, b in zip((gx, gs, gz), one):
            np.testing.assert_array_equal(npy(a), b)
    with tuned(PC_PACKED=2):
        _pc_lsq((16, 32, 10, 10), 1, zpl, ("packed", zpl))
    with tuned(PC_PACKED=0):
        _pc_lsq((16, 8, 10, 10), 1, zpl, ("rows", zpl))
        _pc_lsq((5, 3, 7, 3), 1, zpl, ("rows tail", zpl))


# --------------------------------------------------------------------------- activation alone, K11
@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("lay", LAYS)
def test_act_fwd_bwd(lay, nt):
    """launch_act: forward / backward x three (VEC, NT) pairs x relu / silu."""
    n = sized(5000, lay)
    xc, xd = view("x", n, lay)
    gc, gd = view("g", n, lay)
    with tuned(NONTEMPORAL=nt):
        for act in ("relu", "silu"):
            xg = xd.detach().requires_grad_(True)
            y = FQ.ActivationFn.apply(xg, act)
            gx, = torch.autograd.grad(y, xg, gd)
            G.assert_bitwise_f32(npy(y), act_fwd(n, lay, act), f"y {lay} {act}")
            G.assert_bitwise_f32(npy(gx), O.act_backward(npy(gc), npy(xc), act, REF()), f"grad {lay} {act}")


@pytest.mark.parametrize("vec", [8, 16])
@pytest.mark.parametrize("act", ACTS)
def test_torch_mean_and_std(act, vec):
    """K11 (vector width 8 / 16 x act) and its std pass (act): the means bit for bit the host loop's."""
    n = 300_003
    xc, xd = view("x", n, "tail")
    want = npy(FQ.torch_mean(xc, act=act, ref=(vec, 8)))
    got = npy(FQ.torch_mean(xd, act=act, ref=(vec, 8)))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (act, vec)
    st = npy(FQ.torch_stats(xd, act=act, ref=(vec, 8)))
    assert (np.float32(st[0]), np.float32(st[1])) == (want[2], want[3]), (act, vec)
    assert st[2] == pytest.approx(O.collect_stats(act_fwd(n, "tail", act))[2], rel=1e-6)
