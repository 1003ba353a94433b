"""Shared pieces of the learnable group-wise (PerGroupLSQQuantizer) tests (test_pg_learn_cpu.py,
test_gpu_pg_learn.py).

The oracle is ``oracle.fakequant_np.lsq_forward_backward`` on each group's slice of x and g with
that group's (scale, zp).  ``terms`` recomputes the fp32 terms the gradients sum (oracle
fq_forward on the whole tensor with every element's group qparams), so that T = sum |term| per
group is known: at most 512 fp32-exact terms are added in f64, two addition orders differ by at
most n * 2^-52 * T, hence the bar

    |got - want| <= 2^-43 * gscale * T + 2^-50 * |want|

(the second term covers the final multiply) holds for every order of the sum."""
import numpy as np
import torch

from oracle import fakequant_np as O
from tests import pg_common as P

F32 = np.float32
GSCALE = 0.0371   # any factor: the quantizer's own (qmax * G) ** -0.5 is checked in the manager tests


def groups_of(rowlen, G):
    return -(-rowlen // G)


def make_qparams(x, G, symmetric, qmin, qmax, learn_zp, seed=5):
    """[rows, ngr] f64 (scale, zp) near the observed ones, the scale off by up to 30 % so that the
    clamp cuts at both ends; a learned zero point is no integer, with x.5 ties in every fifth group
    and a rint outside [qmin, qmax] (below, above) in groups 1 and 2 mod 7."""
    from vsiquantization_amd.fakequant import per_group_observe_fq
    r = per_group_observe_fq(x.detach().cpu(), group_size=G, symmetric=symmetric, qmin=qmin, qmax=qmax,
                             obs_bits=(qmax - qmin + 1).bit_length() - 1)   # on the quantizer's own grid
    gen = torch.Generator().manual_seed(seed)
    s = r["scale"] * (0.7 + 0.6 * torch.rand(r["scale"].shape, generator=gen, dtype=torch.float64))
    s = torch.where(s > 0, s, torch.full_like(s, 1e-3))
    z = r["zp"].clone()
    if learn_zp:
        z = z + (torch.rand(z.shape, generator=gen, dtype=torch.float64) - 0.5) * 3
        flat = z.view(-1)
        idx = torch.arange(flat.numel())
        flat[idx % 5 == 0] = torch.floor(flat[idx % 5 == 0]) + 0.5
        flat[idx % 7 == 1] = qmin - 3.2
        flat[idx % 7 == 2] = qmax + 2.5
    return s, z


def zp_in_range(z, qmin, qmax):
    zr = torch.round(z)   # half to even, as rint
    return (zr >= qmin) & (zr <= qmax)


def _elementwise(v, rowlen, G):
    return np.repeat(np.asarray(v, np.float64), G, axis=1)[:, :rowlen]


def terms(x, g, s, z, qmin, qmax, learn_zp, G):
    """Per group: T_s = sum |t1| + |t2|, T_z = sum |gm| + |g*s| (f64 [rows, ngr]) and whether every
    grad_scale / every grad_zp term of the group is finite (bool [rows, ngr] each)."""
    xa = x.detach().cpu().numpy().reshape(x.shape[0], -1)
    ga = g.detach().cpu().numpy().reshape(xa.shape)
    rows, rowlen = xa.shape
    zn = z.detach().cpu().numpy().astype(np.float64).reshape(rows, -1)
    if learn_zp:
        zn = np.clip(np.rint(zn), qmin, qmax)
    se = F32(_elementwise(s.detach().cpu().numpy().reshape(rows, -1), rowlen, G))
    ze = F32(_elementwise(zn, rowlen, G))
    _, q, mask = O.fq_forward(xa, se, ze, qmin, qmax)
    with np.errstate(all="ignore"):
        gq = (ga * se).astype(F32)
        gm = np.where(mask, gq, F32(0.0)).astype(F32)
        t1 = (ga * (q - ze).astype(F32)).astype(F32)
        t2 = ((-gm).astype(F32) * ((xa / se).astype(F32) / se).astype(F32)).astype(F32)
        starts = np.arange(0, rowlen, G)
        a = lambda v: np.add.reduceat(np.abs(v.astype(np.float64)), starts, axis=1)   # noqa: E731
        Ts, Tz = a(t1) + a(t2), a(gm) + a(gq)
    return Ts, Tz, np.isfinite(Ts), np.isfinite(Tz)


def oracle(x, g, s, z, qmin, qmax, gscale, learn_zp, G):
    """dict(y, gx fp32 [rows, rowlen]; gs, gz f64 [rows, ngr]) from lsq_forward_backward group by
    group (gz zeros when the zero point is not learned)."""
    xa = x.detach().cpu().numpy().reshape(x.shape[0], -1)
    ga = g.detach().cpu().numpy().reshape(xa.shape)
    rows, rowlen = xa.shape
    ngr = groups_of(rowlen, G)
    sn, zn = s.detach().cpu().numpy().reshape(rows, ngr), z.detach().cpu().numpy().reshape(rows, ngr)
    y, gx = np.empty_like(xa), np.empty_like(xa)
    gs, gz = np.zeros((rows, ngr)), np.zeros((rows, ngr))
    for r in range(rows):
        for j in range(ngr):
            c = slice(j * G, min((j + 1) * G, rowlen))
            y[r, c], gx[r, c], gs[r, j], v = O.lsq_forward_backward(xa[r, c], ga[r, c], float(sn[r, j]),
                                                                    float(zn[r, j]), qmin, qmax, gscale,
                                                                    learn_zp=bool(learn_zp))
            if learn_zp:
                gz[r, j] = v
    return dict(y=y, gx=gx, gs=gs, gz=gz)


def same_f32(t, a):
    """A float32 tensor against a numpy array, bit for bit."""
    return np.array_equal(t.detach().cpu().numpy().reshape(a.shape).view(np.uint32), a.view(np.uint32))


def within_bar(got, want, T, gscale, where=None):
    """The module docstring's bar on the groups of ``where`` (default: all); returns the groups
    that miss it."""
    got = got.detach().cpu().numpy().reshape(want.shape) if isinstance(got, torch.Tensor) else got
    with np.errstate(all="ignore"):
        bad = ~(np.abs(got - want) <= 2.0 ** -43 * gscale * T + 2.0 ** -50 * np.abs(want))
    if where is not None:
        bad &= where
    return np.argwhere(bad)


def same_nonfinite(got, want):
    """Non-finite in the same way: NaN where ``want`` is NaN, else an infinity of the same sign."""
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.all(np.where(np.isnan(want), np.isnan(got), got == want)))


def run(x, g, s, z, qmin, qmax, gscale, learn_zp, G):
    """The route under test on x's device: the forward, then the backward launch."""
    from vsiquantization_amd.fakequant import per_group_fake_quant, pg_lsq_backward
    y = per_group_fake_quant(x, s, z, qmin, qmax, group_size=G, zp_round=bool(learn_zp))[0]
    gx, gs, gz = pg_lsq_backward(g, x, s, z, qmin, qmax, gscale, learn_zp, G)
    return dict(y=y, gx=gx, gs=gs, gz=gz)


def check_against_oracle(got, x, g, s, z, qmin, qmax, gscale, learn_zp, G, tag):
    """y and gx bit for bit, gs and gz inside the bar on every group (finite data)."""
    want = oracle(x, g, s, z, qmin, qmax, gscale, learn_zp, G)
    Ts, Tz, fin_s, fin_z = terms(x, g, s, z, qmin, qmax, learn_zp, G)
    assert fin_s.all() and fin_z.all(), tag
    assert same_f32(got["y"], want["y"]), (tag, "y")
    assert same_f32(got["gx"], want["gx"]), (tag, "gx")
    assert got["gs"].dtype == torch.float64 and tuple(got["gs"].shape) == want["gs"].shape, tag
    assert not len(within_bar(got["gs"], want["gs"], Ts, gscale)), (tag, "grad_scale")
    assert not len(within_bar(got["gz"], want["gz"], Tz, gscale)), (tag, "grad_zp")
    if learn_zp:   # ClampBackward of the rounded zero point: exactly 0 outside the grid
        out = ~zp_in_range(z, qmin, qmax)
        assert bool((got["gz"].cpu()[out] == 0).all()), (tag, "grad_zp outside the grid")
    else:
        assert bool((got["gz"] == 0).all()), (tag, "grad_zp not learned")
    return want


def check_against_parent_route(got, x, g, s, z, qmin, qmax, gscale, learn_zp, G, tag):
    """Where rowlen % G == 0: the route that existed before, PerChannelLearnFn on x.view(-1, G).
    y and gx bit for bit; its gradients are sums of the same terms in another order."""
    from vsiquantization_amd.fakequant import PerChannelLearnFn
    rows = x.shape[0]
    rowlen = x.numel() // rows
    assert rowlen % G == 0
    xp = x.detach().reshape(-1, G).clone().requires_grad_(True)
    sp = s.detach().reshape(-1).to(x.device).clone().requires_grad_(True)
    zp = z.detach().reshape(-1).to(x.device).clone().requires_grad_(bool(learn_zp))
    y = PerChannelLearnFn.apply(xp, sp, zp, qmin, qmax, gscale, bool(learn_zp))
    y.backward(g.reshape(-1, G))
    assert P.same_bits(y.detach().reshape(got["y"].shape), got["y"]), (tag, "parent y")
    assert P.same_bits(xp.grad.reshape(got["gx"].shape), got["gx"]), (tag, "parent gx")
    Ts, Tz, _, _ = terms(x, g, s, z, qmin, qmax, learn_zp, G)
    assert not len(within_bar(got["gs"], sp.grad.cpu().numpy().reshape(Ts.shape), Ts, gscale)), (tag, "parent gs")
    if learn_zp:
        assert not len(within_bar(got["gz"], zp.grad.cpu().numpy().reshape(Tz.shape), Tz, gscale)), (tag, "parent gz")


def check_special(got, host, x, g, s, z, qmin, qmax, gscale, learn_zp, G, tag):
    """Data with non-finite groups.  ``got`` against the host loop ``host``: y and gx bit for bit
    everywhere; a group with a non-finite grad_scale term has a grad_scale non-finite in the host
    loop's way; every group whose terms are finite -- the non-finite groups' neighbours among them
    -- meets the finite bar against the oracle.  grad_zp of a group whose zero-point terms are not
    finite (a non-finite g) is not pinned."""
    Ts, Tz, fin_s, fin_z = terms(x, g, s, z, qmin, qmax, learn_zp, G)
    assert (~fin_s).any() and fin_s.any() and (~fin_z).any(), tag
    assert P.same_bits(got["y"].cpu(), host["y"]) and P.same_bits(got["gx"].cpu(), host["gx"]), tag
    hs, ds = host["gs"].numpy(), got["gs"].cpu().numpy()
    assert not np.isfinite(hs[~fin_s]).any(), (tag, "the host loop's sums of non-finite terms")
    assert same_nonfinite(ds[~fin_s], hs[~fin_s]), (tag, "grad_scale of a non-finite group")
    with np.errstate(all="ignore"):
        want = oracle(x, g, s, z, qmin, qmax, gscale, learn_zp, G)
    assert not len(within_bar(got["gs"], want["gs"], Ts, gscale, fin_s)), (tag, "leak into grad_scale")
    assert not len(within_bar(got["gz"], want["gz"], Tz, gscale, fin_z)), (tag, "leak into grad_zp")


def special_case(G, extra, seed=11):
    """(x, g) [2, 8 * G + extra]: pg_common.with_special_groups' x (a NaN in group 1, a +Inf in
    group 3, zeros in group 5, a constant group 6) and a g with a -Inf in group 7 and a NaN in the
    short last group 8, each next to ordinary groups."""
    x = P.with_special_groups(P.weights(2, 8 * G + extra, seed), G)
    g = P.weights(2, 8 * G + extra, seed + 1) * 20
    g[:, 7 * G + 5] = float("-inf")
    g[1, 8 * G + 2] = float("nan")
    return x, g
