"""The fake-quant path for CPU tensors: native host loops in the same library
(csrc/k_host.hip, vsiq_host_* in include/vsiq.h) -- the reference's own environment
(BASELINE C1: UniformQuantizer / MinMaxObserver on CPU tensors).  The elementwise
outputs (y, integer codes, masks, grad_x), min / max and the f64 qparams are the HIP
kernels' bit for bit (IEEE fp32 division, rint, NaN-propagating clamp, f64 qparams,
torch CPU's SiLU).  The f64 sums (mean|x|, mean, std, scale / zero-point gradients) are
summed in 16 lanes per 64K chunk, folded in lane then chunk order -- the same bits with
or without AVX-512 (VSIQ_HOST_SIMD=0) and for any thread count, but a different order
from the GPU's tree (equal to it within the f64 rounding of the sum).  This is not a
fallback for CUDA tensors: a CUDA tensor never comes here, and a missing library raises
like every other op.

Only this module calls a vsiq_host_* entry point, and it decides nothing: fakequant.py
sends a CPU tensor here (``is_host``), one plain function per op, and owns the autograd
Functions of both sides.
"""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import _hip as H
from ._hip import qden


def is_host(x) -> bool:
    """A CPU float32 tensor (the host path's input)."""
    return isinstance(x, torch.Tensor) and x.device.type == "cpu" and x.dtype == torch.float32


def _i64(n):
    return H.c_i64(int(n))


def _num(v) -> float:
    if isinstance(v, torch.Tensor):
        if v.numel() != 1:
            raise ValueError(f"expected a scalar qparam, got shape {tuple(v.shape)}")
        return float(v.detach().reshape(()).item())
    if isinstance(v, (numbers.Real, np.floating, np.integer)):
        return float(v)
    raise TypeError(f"unsupported qparam type {type(v).__name__}")


def _f32(x, what="x"):
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: only float32 is supported by the fake-quant path, got {x.dtype}")
    return x.contiguous()


def _check_state(*states):
    """The running state the host loops update in place: contiguous CPU float32, or None."""
    for r in states:
        if r is not None and (r.device.type != "cpu" or r.dtype != torch.float32 or not r.is_contiguous()):
            raise ValueError("host observe: the running state must be a contiguous CPU float32 tensor")


def fake_quant(x, scale, zero_point, qmin, qmax, *, zp_round=False, qp=None, want_mask=False, want_codes=False,
               discrete=False, act=None):
    """Host counterpart of fakequant.fake_quant: (y, mask uint8 | None, codes | None)."""
    x = _f32(x)
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8) if want_mask else None
    codes = H.codes_buffer(x.shape, qmin, "cpu") if want_codes else None
    if qp is not None:
        qp = qp.detach().to("cpu", torch.float64).contiguous()
        s = z = 0.0
    else:
        s, z = _num(scale), _num(zero_point)
    rc = H.lib().vsiq_host_fq_fwd_f32(H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(mask), _i64(x.numel()), H.act_code(act),
                                      H.ptr(qp), s, z, int(bool(zp_round)), int(bool(discrete)), int(qmin), int(qmax))
    H.check(rc, "vsiq_host_fq_fwd_f32")
    return y, mask, codes


def ste_backward(g, mask, scale, *, pre=None, act=None):
    """Host counterpart of fakequant.ste_backward, per-tensor form (``mask``: fake_quant's
    bytes): gx = (mask ? g*s : 0) / s, then the activation's backward at ``pre``."""
    g = _f32(g, "grad_output")
    code = H.act_code(act)
    pre = _f32(pre, "pre-activation") if code != H.ACT_NONE else None
    gx = torch.empty_like(g)
    rc = H.lib().vsiq_host_ste_bwd_f32(H.ptr(g), H.ptr(mask), H.ptr(pre), H.ptr(gx), _i64(g.numel()), code,
                                       _num(scale))
    H.check(rc, "vsiq_host_ste_bwd_f32")
    return gx


def lsq_backward(g, x, scale, zero_point, qmin, qmax, gscale, learn_zp, act=None):
    """Host counterpart of fakequant.lsq_backward (uniform.py:47-56): grad_x and f64[2], the
    closed-form scale / zero-point gradients times the ScaleGradient factor."""
    g = _f32(g, "grad_output")
    x = _f32(x)
    gx = torch.empty_like(g)
    grads = torch.empty(2, dtype=torch.float64)
    rc = H.lib().vsiq_host_lsq_bwd_f32(H.ptr(g), H.ptr(x), H.ptr(gx), _i64(g.numel()), H.act_code(act), _num(scale),
                                       _num(zero_point), int(learn_zp), int(qmin), int(qmax), float(gscale),
                                       H.ptr(grads))
    H.check(rc, "vsiq_host_lsq_bwd_f32")
    return gx, grads


def observe_tensor(x, *, symmetric, num_bits=8, eps=1e-8, run_minmax=None, want_qp=True, want_stats=True,
                   act=None):
    """Host counterpart of fakequant.observe_tensor: one pass -> running update (fp32[2]
    CPU state) -> f64 qparams record, stats record."""
    x = _f32(x)
    if x.numel() == 0:
        raise H.empty_error()
    qp = torch.empty(H.QP_LEN, dtype=torch.float64) if want_qp else None
    st = torch.empty(H.ST_LEN, dtype=torch.float64) if want_stats else None
    _check_state(run_minmax)
    rc = H.lib().vsiq_host_observe_f32(H.ptr(x), _i64(x.numel()), H.act_code(act), H.ptr(st), H.ptr(run_minmax),
                                       H.ptr(qp), int(bool(symmetric)), qden(symmetric, num_bits, eps), float(eps))
    H.check(rc, "vsiq_host_observe_f32")
    return qp, st


def observe_percentile(x, *, symmetric, num_bits=8, eps=1e-8, run_minmax=None, tail, bins=2048, act=None):
    """Host counterpart of fakequant.observe_percentile: the host observer pass for the
    stats record, then the host histogram loop -> (qp, stats, clip f64[2])."""
    _, st = observe_tensor(x, symmetric=symmetric, num_bits=num_bits, eps=eps, run_minmax=None, want_qp=False,
                           act=act)
    x = _f32(x)
    _check_state(run_minmax)
    qp = torch.empty(H.QP_LEN, dtype=torch.float64)
    clip = torch.empty(2, dtype=torch.float64)
    hist = torch.zeros(int(bins), dtype=torch.int64)
    rc = H.lib().vsiq_host_observe_hist_f32(H.ptr(x), _i64(x.numel()), H.act_code(act), H.ptr(st), int(bins),
                                            float(tail), H.ptr(hist), _i64(hist.numel()), H.ptr(run_minmax),
                                            H.ptr(qp), H.ptr(clip), int(bool(symmetric)),
                                            qden(symmetric, num_bits, eps), float(eps))
    H.check(rc, "vsiq_host_observe_hist_f32")
    return qp, st, clip


def observe_mse(x, *, symmetric, num_bits=8, eps=1e-8, run_minmax=None, ratios, qmin, qmax, act=None):
    """Host counterpart of fakequant.observe_mse (which has validated ``ratios`` and the
    grid): the host observer pass for the stats record, then the host search loop ->
    (qp, stats, clip f64[2], err f64[len(ratios)], pick int32[1])."""
    _, st = observe_tensor(x, symmetric=symmetric, num_bits=num_bits, eps=eps, run_minmax=None, want_qp=False,
                           act=act)
    x = _f32(x)
    _check_state(run_minmax)
    qp = torch.empty(H.QP_LEN, dtype=torch.float64)
    clip = torch.empty(2, dtype=torch.float64)
    err = torch.empty(len(ratios), dtype=torch.float64)
    pick = torch.empty(1, dtype=torch.int32)
    table = (H.c_d * len(ratios))(*ratios)
    rc = H.lib().vsiq_host_observe_mse_f32(H.ptr(x), _i64(x.numel()), H.act_code(act), H.ptr(st), table,
                                           len(ratios), int(qmin), int(qmax), H.ptr(run_minmax), H.ptr(qp),
                                           H.ptr(clip), H.ptr(err), H.ptr(pick), int(bool(symmetric)),
                                           qden(symmetric, num_bits, eps), float(eps))
    H.check(rc, "vsiq_host_observe_mse_f32")
    return qp, st, clip, err, pick


def torch_mean(x, act, vec, threads):
    """Host counterpart of fakequant.torch_mean (which has resolved the layout): fp32[4]."""
    x = x.contiguous()
    out = torch.empty(4, dtype=torch.float32)
    rc = H.lib().vsiq_host_torch_mean_f32(H.ptr(x), _i64(x.numel()), H.act_code(act), vec, threads, H.ptr(out))
    H.check(rc, "vsiq_host_torch_mean_f32")
    return out


# --------------------------------------------------------------------------- per-channel
def _rows(x):
    C = x.shape[0] if x.dim() > 0 else 1
    if C == 0 or x.numel() == 0:
        raise H.empty_error()
    return C, x.numel() // C


def _pc_view(x, axis):
    """(rows, rowlen, channels) of per-channel ``axis`` 0 ([C, ...] weights: one row per
    channel) or 1 ([N, C, ...] activations: N * C rows, row r in channel r % C) -- the
    device path's view (fakequant._pc_view)."""
    if axis == 0:
        C, rowlen = _rows(x)
        return C, rowlen, C
    if axis != 1 or x.dim() < 2:
        raise ValueError(f"per-channel axis must be 0 or 1 of a tensor with more dims, got {axis}")
    C, rows = x.shape[1], x.shape[0] * x.shape[1]
    if rows == 0 or x.numel() == 0:
        raise H.empty_error()
    return rows, x.numel() // rows, C


def _row_f64(v, C, what):
    t = (v.detach() if isinstance(v, torch.Tensor) else torch.tensor(float(v))).to("cpu", torch.float64)
    t = t.reshape(-1)
    if t.numel() == 1 and C > 1:
        t = t.expand(C)
    if t.numel() != C:
        raise RuntimeError(f"per-channel {what} has {t.numel()} entries, the tensor has {C} channels")
    return t.contiguous()


def pc_observe_fq(x, *, symmetric, qmin, qmax, obs_bits=8, eps=1e-8, run_min=None, run_max=None,
                  quantize=True, want_mask=False, want_row_stats=False):
    """Host counterpart of fakequant.per_channel_observe_fq (K3): each out-channel row W[c]
    observed (running state per row) and fake-quantized with its own f64 qparams, the
    per-tensor host code on each row.  Same dict as the device function."""
    x = _f32(x)
    C, rowlen = _rows(x)
    run_min, run_max, y, scale, zp, rstats = H.pc_observe_buffers(x, C, run_min, run_max, quantize, want_row_stats)
    _check_state(run_min, run_max)
    mask = torch.empty(x.shape, dtype=torch.uint8) if (want_mask and quantize) else None
    rc = H.lib().vsiq_host_pc_observe_fq_f32(H.ptr(x), H.ptr(y), H.ptr(mask), _i64(C), _i64(rowlen), H.ptr(run_min),
                                             H.ptr(run_max), H.ptr(scale), H.ptr(zp), H.ptr(rstats),
                                             int(bool(symmetric)), qden(symmetric, obs_bits, eps), float(eps),
                                             int(qmin), int(qmax))
    H.check(rc, "vsiq_host_pc_observe_fq_f32")
    return dict(y=y, scale=scale, zp=zp, run_min=run_min, run_max=run_max, mask=mask, codes=None,
                row_stats=rstats)


def pc_observe_mse(x, *, symmetric, qmin, qmax, num_bits=8, eps=1e-8, run_min=None, run_max=None, ratios,
                   quantize=True, want_row_stats=False, want_mask=False):
    """Host counterpart of fakequant.per_channel_observe_mse (which has validated ``ratios``
    and the grid): the host MSE loop on each row W[c] with its own running state, then the
    host per-channel fake quant with the qparams returned.  Same dict as the device function."""
    x = _f32(x)
    C, rowlen = _rows(x)
    run_min, run_max, y, scale, zp, rstats = H.pc_observe_buffers(x, C, run_min, run_max, quantize, want_row_stats)
    _check_state(run_min, run_max)
    mask = torch.empty(x.shape, dtype=torch.uint8) if (want_mask and quantize) else None
    clip = torch.empty(C, 2, dtype=torch.float64)
    err = torch.empty(C, len(ratios), dtype=torch.float64)
    pick = torch.empty(C, dtype=torch.int32)
    table = (H.c_d * len(ratios))(*ratios)
    rc = H.lib().vsiq_host_pc_observe_mse_f32(H.ptr(x), H.ptr(y), H.ptr(mask), _i64(C), _i64(rowlen), table,
                                              len(ratios), H.ptr(run_min), H.ptr(run_max), H.ptr(scale), H.ptr(zp),
                                              H.ptr(clip), H.ptr(err), H.ptr(pick), H.ptr(rstats),
                                              int(bool(symmetric)), int(qmin), int(qmax),
                                              qden(symmetric, num_bits, eps), float(eps))
    H.check(rc, "vsiq_host_pc_observe_mse_f32")
    return dict(y=y, scale=scale, zp=zp, run_min=run_min, run_max=run_max, mask=mask, codes=None, row_stats=rstats,
                clip=clip, err=err, pick=pick)


def pc_fake_quant(x, scale, zp, qmin, qmax, *, zp_round=False, want_mask=False, axis=0):
    """Per-channel fake quant with given [C] qparams along ``axis`` 0 or 1 on the host:
    (y, mask | None)."""
    x = _f32(x)
    rows, rowlen, C = _pc_view(x, axis)
    s = _row_f64(scale, C, "scale")
    z = _row_f64(zp, C, "zero point") if zp is not None else None
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8) if want_mask else None
    rc = H.lib().vsiq_host_pcm_fq_fwd_f32(H.ptr(x), H.ptr(y), H.ptr(mask), _i64(rows), _i64(rowlen), _i64(C),
                                          H.ptr(s), H.ptr(z), int(bool(zp_round)), int(qmin), int(qmax))
    H.check(rc, "vsiq_host_pcm_fq_fwd_f32")
    return y, mask


def pc_ste_backward(g, mask, scale, axis=0):
    """Host counterpart of fakequant.pc_ste_backward (``mask``: pc_fake_quant's bytes)."""
    g = _f32(g, "grad_output")
    rows, rowlen, C = _pc_view(g, axis)
    s = _row_f64(scale, C, "scale")
    gx = torch.empty_like(g)
    rc = H.lib().vsiq_host_pcm_ste_bwd_f32(H.ptr(g), H.ptr(mask), H.ptr(gx), _i64(rows), _i64(rowlen), _i64(C),
                                           H.ptr(s))
    H.check(rc, "vsiq_host_pcm_ste_bwd_f32")
    return gx


def pg_observe_fq(x, group, *, symmetric, qmin, qmax, obs_bits=8, eps=1e-8, run_min=None, run_max=None,
                  quantize=True, want_mask=False):
    """Host counterpart of fakequant.per_group_observe_fq (which has checked ``group``): each
    group of ``group`` consecutive elements of a row observed on its own running state and
    fake-quantized with its own f64 qparams.  Same dict as the device function (byte mask, no codes)."""
    x = _f32(x)
    rows, rowlen = _rows(x)
    ngr = -(-rowlen // group)
    run_min, run_max, y, scale, zp = H.pg_observe_buffers(x, rows, ngr, run_min, run_max, quantize)
    _check_state(run_min, run_max)
    mask = torch.empty(x.shape, dtype=torch.uint8) if (want_mask and quantize) else None
    rc = H.lib().vsiq_host_pg_observe_fq_f32(H.ptr(x), H.ptr(y), H.ptr(mask), _i64(rows), _i64(rowlen), _i64(group),
                                             H.ptr(run_min), H.ptr(run_max), H.ptr(scale), H.ptr(zp),
                                             int(bool(symmetric)), qden(symmetric, obs_bits, eps), float(eps),
                                             int(qmin), int(qmax))
    H.check(rc, "vsiq_host_pg_observe_fq_f32")
    return dict(y=y, scale=scale, zp=zp, run_min=run_min, run_max=run_max, mask=mask, codes=None)


def pg_fake_quant(x, scale, zp, group, qmin, qmax, *, zp_round=False, want_mask=False):
    """Group-wise fake quant with given [rows, ngr] f64 CPU qparams on the host: (y, mask | None)."""
    x = _f32(x)
    rows, rowlen = _rows(x)
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8) if want_mask else None
    rc = H.lib().vsiq_host_pg_fq_fwd_f32(H.ptr(x), H.ptr(y), H.ptr(mask), _i64(rows), _i64(rowlen), _i64(group),
                                         H.ptr(scale), H.ptr(zp), int(bool(zp_round)), int(qmin), int(qmax))
    H.check(rc, "vsiq_host_pg_fq_fwd_f32")
    return y, mask


def pg_ste_backward(g, mask, scale, group):
    """Host counterpart of fakequant.pg_ste_backward (``mask``: pg_fake_quant's bytes; ``scale``
    f64 [rows, ngr] on the CPU)."""
    g = _f32(g, "grad_output")
    rows, rowlen = _rows(g)
    gx = torch.empty_like(g)
    rc = H.lib().vsiq_host_pg_ste_bwd_f32(H.ptr(g), H.ptr(mask), H.ptr(gx), _i64(rows), _i64(rowlen), _i64(group),
                                          H.ptr(scale))
    H.check(rc, "vsiq_host_pg_ste_bwd_f32")
    return gx


def pg_lsq_backward(g, x, scale, zp, group, qmin, qmax, gscale, learn_zp):
    """Host counterpart of fakequant.pg_lsq_backward (``scale`` / ``zp`` f64 [rows, ngr] on the
    CPU): each group the per-tensor learnable host loop on its elements alone; (grad_x,
    grad_scale f64 [rows, ngr], grad_zp f64 [rows, ngr])."""
    g = _f32(g, "grad_output")
    x = _f32(x)
    rows, rowlen = _rows(g)
    gx = torch.empty_like(g)
    gs = torch.empty_like(scale)
    gz = torch.empty_like(scale)
    rc = H.lib().vsiq_host_pg_lsq_bwd_f32(H.ptr(g), H.ptr(x), H.ptr(gx), _i64(rows), _i64(rowlen), _i64(group),
                                          H.ptr(scale), H.ptr(zp), int(bool(learn_zp)), int(qmin), int(qmax),
                                          float(gscale), H.ptr(gs), H.ptr(gz))
    H.check(rc, "vsiq_host_pg_lsq_bwd_f32")
    return gx, gs, gz


def pc_lsq_backward(g, x, scale, zp, qmin, qmax, gscale, learn_zp, axis=0):
    """Host counterpart of fakequant.pc_lsq_backward (``axis`` 0: [C, ...] weights, 1:
    [N, C, ...] activations -- LSQFakeQuantize): each row the per-tensor learnable host
    path with its channel's scale / zero point; (grad_x, grad_scale f64 [C], grad_zp f64 [C]),
    the f64 sums over each channel's rows times gscale."""
    g = _f32(g, "grad_output")
    x = _f32(x)
    rows, rowlen, C = _pc_view(x, axis)
    s = _row_f64(scale, C, "scale")
    z = _row_f64(zp, C, "zero point") if zp is not None else None
    gx = torch.empty_like(g)
    gs = torch.empty(C, dtype=torch.float64)
    gz = torch.empty(C, dtype=torch.float64)
    rc = H.lib().vsiq_host_pcm_lsq_bwd_f32(H.ptr(g), H.ptr(x), H.ptr(gx), _i64(rows), _i64(rowlen), _i64(C),
                                           H.ptr(s), H.ptr(z), int(bool(learn_zp)), int(qmin), int(qmax),
                                           float(gscale), H.ptr(gs), H.ptr(gz))
    H.check(rc, "vsiq_host_pcm_lsq_bwd_f32")
    return gx, gs, gz


# --------------------------------------------------------------------------- export
def quantize_pack(x, scale, zp, nq, rows, rowlen, qmin, qmax, bits, zp_round):
    """Host counterpart of fakequant.quantize_pack (which has checked the arguments):
    (data uint8 [rows, row_bytes], qparams fp32 [nq, 2]) from f64 [nq] CPU qparams."""
    row_bytes = int(H.lib().vsiq_packed_row_bytes(_i64(rowlen), int(bits)))
    data = torch.empty((rows, row_bytes), dtype=torch.uint8)
    qparams = torch.empty((nq, 2), dtype=torch.float32)
    rc = H.lib().vsiq_host_quantize_pack_f32(H.ptr(x), H.ptr(data), H.ptr(qparams), _i64(rows), _i64(rowlen),
                                             H.ptr(scale), H.ptr(zp), _i64(nq), int(bool(zp_round)), int(qmin),
                                             int(qmax), int(bits))
    H.check(rc, "vsiq_host_quantize_pack_f32")
    return data, qparams


def unpack_dequant(data, qparams, shape, rows, rowlen, qmin, bits, want_codes):
    """Host counterpart of fakequant.unpack_dequant: (y fp32, codes | None)."""
    y = torch.empty(shape, dtype=torch.float32)
    codes = H.codes_buffer(shape, qmin, "cpu") if want_codes else None
    rc = H.lib().vsiq_host_unpack_dequant_f32(H.ptr(data), H.ptr(y), H.ptr(codes), _i64(rows), _i64(rowlen),
                                              H.ptr(qparams), _i64(qparams.shape[0]), int(qmin), int(bits))
    H.check(rc, "vsiq_host_unpack_dequant_f32")
    return y, codes


# --------------------------------------------------------------------------- AdaRound
def adaround_forward(w, V, y, reg, rows, rowlen, s, z, nq, zp_round, qmin, qmax, hard, beta):
    """Host leg of fakequant.adaround_forward (which has checked the arguments and made the
    outputs): writes y (or None) and the regulariser reg (or None)."""
    rc = H.lib().vsiq_host_adaround_fwd_f32(H.ptr(w), H.ptr(V), H.ptr(y), None, _i64(rows), _i64(rowlen), H.ptr(s),
                                            H.ptr(z), _i64(nq), int(bool(zp_round)), int(qmin), int(qmax),
                                            int(bool(hard)), beta, H.ptr(reg))
    H.check(rc, "vsiq_host_adaround_fwd_f32")


def adaround_backward(g, w, V, gv, rows, rowlen, s, z, nq, zp_round, qmin, qmax, lam, beta):
    """Host leg of fakequant.adaround_backward: writes grad_V into gv."""
    rc = H.lib().vsiq_host_adaround_bwd_f32(H.ptr(g), H.ptr(w), H.ptr(V), H.ptr(gv), _i64(rows), _i64(rowlen),
                                            H.ptr(s), H.ptr(z), _i64(nq), int(bool(zp_round)), int(qmin), int(qmax),
                                            float(lam), float(beta))
    H.check(rc, "vsiq_host_adaround_bwd_f32")


# --------------------------------------------------------------------------- MX
def mx_fake_quant(x, y, codes, scales, mask, view, fmt):
    """Host leg of fakequant.mx_fake_quant (which has checked the arguments and made the
    outputs; mask: one byte per element): ``view`` is (rows, rowlen) or (outer, channels, inner)."""
    if len(view) == 2:
        rc = H.lib().vsiq_host_mx_fq_fwd_f32(H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(scales), H.ptr(mask),
                                             _i64(view[0]), _i64(view[1]), int(fmt))
        H.check(rc, "vsiq_host_mx_fq_fwd_f32")
    else:
        rc = H.lib().vsiq_host_mx_fq_fwd_cols_f32(H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(scales), H.ptr(mask),
                                                  _i64(view[0]), _i64(view[1]), _i64(view[2]), int(fmt))
        H.check(rc, "vsiq_host_mx_fq_fwd_cols_f32")


def threads() -> int:
    """Host threads the CPU path uses (VSIQ_HOST_THREADS, else the CPUs this process may use)."""
    return int(H.lib().vsiq_host_threads())


def simd() -> bool:
    """True when the host loops run their AVX-512 form (csrc/host_simd.cpp)."""
    return bool(H.lib().vsiq_host_simd())


__all__ = ["is_host", "fake_quant", "ste_backward", "lsq_backward", "observe_tensor", "observe_percentile",
           "observe_mse", "torch_mean", "pc_observe_fq", "pc_observe_mse", "pc_fake_quant", "pc_ste_backward",
           "pc_lsq_backward", "quantize_pack", "unpack_dequant", "adaround_forward", "adaround_backward", "mx_fake_quant", "threads",
           "simd"]
