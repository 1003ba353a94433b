"""torch-facing fake-quant ops over the HIP C ABI (CPU tensors: the native host loops of
host.py, never the oracle).  This is the one module that chooses between the two: an op
with a host counterpart tests ``_host.is_host(x)`` (a CPU float32 tensor) first and hands
the call to host.py's plain function of that op, so the autograd Functions here serve both
sides and callers never branch on the device.

Each op here is one (or two) kernel launches on the tensor's current HIP
stream, no host synchronisation, and is the MI355X replacement of one chain of
eager torch ops in the reference:

  fake_quant               quantizers/uniform.py:54-55,95   (K1)
  observe_tensor           observers/minmax.py:32-88 + quantization_manager.py:66-68 (K2)
  per_channel_observe_fq   per-channel MinMax + UniformQuantizer (K3)
  per_group_observe_fq     the same on every group of 32..256 consecutive elements of a row (k_pg.hip)
  FakeQuantFixedFn         autograd of uniform.py:55,95 with fixed qparams (STE)
  FakeQuantLearnFn         autograd of uniform.py:47-56 (LSQ: ScaleGradient, STE) (K4)
  FakeQuantLearnMultiFn    FakeQuantLearnFn over many tensors in one launch each way
  observe_parts/fold_parts deferred-calibration observer (K2p) and its one-launch fold
  observe_parts_out        K2p that also writes act(x): a fused layer's calibration forward (K2o)
  mx_fake_quant            OCP MX block-scaled fake quant (MXFP4 / MXFP6 / MXFP8), CPU tensors only so far

Every op takes an optional ``act`` ("relu" / "silu", K5): the op is then applied
to act(x) without materializing it -- the fused layers' F.relu / F.silu before
quantize_out (modules/fused.py:124-134, quantizers/fake_quantize.py:49-50) -- and
the backward ops return the gradient with respect to the pre-activation x.
"""
from __future__ import annotations

import ctypes
import numbers

import numpy as np
import torch

from . import _hip as H
from . import host as _host
from ._hip import qden   # re-exported: the observers and distributed.py import it from here


# --------------------------------------------------------------------------- scalars
def _as_f64_device(t: torch.Tensor, device) -> torch.Tensor:
    t = t.detach()
    if t.numel() != 1:
        raise ValueError(f"expected a scalar (1-element) qparam tensor, got shape {tuple(t.shape)}")
    if t.device != device:
        t = t.to(device, non_blocking=True)
    if t.dtype != torch.float64:
        t = t.to(torch.float64)
    return t.contiguous()


def scalar_source(v, device):
    """Resolve a scale / zero-point argument into (device f64 tensor | None, host float).

    Python numbers and CPU tensors are read on the host (no GPU sync); CUDA
    tensors are passed by pointer so the kernel reads the current value."""
    if isinstance(v, torch.Tensor):
        if v.device.type == "cuda":
            return _as_f64_device(v, device), 0.0
        return None, float(v.detach().reshape(()).item())
    if isinstance(v, (numbers.Real, np.floating, np.integer)):
        return None, float(v)
    raise TypeError(f"unsupported qparam type {type(v).__name__}")


def _i64(n):
    return H.c_i64(int(n))


# --------------------------------------------------------------------------- forward (K1)
def fake_quant(x: torch.Tensor, scale, zero_point, qmin: int, qmax: int, *, zp_round: bool = False,
               qp: torch.Tensor | None = None, want_mask: bool = False, want_codes: bool = False,
               discrete: bool = False, act=None):
    """y = (clamp(rint(x/s + zp), qmin, qmax) - zp) * s  (uniform.py:55,95), fp32, bit-exact.
    A CUDA bfloat16 / float16 x: the fp32 result on the exactly widened x, rounded once
    (to nearest even) into y of x's dtype; mask and codes are the fp32 call's.

    qp: optional observer record (f64[QP_LEN] on x.device) used instead of scale/zero_point.
    discrete: return the integer-valued fp32 codes in y instead (discreate_tensor).
    Returns (y, mask|None, codes|None); codes int8 (qmin<0) or uint8.  A CPU tensor takes
    the native host path (host.py; its mask is one byte per element)."""
    if _host.is_host(x):
        return _host.fake_quant(x, scale, zero_point, qmin, qmax, zp_round=zp_round, qp=qp, want_mask=want_mask,
                                want_codes=want_codes, discrete=discrete, act=act)
    x, dt = H.require_device_float(x)
    dev = x.device
    y = torch.empty_like(x)
    mask = H.mask_buffer(1, x.numel(), dev) if want_mask else None
    codes = H.codes_buffer(x.shape, qmin, dev) if want_codes else None
    if qp is not None:
        sd, sh, zd, zh = None, 0.0, None, 0.0
    else:
        sd, sh = scalar_source(scale, dev)
        zd, zh = scalar_source(zero_point, dev)
    rc = H.lib().vsiq_act_fq_fwd_t(H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(mask), _i64(x.numel()), dt,
                                   H.act_code(act), H.ptr(qp), H.ptr(sd), sh, H.ptr(zd), zh,
                                   int(bool(zp_round)), int(bool(discrete)), int(qmin), int(qmax),
                                   H.stream_of(dev))
    H.check(rc, "vsiq_act_fq_fwd_t")
    return y, mask, codes


def ste_backward(g: torch.Tensor, mask: torch.Tensor, scale, rowlen: int = 0, *, pre=None,
                 act=None) -> torch.Tensor:
    """gx = (mask ? g*s : 0) / s  — autograd of uniform.py:55,95 with a fixed scale;
    with ``act``, the activation's backward at the pre-activation ``pre`` follows.
    bfloat16 / float16 g (per-tensor form only; ``pre`` of g's dtype): fake_quant's rule.
    A CPU g: the host loop, per-tensor form (per row: pc_ste_backward); mask as host.fake_quant
    wrote it."""
    if _host.is_host(g):
        return _host.ste_backward(g, mask, scale, pre=pre, act=act)
    g, dt = H.require_device_float(g, "grad_output")
    a = H.act_code(act)
    if a != H.ACT_NONE:
        pre = H.require_same_dtype(pre, g, "pre-activation")
        if pre.shape != g.shape:
            raise ValueError(f"pre-activation shape {tuple(pre.shape)} != grad shape {tuple(g.shape)}")
    dev = g.device
    gx = torch.empty_like(g)
    if isinstance(scale, torch.Tensor) and scale.device.type == "cuda" and scale.numel() > 1:
        g = H.require_device_f32(g, "grad_output")   # per-row scales: fp32 kernels only
        sd, sh = scale.detach().to(torch.float64).contiguous(), 0.0
    else:
        sd, sh = scalar_source(scale, dev)
        rowlen = 0
    rc = H.lib().vsiq_act_ste_bwd_t(H.ptr(g), H.ptr(mask), H.ptr(pre if a else None), H.ptr(gx),
                                    _i64(g.numel()), dt, a, H.ptr(sd), _i64(rowlen), sh, H.stream_of(dev))
    H.check(rc, "vsiq_act_ste_bwd_t")
    return gx


# --------------------------------------------------------------------------- activation alone
class ActivationFn(torch.autograd.Function):
    """act(x) on its own (vsiq_act_fwd_f32 / vsiq_act_bwd_f32): the fused layers' F.silu
    (modules/fused.py:133) where its output is not fake-quantized in the same pass
    (calibration forwards), bit for bit as torch's CPU kernel computes it."""

    @staticmethod
    def forward(ctx, x, act):
        x = H.require_device_f32(x)
        code = H.act_code(act)
        y = torch.empty_like(x)
        H.check(H.lib().vsiq_act_fwd_f32(H.ptr(x), H.ptr(y), _i64(x.numel()), code, H.stream_of(x.device)),
                "vsiq_act_fwd_f32")
        ctx.code = code
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = H.require_device_f32(g, "grad_output")
        gx = torch.empty_like(x)
        H.check(H.lib().vsiq_act_bwd_f32(H.ptr(g), H.ptr(x), H.ptr(gx), _i64(x.numel()), ctx.code,
                                         H.stream_of(x.device)), "vsiq_act_bwd_f32")
        return gx, None


def activation(x, act):
    """The fused layers' F.relu / F.silu (modules/fused.py:133) as the reference computes
    them on its CPU tensors: a CUDA fp32 tensor goes through ActivationFn (torch's HIP silu
    uses another exp, and its HIP relu turns -0.0 into +0.0 where the CPU kernel keeps
    -0.0); anything else is torch's own CPU op, i.e. the reference's."""
    if act not in ("relu", "silu"):
        raise ValueError(f"unsupported fused activation {act!r} ('relu' or 'silu')")
    if isinstance(x, torch.Tensor) and x.device.type == "cuda" and x.dtype == torch.float32:
        return ActivationFn.apply(x, act)
    return torch.nn.functional.relu(x) if act == "relu" else torch.nn.functional.silu(x)


def _ste_grad(ctx, gy):
    """grad_x of a per-tensor Function that saved (mask[, pre-activation]) and set ctx.scale / ctx.act."""
    saved = ctx.saved_tensors
    pre = saved[1] if len(saved) > 1 else None
    return ste_backward(gy.contiguous(), saved[0], ctx.scale, pre=pre, act=ctx.act)


class FakeQuantFixedFn(torch.autograd.Function):
    """Fixed-qparam fake quant with the reference's STE gradient (x only)."""

    @staticmethod
    def forward(ctx, x, scale, zero_point, qmin, qmax, qp, act=None):
        y, mask, _ = fake_quant(x, scale, zero_point, qmin, qmax, qp=qp, want_mask=True, act=act)
        ctx.act = act
        ctx.dtype = x.dtype
        if H.act_code(act) != H.ACT_NONE:
            ctx.save_for_backward(mask, x)
        else:
            ctx.save_for_backward(mask)
        if qp is not None:
            ctx.scale = qp[H.QP_SCALE:H.QP_SCALE + 1]
        else:
            ctx.scale = scale.detach() if isinstance(scale, torch.Tensor) else scale
        return y

    @staticmethod
    def backward(ctx, gy):
        if gy.dtype != ctx.dtype:
            raise TypeError(f"grad_output is {gy.dtype}, the fake-quantized tensor was {ctx.dtype}")
        return _ste_grad(ctx, gy), None, None, None, None, None, None


def _is_half(x) -> bool:
    """A CUDA bfloat16 / float16 tensor: served by the typed kernels through the Python
    autograd Functions."""
    return isinstance(x, torch.Tensor) and x.device.type == "cuda" and x.dtype in (torch.bfloat16, torch.float16)


def _qarg(v):
    """A scale / zero-point argument as (tensor | None, host float) for the C++ nodes:
    tensors go through as tensors (the node reads a CUDA one by pointer and keeps the
    autograd edge of a learnable one), numbers as host floats."""
    if isinstance(v, torch.Tensor):
        return v, 0.0
    if isinstance(v, (numbers.Real, np.floating, np.integer)):
        return None, float(v)
    raise TypeError(f"unsupported qparam type {type(v).__name__}")


def fake_quant_fixed(x, scale, zero_point, qmin, qmax, qp=None, act=None):
    """Fixed-qparam fake quant; with a gradient-requiring x, the STE backward is attached
    (C++ node of _vsiq_torch.so, or FakeQuantFixedFn with VSIQ_TORCH_EXT=0; the C++ nodes
    are fp32-only, so a bfloat16 / float16 x always takes FakeQuantFixedFn).  CPU tensors:
    the native host path (host.py)."""
    host = _host.is_host(x)   # never the C++ node: FakeQuantFixedFn's fake_quant / ste_backward take the host loops
    if x.requires_grad and torch.is_grad_enabled():
        if H.torch_ext_enabled() and not host and not _is_half(x):
            x = H.require_device_f32(x)
            st, sh = _qarg(scale) if qp is None else (None, 0.0)
            zt, zh = _qarg(zero_point) if qp is None else (None, 0.0)
            return H.torch_ext().fq_fixed(x, st, sh, zt, zh, int(qmin), int(qmax), qp, H.act_code(act))
        return FakeQuantFixedFn.apply(x, scale, zero_point, qmin, qmax, qp, act)
    return fake_quant(x, scale, zero_point, qmin, qmax, qp=qp, act=act)[0]


def fake_quant_learn(x, scale, zero_point, qmin, qmax, gscale, learn_zp, act=None):
    """Learnable fake quant (uniform.py:47-56): K1/K5 forward, K4 backward with the
    ScaleGradient factor ``gscale`` (C++ node of _vsiq_torch.so, or FakeQuantLearnFn
    with VSIQ_TORCH_EXT=0 or a bfloat16 / float16 x).  CPU tensors: the native host path
    (host.py: FakeQuantLearnFn's fake_quant / lsq_backward take the host loops)."""
    # the C++ node takes its K4 workspace from its own cache
    if H.torch_ext_enabled() and learn_zp != 2 and not _host.is_host(x) and not _is_half(x):
        x = H.require_device_f32(x)
        st, sh = _qarg(scale)
        zt, zh = _qarg(zero_point)
        return H.torch_ext().fq_learn(x, st, sh, zt, zh, int(qmin), int(qmax), float(gscale), bool(learn_zp),
                                      H.act_code(act))
    return FakeQuantLearnFn.apply(x, scale, zero_point, qmin, qmax, gscale, learn_zp, act)


# --------------------------------------------------------------------------- learnable (K4)
def lsq_backward(g, x, scale, zero_point, qmin, qmax, gscale, learn_zp, act=None):
    """K4: (grad_x, f64[2] {grad_scale, grad_zp}); with ``act``, x is the pre-activation
    and grad_x goes through the activation's backward.  bfloat16 / float16 g and x (the
    same dtype): fake_quant's rule; the f64 gradients are the fp32 call's on the widened
    tensors, bit for bit.  A CPU g: the host loop."""
    if _host.is_host(g):
        return _host.lsq_backward(g, x, scale, zero_point, qmin, qmax, gscale, learn_zp, act)
    g, dt = H.require_device_float(g, "grad_output")
    x = H.require_same_dtype(x, g, "x")
    dev = g.device
    gx = torch.empty_like(g)
    grads = torch.empty(2, dtype=torch.float64, device=dev)
    sd, sh = scalar_source(scale, dev)
    zd, zh = scalar_source(zero_point, dev)
    w = H.workspace(dev, g.numel())
    rc = H.lib().vsiq_act_lsq_bwd_t(H.ptr(g), H.ptr(x), H.ptr(gx), _i64(g.numel()), dt, H.act_code(act),
                                    H.ptr(sd), sh, H.ptr(zd), zh, int(learn_zp), int(qmin),
                                    int(qmax), float(gscale), H.ptr(grads), H.ptr(w.ws),
                                    _i64(w.ws_len), H.ptr(w.counter), H.stream_of(dev))
    H.check(rc, "vsiq_act_lsq_bwd_t")
    return gx, grads


def _qparam_grad(g, v, needed):
    """The f64 gradient g of the scale / zero-point input v as autograd takes it: on v's
    device, in v's dtype and shape; None where v is no tensor or its gradient is not needed."""
    if needed and isinstance(v, torch.Tensor):
        return g.to(device=v.device, dtype=v.dtype).reshape(v.shape)
    return None


class FakeQuantLearnFn(torch.autograd.Function):
    """Learnable-scale (and, asymmetric, learnable zero-point) fake quant.

    Forward = uniform.py:47-56; backward = the reference's autograd graph in closed
    form (ScaleGradient x gscale on scale and zp, ClampBackward1 mask, STE)."""

    @staticmethod
    def forward(ctx, x, scale, zero_point, qmin, qmax, gscale, learn_zp, act=None):
        y, _, _ = fake_quant(x, scale, zero_point, qmin, qmax, zp_round=learn_zp == 1, act=act)   # checks x
        ctx.save_for_backward(x.contiguous())
        ctx.scale, ctx.zp = scale, zero_point
        ctx.args = (qmin, qmax, gscale, learn_zp, act)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        qmin, qmax, gscale, learn_zp, act = ctx.args
        s, z = ctx.scale, ctx.zp
        if gy.dtype != x.dtype:
            raise TypeError(f"grad_output is {gy.dtype}, the fake-quantized tensor was {x.dtype}")
        gx, grads = lsq_backward(gy.contiguous(), x, s, z, qmin, qmax, gscale, learn_zp, act=act)
        gs = _qparam_grad(grads[0], s, ctx.needs_input_grad[1])
        gz = _qparam_grad(grads[1], z, learn_zp and ctx.needs_input_grad[2])
        return gx, gs, gz, None, None, None, None, None


# --------------------------------------------------------------------------- multi-tensor learnable
class LsqSpec:
    """One tensor of a multi-tensor learnable fake quant: qmin/qmax, the ScaleGradient
    factor, whether the zero point is learned, and scale / zero point as device f64
    tensors or host numbers (exactly the arguments of FakeQuantLearnFn)."""

    __slots__ = ("scale", "zero_point", "qmin", "qmax", "gscale", "learn_zp")

    def __init__(self, scale, zero_point, qmin, qmax, gscale, learn_zp):
        if int(learn_zp) not in (0, 1):   # mode 2 (zp as given, no ScaleGradient) is the per-tensor K4's alone
            raise ValueError(f"multi-tensor learnable fake quant: learn_zp must be 0 or 1, got {learn_zp!r}")
        self.scale, self.zero_point = scale, zero_point
        self.qmin, self.qmax, self.gscale, self.learn_zp = int(qmin), int(qmax), float(gscale), bool(learn_zp)


def _lsq_descs(specs, xs, ys=None, gs=None, gxs=None, grads=None):
    """ctypes array of vsiq_lsq_tensor + the device f64 scale/zp copies it points to."""
    arr = (H.LsqTensor * len(specs))()
    keep = []
    for i, (sp, x) in enumerate(zip(specs, xs)):
        d = arr[i]
        sd, sh = scalar_source(sp.scale, x.device)
        zd, zh = scalar_source(sp.zero_point, x.device)
        keep += [sd, zd]
        d.x = x.data_ptr()
        d.y = ys[i].data_ptr() if ys is not None else None
        d.g = gs[i].data_ptr() if gs is not None else None
        d.gx = gxs[i].data_ptr() if gxs is not None else None
        d.scale_dev = sd.data_ptr() if sd is not None else None
        d.zp_dev = zd.data_ptr() if zd is not None else None
        d.grad_out = grads[i].data_ptr() if grads is not None else None
        d.n, d.scale_host, d.zp_host, d.gscale = x.numel(), sh, zh, sp.gscale
        d.qmin, d.qmax, d.zp_learn = sp.qmin, sp.qmax, int(sp.learn_zp)
    return arr, keep


class FakeQuantLearnMultiFn(torch.autograd.Function):
    """FakeQuantLearnFn over many tensors at once (k_multi.hip): one forward launch and
    one backward launch for all of them; per tensor bit-identical to FakeQuantLearnFn.

    apply(specs, *xs, *scale_and_zp_tensors): the learnable tensors referenced by the
    specs are passed again as inputs so autograd routes their gradients."""

    @staticmethod
    def forward(ctx, specs, *inputs):
        k = len(specs)
        xs = [H.require_device_f32(x) for x in inputs[:k]]
        if not xs:
            return ()
        dev = xs[0].device
        if any(x.device != dev for x in xs):
            raise ValueError("multi-tensor fake quant: all tensors must be on one device")
        ys = [torch.empty_like(x) for x in xs]
        arr, keep = _lsq_descs(specs, xs, ys=ys)
        H.check(H.lib().vsiq_lsq_fwd_multi_f32(ctypes.cast(arr, ctypes.c_void_p), k, H.stream_of(dev)),
                "vsiq_lsq_fwd_multi_f32")
        ctx.save_for_backward(*xs)
        ctx.specs = specs
        ctx.params = inputs[k:]
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gys):
        xs = ctx.saved_tensors
        specs = ctx.specs
        k = len(specs)
        dev = xs[0].device
        gs = [H.require_device_f32(g, "grad_output") for g in gys]
        gxs = [torch.empty_like(x) for x in xs]
        grads = torch.empty(k, 2, dtype=torch.float64, device=dev)
        arr, keep = _lsq_descs(specs, xs, gs=gs, gxs=gxs, grads=grads)
        p = ctypes.cast(arr, ctypes.c_void_p)
        need = int(H.lib().vsiq_lsq_multi_workspace_doubles(p, k))
        H.check(need if need < 0 else 0, "vsiq_lsq_multi_workspace_doubles")
        w = H.workspace(dev).reserve_doubles(need)
        rc = H.lib().vsiq_lsq_bwd_multi_f32(p, k, H.ptr(w.ws), _i64(w.ws_len), H.ptr(w.counter),
                                            H.stream_of(dev))
        H.check(rc, "vsiq_lsq_bwd_multi_f32")
        # gradients of the learnable scale / zero-point tensors, in input order
        out = []
        j = k
        for i, sp in enumerate(specs):
            for col, v, learn in ((0, sp.scale, True), (1, sp.zero_point, sp.learn_zp)):
                if isinstance(v, torch.Tensor) and v.requires_grad:
                    out.append(_qparam_grad(grads[i, col], v, learn and ctx.needs_input_grad[1 + j]))
                    j += 1
        return (None, *gxs, *out)


def _ext_qarg(v):
    """(CUDA tensor | None, host float) of a scale / zero point for the C++ K7 node, or
    None when only the Python Function routes it (a gradient-requiring host tensor)."""
    if isinstance(v, torch.Tensor):
        if v.device.type == "cuda":
            return v, 0.0
        if v.requires_grad:
            return None
        return None, float(v.detach().reshape(()).item())
    return None, float(v)


def lsq_fake_quant_multi(xs, specs):
    """Learnable fake quant of every x in ``xs`` with its LsqSpec, in one launch each way
    (the C++ node LsqMultiBackward of _vsiq_torch.so, or FakeQuantLearnMultiFn with
    VSIQ_TORCH_EXT=0)."""
    if H.torch_ext_enabled() and xs:
        qs = [(_ext_qarg(sp.scale), _ext_qarg(sp.zero_point)) for sp in specs]
        if all(a is not None and b is not None for a, b in qs):
            xs = [H.require_device_f32(x) for x in xs]
            return tuple(H.torch_ext().lsq_multi(xs, [a[0] for a, _ in qs], [a[1] for a, _ in qs],
                                                 [b[0] for _, b in qs], [b[1] for _, b in qs],
                                                 [sp.qmin for sp in specs], [sp.qmax for sp in specs],
                                                 [sp.gscale for sp in specs], [sp.learn_zp for sp in specs]))
    params = [v for sp in specs for v in (sp.scale, sp.zero_point)
              if isinstance(v, torch.Tensor) and v.requires_grad]
    return FakeQuantLearnMultiFn.apply(tuple(specs), *xs, *params)


# --------------------------------------------------------------------------- observer (K2)
def observe_tensor(x: torch.Tensor, *, symmetric: bool, num_bits: int = 8, eps: float = 1e-8,
                   run_minmax: torch.Tensor | None = None, want_qp: bool = True,
                   want_stats: bool = True, act=None):
    """One pass over x: min/max/NaN/sums -> running state update -> f64 qparams (no sync).

    Returns (qp f64[QP_LEN] | None, stats f64[ST_LEN] | None).  CPU tensors: the native
    host path (host.py; run_minmax a CPU fp32[2]).  A CUDA bfloat16 / float16 x: the
    record, state and qparams of the fp32 call on the widened values, bit for bit."""
    if _host.is_host(x):
        return _host.observe_tensor(x, symmetric=symmetric, num_bits=num_bits, eps=eps, run_minmax=run_minmax,
                                    want_qp=want_qp, want_stats=want_stats, act=act)
    x, dt = H.require_device_float(x)
    if x.numel() == 0:
        raise H.empty_error()
    dev = x.device
    qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=dev) if want_qp else None
    st = torch.empty(H.ST_LEN, dtype=torch.float64, device=dev) if want_stats else None
    w = H.workspace(dev, x.numel())
    rc = H.lib().vsiq_act_observe_t(H.ptr(x), _i64(x.numel()), dt, H.act_code(act), H.ptr(st),
                                    H.ptr(run_minmax), H.ptr(qp), int(bool(symmetric)),
                                    qden(symmetric, num_bits, eps), float(eps), H.ptr(w.ws),
                                    _i64(w.ws_len), H.ptr(w.counter), H.stream_of(dev))
    H.check(rc, "vsiq_act_observe_t")
    return qp, st


def percentile_tail(percentile) -> float:
    """t = (100 - percentile) / 100 as a Python float: the fraction of a call's elements each
    end of its range may lose (0 <= t < 0.5, else ValueError)."""
    t = (100.0 - percentile) / 100.0
    if not 0.0 <= t < 0.5:
        raise ValueError(f"percentile must be in (50, 100], got {percentile!r}")
    return t


def observe_percentile(x: torch.Tensor, *, symmetric: bool, num_bits: int = 8, eps: float = 1e-8,
                       run_minmax: torch.Tensor | None = None, tail: float, bins: int = 2048, act=None):
    """observe_tensor with the call's range clipped to a percentile of its values before the
    running update (PercentileObserver): K2 for the stats record (of the unclipped tensor),
    then the histogram pass, which reads that record on the device (no sync), drops up to
    floor(N * tail) elements' worth of bins at each end and applies the running update and
    f64 qparams to the clipped range.  Returns (qp f64[QP_LEN], stats f64[ST_LEN], clip
    f64[2] = (lo, hi)).  fp32 only; CPU tensors: the native host loop (host.py)."""
    tail = float(tail)
    if not 0.0 <= tail < 0.5:
        raise ValueError(f"tail must be in [0, 0.5), got {tail!r}")
    if bins & (bins - 1) or not H.HIST_MIN_BINS <= bins <= H.HIST_MAX_BINS:
        raise ValueError(f"bins must be a power of two in [{H.HIST_MIN_BINS}, {H.HIST_MAX_BINS}], got {bins!r}")
    if _host.is_host(x):
        return _host.observe_percentile(x, symmetric=symmetric, num_bits=num_bits, eps=eps, run_minmax=run_minmax,
                                        tail=tail, bins=bins, act=act)
    x = H.require_device_f32(x)
    _, st = observe_tensor(x, symmetric=symmetric, num_bits=num_bits, eps=eps, run_minmax=None, want_qp=False,
                           act=act)
    dev = x.device
    qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=dev)
    clip = torch.empty(2, dtype=torch.float64, device=dev)
    w = H.workspace(dev, x.numel())
    hist = w.histogram()
    rc = H.lib().vsiq_act_observe_hist_f32(H.ptr(x), _i64(x.numel()), H.act_code(act), H.ptr(st), int(bins), tail,
                                           H.ptr(hist), _i64(hist.numel()), H.ptr(w.counter), H.ptr(run_minmax),
                                           H.ptr(qp), H.ptr(clip), int(bool(symmetric)),
                                           qden(symmetric, num_bits, eps), float(eps), H.stream_of(dev))
    H.check(rc, "vsiq_act_observe_hist_f32")
    return qp, st, clip


def mse_ratios(candidates: int = 64, min_ratio: float = 2.0 ** -8) -> tuple:
    """The geometric shrink table of MSEObserver: ``min_ratio ** (k / (candidates - 1))`` in
    Python floats, k = 0 .. candidates - 1 (so ratios[0] == 1.0 exactly); one candidate: (1.0,)."""
    candidates = int(candidates)
    if not 1 <= candidates <= H.MSE_MAX_CANDIDATES:
        raise ValueError(f"candidates must be in [1, {H.MSE_MAX_CANDIDATES}], got {candidates!r}")
    min_ratio = float(min_ratio)
    if not 0.0 < min_ratio <= 1.0:
        raise ValueError(f"min_ratio must be in (0, 1], got {min_ratio!r}")
    if candidates == 1:
        return (1.0,)
    return tuple(min_ratio ** (k / (candidates - 1)) for k in range(candidates))


def check_mse_ratios(ratios) -> tuple:
    """``ratios`` as a tuple of Python floats, or ValueError: 1 to 128 of them, the first
    1.0, every one in (0, 1]."""
    r = tuple(float(v) for v in ratios)
    if not 1 <= len(r) <= H.MSE_MAX_CANDIDATES:
        raise ValueError(f"ratios: 1 to {H.MSE_MAX_CANDIDATES} candidates, got {len(r)}")
    if r[0] != 1.0:
        raise ValueError(f"ratios[0] must be 1.0 (the min / max range itself), got {r[0]!r}")
    for v in r:
        if not 0.0 < v <= 1.0:
            raise ValueError(f"every ratio must be in (0, 1], got {v!r}")
    return r


def observe_mse(x: torch.Tensor, *, symmetric: bool, num_bits: int = 8, eps: float = 1e-8,
                run_minmax: torch.Tensor | None = None, ratios, qmin: int, qmax: int, act=None):
    """observe_tensor with the call's range shrunk to the candidate of the smallest
    quantization error before the running update (MSEObserver): K2 for the stats record (of
    the whole tensor), then the search pass, which reads that record on the device (no
    sync), fake-quantizes every element on the grid (qmin, qmax) with the qparams of each
    range ratios[k] * (min, max), sums the squared errors in f64 and applies the running
    update and f64 qparams to the range of the smallest sum (include/vsiq.h states the
    definition).  Returns (qp f64[QP_LEN], stats f64[ST_LEN], clip f64[2] = (lo, hi), err
    f64[len(ratios)], pick int32[1]).  fp32 only; CPU tensors: the native host loop (host.py)."""
    r = check_mse_ratios(ratios)
    qmin, qmax = int(qmin), int(qmax)
    if qmin >= qmax:
        raise ValueError(f"qmin must be below qmax, got ({qmin}, {qmax})")
    if _host.is_host(x):
        return _host.observe_mse(x, symmetric=symmetric, num_bits=num_bits, eps=eps, run_minmax=run_minmax,
                                 ratios=r, qmin=qmin, qmax=qmax, act=act)
    x = H.require_device_f32(x)
    _, st = observe_tensor(x, symmetric=symmetric, num_bits=num_bits, eps=eps, run_minmax=None, want_qp=False,
                           act=act)
    dev = x.device
    qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=dev)
    clip = torch.empty(2, dtype=torch.float64, device=dev)
    err = torch.empty(len(r), dtype=torch.float64, device=dev)
    pick = torch.empty(1, dtype=torch.int32, device=dev)
    lib = H.lib()
    w = H.workspace(dev, x.numel())
    w.reserve_doubles(max(1, int(lib.vsiq_observe_mse_ws_doubles(_i64(x.numel()), len(r)))))
    table = (H.c_d * len(r))(*r)
    rc = lib.vsiq_act_observe_mse_f32(H.ptr(x), _i64(x.numel()), H.act_code(act), H.ptr(st), table, len(r), qmin,
                                      qmax, H.ptr(w.ws), _i64(w.ws_len), H.ptr(w.counter), H.ptr(run_minmax),
                                      H.ptr(qp), H.ptr(clip), H.ptr(err), H.ptr(pick), int(bool(symmetric)),
                                      qden(symmetric, num_bits, eps), float(eps), H.stream_of(dev))
    H.check(rc, "vsiq_act_observe_mse_f32")
    return qp, st, clip, err, pick


# K8 (one workgroup holds the tensor) up to here; K9 above: through the API K8 is
# 10.9-12.1 us against 17.9-18.2 us for K2 + K1 at 432-16384 elements, but its GPU time
# grows past K2 + K1's ~9 us above ~16K elements (65536: 16.2 us).
_K8_ELEMS = 16384


def observe_fq_max_elems() -> int:
    """Largest tensor observe_fake_quant takes in ONE launch (K8: one workgroup holds it
    in registers)."""
    return int(H.lib().vsiq_observe_fq_max_elems())


def observe_fq_parts_max_elems() -> int:
    """Largest tensor observe_fake_quant takes on the K2p + fold-in-every-workgroup path (K9)."""
    return int(H.lib().vsiq_observe_fq_parts_max_elems())


def observe_fake_quant(x: torch.Tensor, *, symmetric: bool, num_bits: int = 8, eps: float = 1e-8,
                       qmin: int, qmax: int, run_minmax: torch.Tensor | None = None, act=None,
                       want_mask: bool = False, want_codes: bool = False, parts: bool | None = None):
    """Per-tensor observe (running update, f64 qparams, stats) + fake quant of one tensor
    -- observe_tensor + fake_quant(qp=...) fused.  K8 (one launch, one workgroup) up to
    ``_K8_ELEMS`` elements, K9 (K2p records + a fake-quant launch whose every workgroup
    folds them; no arrival chain) above, up to observe_fq_parts_max_elems().  ``parts``:
    False forces K8, True / "k9" K9, "k10" the one-launch K10 (K2p records, a grid
    barrier, every workgroup folds them and quantizes from registers; the same bits as K9,
    and no faster on MI355X: the barrier costs what the second launch does).
    Returns (y, qp f64[QP_LEN], stats f64[ST_LEN], mask | None, codes | None)."""
    x = H.require_device_f32(x)
    n = x.numel()
    if n == 0:
        raise H.empty_error()
    dev = x.device
    y = torch.empty_like(x)
    qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=dev)
    st = torch.empty(H.ST_LEN, dtype=torch.float64, device=dev)
    mask = H.mask_buffer(1, n, dev) if want_mask else None
    codes = H.codes_buffer(x.shape, qmin, dev) if want_codes else None
    if parts is None:
        parts = n > _K8_ELEMS
    # the arguments the three entry points share
    args = (H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(mask), _i64(n), H.act_code(act), H.ptr(st), H.ptr(run_minmax),
            H.ptr(qp), int(bool(symmetric)), qden(symmetric, num_bits, eps), float(eps), int(qmin), int(qmax))
    if parts == "k10":
        w = H.workspace(dev, n)
        rc = H.lib().vsiq_act_observe_fq_grid_f32(*args, H.ptr(w.ws), _i64(w.ws_len), H.ptr(w.counter),
                                                  H.stream_of(dev))
        H.check(rc, "vsiq_act_observe_fq_grid_f32")
        # a workgroup that timed out at the grid barrier wrote NaN and counted itself: fail
        # loudly (one host sync; K10 is an opt-in measurement path; not checkable while the
        # stream is being captured into a HIP graph -- the next eager call reports it)
        err = w.counter[H.COUNTER_GRID_ERRORS:H.COUNTER_GRID_ERRORS + 1]
        if not torch.cuda.is_current_stream_capturing() and int(err.item()):
            err.zero_()
            raise H.VsiqError("vsiq_act_observe_fq_grid_f32: grid barrier timed out (the grid was not "
                              "co-resident); the outputs of the timed-out workgroups are NaN")
    elif parts:   # True / "k9"
        w = H.workspace(dev, n)
        rc = H.lib().vsiq_act_observe_fq_parts_f32(*args, H.ptr(w.ws), _i64(w.ws_len), H.stream_of(dev))
        H.check(rc, "vsiq_act_observe_fq_parts_f32")
    else:
        rc = H.lib().vsiq_act_observe_fq_f32(*args, H.stream_of(dev))
        H.check(rc, "vsiq_act_observe_fq_f32")
    return y, qp, st, mask, codes


class ObserveFakeQuantFn(torch.autograd.Function):
    """K8 forward (observe + fake quant in one launch) with the reference's STE gradient
    at fp32(scale) of this call (the FakeQuantFixedFn backward)."""

    @staticmethod
    def forward(ctx, x, symmetric, num_bits, eps, qmin, qmax, run_minmax, act):
        y, qp, st, mask, _ = observe_fake_quant(x, symmetric=symmetric, num_bits=num_bits, eps=eps, qmin=qmin,
                                                qmax=qmax, run_minmax=run_minmax, act=act, want_mask=True)
        ctx.act = act
        ctx.save_for_backward(mask, x) if H.act_code(act) != H.ACT_NONE else ctx.save_for_backward(mask)
        ctx.scale = qp[H.QP_SCALE:H.QP_SCALE + 1]
        ctx.mark_non_differentiable(qp, st)
        return y, qp, st

    @staticmethod
    def backward(ctx, gy, _gqp, _gst):
        return _ste_grad(ctx, gy), None, None, None, None, None, None, None


def part_slot_doubles(n: int | None = None) -> int:
    """Doubles of one deferred-observer slot for n elements (K2p records x VSIQ_PART_LEN);
    n None: a slot that fits any n."""
    if n is None:
        return H.PART_MAX_RECORDS * H.PART_LEN
    r = int(H.lib().vsiq_observe_part_records(_i64(n)))
    H.check(r if r < 0 else 0, "vsiq_observe_part_records")
    return r * H.PART_LEN


def part_out_slot_doubles(n: int) -> int:
    """Doubles of one K2o slot for n elements (vsiq_observe_part_out_records(n) x
    VSIQ_PART_LEN; one record per workgroup of the one-shot pass)."""
    r = int(H.lib().vsiq_observe_part_out_records(_i64(n)))
    H.check(r if r < 0 else 0, "vsiq_observe_part_out_records")
    return r * H.PART_LEN


def observe_parts(x: torch.Tensor, out: torch.Tensor | None = None, act=None) -> torch.Tensor:
    """Deferred observer pass (K2p): the per-wave partial records of act(x) into
    ``out`` (f64, >= part_slot_doubles(numel) entries; allocated when None), no fold,
    no running update.  Fold with ``fold_parts``."""
    x = H.require_device_f32(x)
    if x.numel() == 0:
        raise H.empty_error()
    need = part_slot_doubles(x.numel())
    if out is None:
        out = torch.empty(need, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or out.device != x.device or not out.is_contiguous():
        raise ValueError("observe_parts: out must be a contiguous float64 tensor on x's device")
    rc = H.lib().vsiq_act_observe_part_f32(H.ptr(x), _i64(x.numel()), H.act_code(act), H.ptr(out),
                                           _i64(out.numel()), H.stream_of(x.device))
    H.check(rc, "vsiq_act_observe_part_f32")
    return out


def observe_parts_out(x: torch.Tensor, act, out: torch.Tensor | None = None):
    """K2o: y = act(x) and the deferred observer records of act(x) (observe_parts) in ONE
    pass -- a fused layer's calibration forward (modules/fused.py:133 + minmax.py:42-43).
    ``out`` holds >= part_out_slot_doubles(numel) doubles (records in observe_parts'
    format, one per workgroup; fold with ``fold_parts``).  Returns (y, out)."""
    x = H.require_device_f32(x)
    if x.numel() == 0:
        raise H.empty_error()
    need = part_out_slot_doubles(x.numel())
    if out is None:
        out = torch.empty(need, dtype=torch.float64, device=x.device)
    elif out.dtype != torch.float64 or out.device != x.device or not out.is_contiguous() or out.numel() < need:
        raise ValueError("observe_parts_out: out must be a contiguous float64 tensor on x's device")
    y = torch.empty_like(x)
    rc = H.lib().vsiq_act_observe_part_out_f32(H.ptr(x), H.ptr(y), _i64(x.numel()), H.act_code(act), H.ptr(out),
                                               _i64(out.numel()), H.stream_of(x.device))
    H.check(rc, "vsiq_act_observe_part_out_f32")
    return y, out


def observe_parts_multi(xs, outs, act=None) -> list:
    """K2m: the deferred observer pass (observe_parts) of every x in ``xs`` into its slot
    in ``outs`` (None: allocated) in one launch per 32 tensors, on the current stream of
    the first x's device.  Records bit-identical to one observe_parts call per x."""
    if not xs:
        return []
    dev = xs[0].device
    arr = (H.PartTensor * len(xs))()
    res = []
    for i, x in enumerate(xs):
        x = H.require_device_f32(x)
        if x.device != dev:
            raise ValueError("observe_parts_multi: all tensors must be on one device")
        if x.numel() == 0:
            raise H.empty_error()
        out = outs[i] if outs is not None else None
        need = part_slot_doubles(x.numel())
        if out is None:
            out = torch.empty(need, dtype=torch.float64, device=dev)
        elif out.dtype != torch.float64 or out.device != dev or not out.is_contiguous():
            raise ValueError("observe_parts_multi: slots must be contiguous float64 tensors on x's device")
        arr[i] = H.PartTensor(x.data_ptr(), x.numel(), out.data_ptr(), out.numel())
        res.append(out)
    rc = H.lib().vsiq_act_observe_part_multi_f32(arr, len(xs), H.act_code(act), H.stream_of(dev))
    H.check(rc, "vsiq_act_observe_part_multi_f32")
    return res


def fold_parts(parts: torch.Tensor) -> torch.Tensor:
    """Fold deferred observer slots ``parts`` [calls, stride] (f64, one call per row) into
    stats records f64 [calls, ST_LEN] in one launch."""
    if parts.dim() != 2 or parts.dtype != torch.float64 or not parts.is_cuda or not parts.is_contiguous():
        raise ValueError("fold_parts: parts must be a contiguous CUDA float64 [calls, stride] tensor")
    st = torch.empty(parts.shape[0], H.ST_LEN, dtype=torch.float64, device=parts.device)
    rc = H.lib().vsiq_observe_fold_parts(H.ptr(parts), _i64(parts.shape[0]), _i64(parts.shape[1]),
                                         H.ptr(st), H.stream_of(parts.device))
    H.check(rc, "vsiq_observe_fold_parts")
    return st


def observe_finalize(stats: torch.Tensor, run_minmax, *, symmetric, num_bits=8, eps=1e-8):
    """Running update + qparams from an (all-reduced) stats record; returns qp f64[QP_LEN]."""
    dev = stats.device
    qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=dev)
    rc = H.lib().vsiq_observe_finalize(H.ptr(stats), H.ptr(run_minmax), H.ptr(qp), int(bool(symmetric)),
                                       qden(symmetric, num_bits, eps), float(eps), H.stream_of(dev))
    H.check(rc, "vsiq_observe_finalize")
    return qp


# --------------------------------------------------------------------------- per-channel (K3)
def per_channel_observe_fq(x: torch.Tensor, *, symmetric: bool, qmin: int, qmax: int,
                           obs_bits: int = 8, eps: float = 1e-8, run_min=None, run_max=None,
                           quantize: bool = True, want_mask: bool = False, want_codes: bool = False,
                           want_row_stats: bool = False):
    """Fused per-channel (axis 0) MinMax observe + f64 qparams + fake quant, one pass (K3).

    quantize=False observes only (state, qparams, stats; y is None).
    Returns dict(y, scale f64[C], zp f64[C], run_min, run_max, mask, codes, row_stats f64[C,3]).
    A CPU tensor takes the native host loops (host.pc_observe_fq; byte mask, no codes)."""
    if _host.is_host(x) and not want_codes:
        return _host.pc_observe_fq(x, symmetric=symmetric, qmin=qmin, qmax=qmax, obs_bits=obs_bits, eps=eps,
                                   run_min=run_min, run_max=run_max, quantize=quantize, want_mask=want_mask,
                                   want_row_stats=want_row_stats)
    x = H.require_device_f32(x)
    dev = x.device
    C = x.shape[0] if x.dim() > 0 else 1
    rowlen = x.numel() // max(C, 1)
    run_min, run_max, y, scale, zp, rstats = H.pc_observe_buffers(x, C, run_min, run_max, quantize, want_row_stats)
    mask = H.mask_buffer(C, rowlen, dev) if (want_mask and quantize) else None
    codes = H.codes_buffer(x.shape, qmin, dev) if (want_codes and quantize) else None
    rc = H.lib().vsiq_pc_observe_fq_f32(H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(mask), _i64(C),
                                        _i64(rowlen), H.ptr(run_min), H.ptr(run_max), H.ptr(scale),
                                        H.ptr(zp), H.ptr(rstats), int(bool(symmetric)), int(qmin),
                                        int(qmax), qden(symmetric, obs_bits, eps), float(eps),
                                        H.stream_of(dev))
    H.check(rc, "vsiq_pc_observe_fq_f32")
    return dict(y=y, scale=scale, zp=zp, run_min=run_min, run_max=run_max, mask=mask, codes=codes,
                row_stats=rstats)


def _mean_layout(ref):
    """(vec, threads) of the host layout ``ref``: default H.mean_reference(), else this process's threads."""
    if ref is None:
        ref = H.mean_reference() or (8, torch.get_num_threads())
    return int(ref[0]), int(ref[1])


def _torch_mean_launch(x, act, layout, out, st, what):
    """vsiq_torch_mean_f32 of a CUDA fp32 x into ``out`` (fp32[4]) or ``st`` (a stats record),
    with the workspace its layout needs."""
    nb = int(H.lib().vsiq_torch_mean_ws_bytes(_i64(x.numel()), *layout))
    if nb < 0:
        raise ValueError(f"{what}: unsupported layout {layout} for {x.numel()} elements")
    ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=x.device)
    rc = H.lib().vsiq_torch_mean_f32(H.ptr(x), _i64(x.numel()), H.act_code(act), *layout, H.ptr(out), H.ptr(st),
                                     H.ptr(ws), _i64(ws.numel()), H.stream_of(x.device))
    H.check(rc, "vsiq_torch_mean_f32")


def torch_mean(x: torch.Tensor, act=None, ref=None) -> torch.Tensor:
    """K11: fp32[4] {sum|act(x)|, sum act(x), mean|act(x)|, mean act(x)} bit for bit as
    torch's CPU kernel sums them on a host of layout ``ref`` = (vec, threads) (default
    H.mean_reference(), else this process's threads) -- quantization_manager.py:66-67's
    torch.mean(torch.abs(x)) / torch.mean(x).  On x's device (CPU tensors: the host loop)."""
    layout = _mean_layout(ref)
    if _host.is_host(x):
        return _host.torch_mean(x, act, *layout)
    x = H.require_device_f32(x)
    out = torch.empty(4, dtype=torch.float32, device=x.device)
    _torch_mean_launch(x, act, layout, out, None, "torch_mean")
    return out


def torch_stats(x: torch.Tensor, act=None, ref=None) -> torch.Tensor:
    """f64[3] {mean|act(x)|, mean act(x), std act(x)} as quantization_manager.py:66-68
    records them on a host of layout ``ref`` (torch.mean / torch.std of the fp32 tensor,
    .item()-ed): K11 and its std pass (vsiq_torch_mean_f32 with a stats record), on x's
    device.  CPU tensors: torch_mean's two means and NaN for std (the host observer's
    record holds the host std)."""
    if _host.is_host(x):
        m = torch_mean(x, act=act, ref=ref)
        return torch.stack([m[2].double(), m[3].double(), torch.tensor(float("nan"), dtype=torch.float64)])
    x = H.require_device_f32(x)
    st = torch.empty(H.ST_LEN, dtype=torch.float64, device=x.device)   # the three fields read are all written
    _torch_mean_launch(x, act, _mean_layout(ref), None, st, "torch_stats")
    return st[H.ST_MEANABS:H.ST_STD + 1]


def stats_from_row_sums(row_stats: torch.Tensor, numel: int) -> torch.Tensor:
    """[C,3] per-row (sum|x|, sum x, sum x^2) -> f64[3] fp32-rounded (mean|x|, mean, std)
    (quantization_manager.py:66-68), on the device, no sync."""
    tot = row_stats.sum(0)
    n = float(numel)
    mean = tot[1] / n
    var = (tot[2] - tot[1] * mean) / (n - 1.0) if numel > 1 else torch.full_like(mean, float("nan"))
    out = torch.stack([tot[0] / n, mean, var.clamp_min(0.0).sqrt()])
    return out.to(torch.float32).to(torch.float64)


def _pc_view(x: torch.Tensor, axis: int):
    """(rows, rowlen, channels) of the row view of x for per-channel axis 0 or 1."""
    if axis not in (0, 1) or x.dim() <= axis:
        raise ValueError(f"per-channel axis must be 0 or 1 of a tensor with more dims, got {axis}")
    C = x.shape[axis]
    rows = C if axis == 0 else x.shape[0] * C
    if rows == 0:
        return 0, 1, max(C, 1)
    return rows, x.numel() // rows, C


def _per_channel_f64(v, C, dev, what):
    """v (a [C]-element tensor, or a 1-element tensor / a number: every channel's) as f64 [C] on dev."""
    v = v.detach() if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float64)
    t = v.to(dev, torch.float64).reshape(-1).contiguous()
    if t.numel() == 1 and C > 1:
        t = t.expand(C).contiguous()
    if t.numel() != C:
        raise RuntimeError(f"per-channel {what} has {t.numel()} entries, the tensor has {C} channels")
    return t


def per_channel_fake_quant(x, scale: torch.Tensor, zp, qmin, qmax, *, zp_round=False,
                           want_mask=False, want_codes=False, axis=0):
    """Per-channel fake quant with given [C] qparams (any float dtype; zp may be None = 0)
    along ``axis`` 0 ([C, ...] weights) or 1 ([N, C, ...] activations).  Returns (y, mask | None,
    codes | None).  A CPU tensor takes the native host loops (host.pc_fake_quant; byte mask, no codes)."""
    if _host.is_host(x) and not want_codes:
        return (*_host.pc_fake_quant(x, scale, zp, qmin, qmax, zp_round=zp_round, want_mask=want_mask, axis=axis),
                None)
    x = H.require_device_f32(x)
    dev = x.device
    rows, rowlen, C = _pc_view(x, axis)
    y = torch.empty_like(x)
    mask = H.mask_buffer(rows, rowlen, dev) if want_mask else None
    codes = H.codes_buffer(x.shape, qmin, dev) if want_codes else None
    s = _per_channel_f64(scale, C, dev, "scale")
    z = _per_channel_f64(zp, C, dev, "zero point") if zp is not None else None
    rc = H.lib().vsiq_pcm_fq_fwd_f32(H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(mask), _i64(rows),
                                     _i64(rowlen), _i64(C), H.ptr(s), H.ptr(z), int(bool(zp_round)),
                                     int(qmin), int(qmax), H.stream_of(dev))
    H.check(rc, "vsiq_pcm_fq_fwd_f32")
    return y, mask, codes


def pc_ste_backward(g, mask, scale, axis=0):
    """The per-channel STE backward: row r of g's row view (``axis`` as per_channel_fake_quant)
    is (mask ? g*s : 0) / s with s = fp32(scale[r % C]); ``mask`` as the forward on g's side
    wrote it (device: H.mask_buffer's 1-bit words; CPU: one byte per element)."""
    if _host.is_host(g):
        return _host.pc_ste_backward(g, mask, scale, axis)
    rows, rowlen, C = _pc_view(g, axis)
    s = _per_channel_f64(scale, C, g.device, "scale")
    if rows != C:   # axis 1: the STE kernel takes one scale per row
        s = s.repeat(rows // C)
    return ste_backward(g.contiguous(), mask, s, rowlen)


class PerChannelFQFn(torch.autograd.Function):
    """Per-channel fake quant with given [C] qparams and the STE backward."""

    @staticmethod
    def forward(ctx, x, scale, zp, qmin, qmax, axis=0):
        y, mask, _ = per_channel_fake_quant(x, scale, zp, qmin, qmax, want_mask=True, axis=axis)
        ctx.save_for_backward(mask, _per_channel_f64(scale, x.shape[axis], x.device, "scale"))
        ctx.axis = axis
        return y

    @staticmethod
    def backward(ctx, gy):
        mask, scale = ctx.saved_tensors
        return pc_ste_backward(gy, mask, scale, ctx.axis), None, None, None, None, None


def pc_lsq_backward(g, x, scale, zp, qmin, qmax, gscale, learn_zp, axis=0):
    """K6: (grad_x, grad_scale f64 [C], grad_zp f64 [C]).  A CPU g: the host loops."""
    if _host.is_host(g):
        return _host.pc_lsq_backward(g, x, scale, zp, qmin, qmax, gscale, learn_zp, axis)
    g = H.require_device_f32(g, "grad_output")
    dev = g.device
    rows, rowlen, C = _pc_view(x, axis)
    s = _per_channel_f64(scale, C, dev, "scale")
    z = _per_channel_f64(zp, C, dev, "zero point") if zp is not None else None
    gx = torch.empty_like(g)
    gs = torch.empty(C, dtype=torch.float64, device=dev)
    gz = torch.empty(C, dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, int(H.lib().vsiq_pcm_workspace_doubles(rows, rowlen))), dtype=torch.float64,
                     device=dev)
    cnt = H.workspace(dev).channel_counters(C)   # per (device, stream / capture): the fold in the launch
    rc = H.lib().vsiq_pcm_lsq_bwd_arrive_f32(H.ptr(g), H.ptr(x), H.ptr(gx), _i64(rows), _i64(rowlen), _i64(C),
                                             H.ptr(s), H.ptr(z), int(bool(learn_zp)), int(qmin), int(qmax),
                                             float(gscale), H.ptr(gs), H.ptr(gz), H.ptr(ws), _i64(ws.numel()),
                                             H.ptr(cnt), _i64(cnt.numel()), H.stream_of(dev))
    H.check(rc, "vsiq_pcm_lsq_bwd_arrive_f32")
    return gx, gs, gz


class PerChannelLearnFn(torch.autograd.Function):
    """Learnable per-channel fake quant (K3-fixed forward, K6 backward): LSQFakeQuantize's
    per-channel path (quantizers/lsq_module.py:134-166) and the learnable
    PerChannelUniformQuantizer.  scale / zero_point are [C]-element tensors (any shape
    with C elements, any float dtype); their gradients come back in that shape/dtype,
    already multiplied by ``gscale`` (ScaleGradient, uniform.py:242-255)."""

    @staticmethod
    def forward(ctx, x, scale, zero_point, qmin, qmax, gscale, learn_zp, axis=0):
        y, _, _ = per_channel_fake_quant(x, scale, zero_point, qmin, qmax, zp_round=learn_zp, axis=axis)   # checks x
        ctx.save_for_backward(x.contiguous())
        ctx.scale, ctx.zp = scale, zero_point
        ctx.args = (qmin, qmax, gscale, learn_zp, axis)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        qmin, qmax, gscale, learn_zp, axis = ctx.args
        s, z = ctx.scale, ctx.zp
        gx, gs, gz = pc_lsq_backward(gy.contiguous(), x, s, z, qmin, qmax, gscale, learn_zp, axis)
        gs = _qparam_grad(gs, s, ctx.needs_input_grad[1])
        gz = _qparam_grad(gz, z, learn_zp and ctx.needs_input_grad[2])
        return gx, gs, gz, None, None, None, None, None


class PerChannelObserveFQFn(torch.autograd.Function):
    """Per-channel observe + fake quant with the STE backward (row c uses fp32(scale_c))."""

    @staticmethod
    def forward(ctx, x, symmetric, qmin, qmax, obs_bits, eps, run_min, run_max, want_row_stats):
        r = per_channel_observe_fq(x, symmetric=symmetric, qmin=qmin, qmax=qmax, obs_bits=obs_bits,
                                   eps=eps, run_min=run_min, run_max=run_max, want_mask=True,
                                   want_row_stats=want_row_stats)
        ctx.save_for_backward(r["mask"], r["scale"])
        rs = r["row_stats"] if want_row_stats else r["scale"].new_zeros(0)
        ctx.mark_non_differentiable(r["scale"], r["zp"], rs)
        return r["y"], r["scale"], r["zp"], rs

    @staticmethod
    def backward(ctx, gy, _gs, _gz, _gr):
        mask, scale = ctx.saved_tensors
        return pc_ste_backward(gy, mask, scale), None, None, None, None, None, None, None, None


# --------------------------------------------------------------------------- per-channel MSE
def per_channel_observe_mse(x: torch.Tensor, *, symmetric: bool, qmin: int, qmax: int, num_bits: int = 8,
                            eps: float = 1e-8, run_min=None, run_max=None, ratios, quantize: bool = True,
                            want_row_stats: bool = False, want_mask: bool = False):
    """Per-channel (axis 0) MSE observe + f64 qparams + fake quant in one launch and one read
    of the tensor (csrc/k_pc_mse.hip): every row W[c] searched as observe_mse searches a tensor
    -- its own min / max, its own candidates ratios[k] * (min, max) scored on the grid (qmin,
    qmax), its own pick and fallback -- then the running update of (run_min[c], run_max[c]) and
    the row's f64 qparams (include/vsiq.h states the definition).

    quantize=False observes only (y is None).  Returns per_channel_observe_fq's dict plus
    clip f64[C, 2] = (lo, hi), err f64[C, len(ratios)], pick int32[C].  fp32 only; CPU tensors:
    the native host loop (host.pc_observe_mse)."""
    r = check_mse_ratios(ratios)
    qmin, qmax = int(qmin), int(qmax)
    if qmin >= qmax:
        raise ValueError(f"qmin must be below qmax, got ({qmin}, {qmax})")
    if _host.is_host(x):
        return _host.pc_observe_mse(x, symmetric=symmetric, qmin=qmin, qmax=qmax, num_bits=num_bits, eps=eps,
                                    run_min=run_min, run_max=run_max, ratios=r, quantize=quantize,
                                    want_row_stats=want_row_stats, want_mask=want_mask)
    x = H.require_device_f32(x)
    dev = x.device
    C = x.shape[0] if x.dim() > 0 else 1
    rowlen = x.numel() // max(C, 1)
    run_min, run_max, y, scale, zp, rstats = H.pc_observe_buffers(x, C, run_min, run_max, quantize, want_row_stats)
    clip = torch.empty(C, 2, dtype=torch.float64, device=dev)
    err = torch.empty(C, len(r), dtype=torch.float64, device=dev)
    pick = torch.empty(C, dtype=torch.int32, device=dev)
    mask = H.mask_buffer(C, rowlen, dev) if (want_mask and quantize) else None
    table = (H.c_d * len(r))(*r)
    rc = H.lib().vsiq_pc_observe_mse_f32(H.ptr(x), H.ptr(y), None, H.ptr(mask), _i64(C), _i64(rowlen), table, len(r),
                                         H.ptr(run_min), H.ptr(run_max), H.ptr(scale), H.ptr(zp), H.ptr(clip),
                                         H.ptr(err), H.ptr(pick), H.ptr(rstats), int(bool(symmetric)), qmin, qmax,
                                         qden(symmetric, num_bits, eps), float(eps), H.stream_of(dev))
    H.check(rc, "vsiq_pc_observe_mse_f32")
    return dict(y=y, scale=scale, zp=zp, run_min=run_min, run_max=run_max, mask=mask, codes=None, row_stats=rstats,
                clip=clip, err=err, pick=pick)


class PerChannelObserveMSEFn(torch.autograd.Function):
    """per_channel_observe_mse with the STE backward (row c uses fp32(scale_c)), in the style
    of PerChannelObserveFQFn.  Returns (y, scale, zp, row_stats, err, pick)."""

    @staticmethod
    def forward(ctx, x, symmetric, qmin, qmax, num_bits, eps, run_min, run_max, ratios, want_row_stats):
        r = per_channel_observe_mse(x, symmetric=symmetric, qmin=qmin, qmax=qmax, num_bits=num_bits, eps=eps,
                                    run_min=run_min, run_max=run_max, ratios=ratios, want_mask=True,
                                    want_row_stats=want_row_stats)
        ctx.save_for_backward(r["mask"], r["scale"])
        rs = r["row_stats"] if want_row_stats else r["scale"].new_zeros(0)
        ctx.mark_non_differentiable(r["scale"], r["zp"], rs, r["err"], r["pick"])
        return r["y"], r["scale"], r["zp"], rs, r["err"], r["pick"]

    @staticmethod
    def backward(ctx, gy, _gs, _gz, _gr, _ge, _gp):
        mask, scale = ctx.saved_tensors
        return pc_ste_backward(gy, mask, scale), None, None, None, None, None, None, None, None, None


# --------------------------------------------------------------------------- per-group
def check_group_size(group_size) -> int:
    """``group_size`` as an int, or ValueError: one of H.PG_GROUPS (32, 64, 128, 256)."""
    if group_size not in H.PG_GROUPS or not isinstance(group_size, (int, np.integer)):   # 128.0, "128", True: no
        raise ValueError(f"per-group quantization: group_size must be one of {H.PG_GROUPS}, got {group_size!r}")
    return int(group_size)


def _pg_input(x, what="x"):
    """(contiguous fp32 tensor, is_host) of a per-group op's tensor; TypeError for anything but
    float32 (the 16-bit kernels are per-tensor only)."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(f"per-group quantization: {what} must be float32, got {x.dtype}")
    kind = x.device.type
    if kind == "cuda" or kind == "cpu":
        return x.contiguous(), kind == "cpu"
    return H.require_device_f32(x, what), False   # raises: neither the GPU nor the host path


def _pg_view(x, group):
    """(rows, rowlen, ngr) of the group-wise view of x: axis-0 rows as K3, ngr groups per row."""
    rows = x.shape[0] if x.dim() > 0 else 1
    if rows == 0 or x.numel() == 0:
        raise H.empty_error()
    rowlen = x.numel() // rows
    return rows, rowlen, -(-rowlen // group)


def _pg_f64(v, rows, ngr, dev, what):
    """v as a contiguous f64 [rows, ngr] tensor on dev (any float dtype, any shape of rows * ngr entries)."""
    if not isinstance(v, torch.Tensor):
        raise TypeError(f"per-group {what} must be a [rows, groups] tensor, got {type(v).__name__}")
    t = v.detach().to(dev, torch.float64)
    if t.numel() != rows * ngr:
        raise ValueError(f"per-group {what} has {t.numel()} entries, the tensor has {rows} x {ngr} groups")
    return t.reshape(rows, ngr).contiguous()


def per_group_observe_fq(x: torch.Tensor, *, group_size: int, symmetric: bool, qmin: int, qmax: int,
                         obs_bits: int = 8, eps: float = 1e-8, run_min=None, run_max=None,
                         quantize: bool = True, want_mask: bool = False, want_codes: bool = False):
    """Fused group-wise MinMax observe + f64 qparams + fake quant in one launch and one read of
    x (csrc/k_pg.hip).  x is viewed as x.shape[0] rows (K3's view); every run of ``group_size``
    (32 / 64 / 128 / 256) consecutive elements of a row -- the last one of a row may be short --
    is observed and quantized exactly as per_channel_observe_fq treats a row holding those
    elements, on its own running (run_min, run_max)[row, group] (fp32 [rows, ngr]; fresh 0/0
    when None; updated in place).

    quantize=False observes only (y is None).  Returns dict(y, scale f64[rows, ngr], zp
    f64[rows, ngr], run_min, run_max, mask, codes); the mask is the whole tensor's 1-bit
    (rows, rowlen) mask (include/vsiq.h).  A CPU tensor takes the native host loops
    (host.pg_observe_fq; byte mask; codes are a device output only)."""
    group = check_group_size(group_size)
    x, host = _pg_input(x)
    if host:
        if want_codes:
            raise NotImplementedError("per_group_observe_fq: integer codes are written by the HIP kernel only; "
                                      "the host loops have none")
        return _host.pg_observe_fq(x, group, symmetric=symmetric, qmin=qmin, qmax=qmax, obs_bits=obs_bits, eps=eps,
                                   run_min=run_min, run_max=run_max, quantize=quantize, want_mask=want_mask)
    dev = x.device
    rows, rowlen, ngr = _pg_view(x, group)
    run_min, run_max, y, scale, zp = H.pg_observe_buffers(x, rows, ngr, run_min, run_max, quantize)
    mask = H.mask_buffer(rows, rowlen, dev) if (want_mask and quantize) else None
    codes = H.codes_buffer(x.shape, qmin, dev) if (want_codes and quantize) else None
    rc = H.lib().vsiq_pg_observe_fq_f32(H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(mask), _i64(rows), _i64(rowlen),
                                        _i64(group), H.ptr(run_min), H.ptr(run_max), H.ptr(scale), H.ptr(zp),
                                        int(bool(symmetric)), int(qmin), int(qmax), qden(symmetric, obs_bits, eps),
                                        float(eps), H.stream_of(dev))
    H.check(rc, "vsiq_pg_observe_fq_f32")
    return dict(y=y, scale=scale, zp=zp, run_min=run_min, run_max=run_max, mask=mask, codes=codes)


def per_group_fake_quant(x, scale, zp, qmin, qmax, *, group_size, zp_round=False, want_mask=False,
                         want_codes=False):
    """Group-wise fake quant with given [rows, ngr] qparams (per_group_observe_fq's layout; any
    float dtype).  Returns (y, mask | None, codes | None).  A CPU tensor takes the native host
    loops (host.pg_fake_quant; byte mask, no codes)."""
    group = check_group_size(group_size)
    x, host = _pg_input(x)
    rows, rowlen, ngr = _pg_view(x, group)
    s = _pg_f64(scale, rows, ngr, x.device, "scale")
    z = _pg_f64(zp, rows, ngr, x.device, "zero point")
    if host:
        if want_codes:
            raise NotImplementedError("per_group_fake_quant: integer codes are written by the HIP kernel only; "
                                      "the host loops have none")
        return (*_host.pg_fake_quant(x, s, z, group, qmin, qmax, zp_round=zp_round, want_mask=want_mask), None)
    dev = x.device
    y = torch.empty_like(x)
    mask = H.mask_buffer(rows, rowlen, dev) if want_mask else None
    codes = H.codes_buffer(x.shape, qmin, dev) if want_codes else None
    rc = H.lib().vsiq_pg_fq_fwd_f32(H.ptr(x), H.ptr(y), H.ptr(codes), H.ptr(mask), _i64(rows), _i64(rowlen),
                                    _i64(group), H.ptr(s), H.ptr(z), int(bool(zp_round)), int(qmin), int(qmax),
                                    H.stream_of(dev))
    H.check(rc, "vsiq_pg_fq_fwd_f32")
    return y, mask, codes


def pg_ste_backward(g, mask, scale, group_size):
    """The group-wise STE backward: gx = (mask ? g*s : 0) / s with s = fp32(scale[row, group]) of
    each element's group; ``mask`` as the forward on g's side wrote it (device: the 1-bit
    words; CPU: one byte per element)."""
    group = check_group_size(group_size)
    g, host = _pg_input(g, "grad_output")
    rows, rowlen, ngr = _pg_view(g, group)
    s = _pg_f64(scale, rows, ngr, g.device, "scale")
    if host:
        return _host.pg_ste_backward(g, mask, s, group)
    gx = torch.empty_like(g)
    rc = H.lib().vsiq_pg_ste_bwd_f32(H.ptr(g), H.ptr(mask), H.ptr(gx), _i64(rows), _i64(rowlen), _i64(group),
                                     H.ptr(s), H.stream_of(g.device))
    H.check(rc, "vsiq_pg_ste_bwd_f32")
    return gx


class PerGroupObserveFQFn(torch.autograd.Function):
    """per_group_observe_fq with the STE backward (each element uses fp32(scale) of its group).
    Returns (y, scale, zp)."""

    @staticmethod
    def forward(ctx, x, group_size, symmetric, qmin, qmax, obs_bits, eps, run_min, run_max):
        r = per_group_observe_fq(x, group_size=group_size, symmetric=symmetric, qmin=qmin, qmax=qmax,
                                 obs_bits=obs_bits, eps=eps, run_min=run_min, run_max=run_max, want_mask=True)
        ctx.save_for_backward(r["mask"], r["scale"])
        ctx.group = group_size
        ctx.mark_non_differentiable(r["scale"], r["zp"])
        return r["y"], r["scale"], r["zp"]

    @staticmethod
    def backward(ctx, gy, _gs, _gz):
        mask, scale = ctx.saved_tensors
        return pg_ste_backward(gy, mask, scale, ctx.group), None, None, None, None, None, None, None, None


class PerGroupFQFn(torch.autograd.Function):
    """Group-wise fake quant with given [rows, ngr] qparams and the STE backward."""

    @staticmethod
    def forward(ctx, x, scale, zp, qmin, qmax, group_size):
        y, mask, _ = per_group_fake_quant(x, scale, zp, qmin, qmax, group_size=group_size, want_mask=True)
        ctx.save_for_backward(mask, scale.detach().to(x.device, torch.float64))
        ctx.group = group_size
        return y

    @staticmethod
    def backward(ctx, gy):
        mask, scale = ctx.saved_tensors
        return pg_ste_backward(gy, mask, scale, ctx.group), None, None, None, None, None


def pg_lsq_backward(g, x, scale, zp, qmin, qmax, gscale, learn_zp, group_size):
    """The group-wise learnable (LSQ) backward, one launch (csrc/k_pg.hip): (grad_x, grad_scale
    f64 [rows, ngr], grad_zp f64 [rows, ngr]).  Every group is the per-tensor learnable backward
    on its elements alone with (scale, zp)[row, group]; ``learn_zp``: the forward used
    clamp(rint(zp)) (per_group_fake_quant's zp_round) and grad_zp is its gradient, else zeros.
    The gradients are already multiplied by ``gscale``.  A CPU g: the host loops."""
    group = check_group_size(group_size)
    g, host = _pg_input(g, "grad_output")
    x, xhost = _pg_input(x)
    if xhost != host or x.device != g.device:
        raise ValueError(f"grad_output is on {g.device}, x on {x.device}")
    if x.shape != g.shape:
        raise ValueError(f"grad_output has shape {tuple(g.shape)}, x {tuple(x.shape)}")
    rows, rowlen, ngr = _pg_view(g, group)
    s = _pg_f64(scale, rows, ngr, g.device, "scale")
    z = _pg_f64(zp, rows, ngr, g.device, "zero point")
    if host:
        return _host.pg_lsq_backward(g, x, s, z, group, qmin, qmax, gscale, learn_zp)
    gx = torch.empty_like(g)
    gs = torch.empty_like(s)
    gz = torch.empty_like(s)
    rc = H.lib().vsiq_pg_lsq_bwd_f32(H.ptr(g), H.ptr(x), H.ptr(gx), _i64(rows), _i64(rowlen), _i64(group),
                                     H.ptr(s), H.ptr(z), int(bool(learn_zp)), int(qmin), int(qmax), float(gscale),
                                     H.ptr(gs), H.ptr(gz), H.stream_of(g.device))
    H.check(rc, "vsiq_pg_lsq_bwd_f32")
    return gx, gs, gz


class PerGroupLearnFn(torch.autograd.Function):
    """Learnable group-wise fake quant: per_group_fake_quant forward (zp_round = learn_zp),
    pg_lsq_backward backward.  scale / zero_point are tensors of rows * ngr entries (any shape,
    any float dtype); their gradients come back in that shape / dtype, already multiplied by
    ``gscale`` (ScaleGradient, uniform.py:242-255)."""

    @staticmethod
    def forward(ctx, x, scale, zero_point, qmin, qmax, gscale, learn_zp, group_size):
        y, _, _ = per_group_fake_quant(x, scale, zero_point, qmin, qmax, group_size=group_size,
                                       zp_round=learn_zp)   # checks x
        ctx.save_for_backward(x.contiguous())
        ctx.scale, ctx.zp = scale, zero_point
        ctx.args = (qmin, qmax, gscale, learn_zp, group_size)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        qmin, qmax, gscale, learn_zp, group_size = ctx.args
        s, z = ctx.scale, ctx.zp
        gx, gs, gz = pg_lsq_backward(gy.contiguous(), x, s, z, qmin, qmax, gscale, learn_zp, group_size)
        gs = _qparam_grad(gs, s, ctx.needs_input_grad[1])
        gz = _qparam_grad(gz, z, learn_zp and ctx.needs_input_grad[2])
        return gx, gs, gz, None, None, None, None, None


# --------------------------------------------------------------------------- export
PACK_BITS = (2, 4, 8)


class PackedTensor:
    """A tensor exported as packed integer codes (layout: include/vsiq.h, "Packed codes").

    data     uint8 [rows, row_bytes]: unsigned ``bits``-wide fields holding code - qmin
    shape    the tensor's shape
    bits     2, 4 or 8
    qmin, qmax   the integer grid the codes lie on
    qparams  fp32 [nq, 2]: the (scale, zero point) pairs the kernel used; nq = 1 (per tensor)
             or shape[0] (per channel)
    axis     0 (per channel along axis 0) or None (per tensor)

    ``state()`` / ``from_state()`` map it to and from a dict of tensors, ints, a list and
    None: plain data that torch.save / torch.load(weights_only=True) round-trips."""

    __slots__ = ("data", "shape", "bits", "qmin", "qmax", "qparams", "axis")

    def __init__(self, data, shape, bits, qmin, qmax, qparams, axis=None):
        bits, qmin, qmax = int(bits), int(qmin), int(qmax)
        shape = tuple(int(d) for d in shape)
        if bits not in PACK_BITS:
            raise ValueError(f"packed bits must be one of {PACK_BITS}, got {bits}")
        if axis not in (None, 0):
            raise ValueError(f"packed axis must be 0 or None, got {axis!r}")
        if qmin > qmax or qmax - qmin + 1 > 2 ** bits:
            raise ValueError(f"the grid [{qmin}, {qmax}] does not fit {bits}-bit fields")
        rows, rowlen = _pack_view(shape, axis)
        nq = rows if axis == 0 else 1
        row_bytes = 4 * ((rowlen * bits + 31) // 32)
        if data.dtype != torch.uint8 or tuple(data.shape) != (rows, row_bytes):
            raise ValueError(f"packed data must be uint8 [{rows}, {row_bytes}] for shape {shape} at {bits} bits, "
                             f"got {data.dtype} {tuple(data.shape)}")
        if qparams.dtype != torch.float32 or tuple(qparams.shape) != (nq, 2):
            raise ValueError(f"packed qparams must be float32 [{nq}, 2], got {qparams.dtype} {tuple(qparams.shape)}")
        if qparams.device != data.device:
            raise ValueError(f"packed data is on {data.device}, its qparams on {qparams.device}")
        self.data, self.shape, self.bits, self.qmin, self.qmax = data, shape, bits, qmin, qmax
        self.qparams, self.axis = qparams, axis

    def state(self) -> dict:
        return {"data": self.data, "shape": list(self.shape), "bits": self.bits, "qmin": self.qmin,
                "qmax": self.qmax, "qparams": self.qparams, "axis": self.axis}

    @classmethod
    def from_state(cls, state: dict) -> "PackedTensor":
        return cls(state["data"], state["shape"], state["bits"], state["qmin"], state["qmax"], state["qparams"],
                   state["axis"])

    def to(self, device) -> "PackedTensor":
        return PackedTensor(self.data.to(device), self.shape, self.bits, self.qmin, self.qmax,
                            self.qparams.to(device), self.axis)

    def __repr__(self):
        return (f"PackedTensor(shape={self.shape}, bits={self.bits}, grid=[{self.qmin}, {self.qmax}], "
                f"axis={self.axis}, device={self.data.device})")


def _pack_view(shape, axis):
    """(rows, rowlen) of the row view: per tensor one row of numel, axis 0 one row per channel."""
    n = 1
    for d in shape:
        n *= d
    if n == 0:
        raise ValueError(f"cannot pack an empty tensor (shape {tuple(shape)})")
    if axis is None:
        return 1, n
    if len(shape) < 1:
        raise ValueError("per-channel packing (axis=0) needs a tensor with at least one dim")
    return shape[0], n // shape[0]


def pack_bits_for(qmin: int, qmax: int) -> int:
    """The smallest field width of 2 / 4 / 8 bits that holds the grid [qmin, qmax]."""
    for b in PACK_BITS:
        if qmax - qmin + 1 <= 2 ** b:
            return b
    raise ValueError(f"the grid [{qmin}, {qmax}] is wider than 8 bits")


def _pack_scalar_f64(v, dev):
    """A per-tensor qparam as an f64 [1] tensor on dev (a CUDA tensor is passed on without a sync)."""
    if isinstance(v, torch.Tensor):
        return _as_f64_device(v, dev).reshape(1)
    if isinstance(v, (numbers.Real, np.floating, np.integer)):
        return torch.tensor([float(v)], dtype=torch.float64, device=dev)
    raise TypeError(f"unsupported qparam type {type(v).__name__}")


def _row_qparams(t, scale, zero_point, axis, what):
    """(rows, rowlen, nq, f64 scale [nq], f64 zp [nq] | None) of a pack or AdaRound call on t, on
    t's device: axis None one row and scalar qparams, axis 0 one row and one (scale, zero
    point) per out-channel (a number is every channel's)."""
    if axis not in (None, 0):
        raise ValueError(f"{what}: axis must be 0 or None, got {axis!r}")
    rows, rowlen = _pack_view(t.shape, axis)
    dev = t.device
    if axis is None:
        s = _pack_scalar_f64(scale, dev)
        z = _pack_scalar_f64(zero_point, dev) if zero_point is not None else None
        return rows, rowlen, 1, s, z
    s = _per_channel_f64(scale, rows, dev, "scale")
    z = _per_channel_f64(zero_point, rows, dev, "zero point") if zero_point is not None else None
    return rows, rowlen, rows, s, z


def quantize_pack(x: torch.Tensor, scale, zero_point, qmin: int, qmax: int, *, bits=None, axis=None,
                  zp_round: bool = False) -> PackedTensor:
    """Quantize x to the integer codes clamp(rint(x/s + zp), qmin, qmax) of the forward
    kernels (NaN -> code 0) and pack them into ``bits``-wide fields (None: the smallest of
    2 / 4 / 8 that holds the grid): one launch, one read of x.  axis=None: scalar qparams;
    axis=0: [C] qparams, one per out-channel row (zero_point None = 0).  The returned
    PackedTensor carries the fp32 (scale, zero point) the kernel used, after ``zp_round``
    (clamp(rint(zp), qmin, qmax), the learnable zero point's rounding); unpack_dequant
    reproduces the forward's y from them.  A CPU tensor takes the native host loops."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a torch.Tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(f"x: only float32 is supported by the HIP fake-quant path, got {x.dtype}")
    if not x.is_contiguous():
        raise TypeError("x: quantize_pack needs a contiguous tensor (call .contiguous() first)")
    qmin, qmax = int(qmin), int(qmax)
    if bits is None:
        bits = pack_bits_for(qmin, qmax)
    bits = int(bits)
    if bits not in PACK_BITS:
        raise ValueError(f"packed bits must be one of {PACK_BITS}, got {bits}")
    if qmin > qmax or qmax - qmin + 1 > 2 ** bits:
        raise ValueError(f"the grid [{qmin}, {qmax}] does not fit {bits}-bit fields")
    rows, rowlen, nq, s, z = _row_qparams(x, scale, zero_point, axis, "quantize_pack")
    dev = x.device
    if dev.type == "cpu":
        data, qparams = _host.quantize_pack(x, s, z, nq, rows, rowlen, qmin, qmax, bits, zp_round)
        return PackedTensor(data, x.shape, bits, qmin, qmax, qparams, axis)
    x = H.require_device_f32(x)
    row_bytes = int(H.lib().vsiq_packed_row_bytes(_i64(rowlen), bits))
    data = torch.empty((rows, row_bytes), dtype=torch.uint8, device=dev)
    qparams = torch.empty((nq, 2), dtype=torch.float32, device=dev)
    rc = H.lib().vsiq_quantize_pack_f32(H.ptr(x), H.ptr(data), H.ptr(qparams), _i64(rows), _i64(rowlen), H.ptr(s),
                                        H.ptr(z), _i64(nq), int(bool(zp_round)), qmin, qmax, bits, H.stream_of(dev))
    H.check(rc, "vsiq_quantize_pack_f32")
    return PackedTensor(data, x.shape, bits, qmin, qmax, qparams, axis)


def unpack_dequant(p: PackedTensor, dtype=torch.float32, want_codes: bool = False):
    """The inverse of quantize_pack: y = (code - zp) * s in fp32 -- the forward kernels' last
    two operations on the qparams the pack call recorded -- rounded once to ``dtype``
    (float32 / bfloat16 / float16).  Returns y, or (y, codes) with the int8 (qmin < 0) /
    uint8 codes in the layout ``want_codes`` of the fake-quant functions produces."""
    if not isinstance(p, PackedTensor):
        raise TypeError(f"unpack_dequant takes a PackedTensor, got {type(p).__name__}")
    if dtype not in H._DT_CODES:
        raise TypeError(f"unpack_dequant: float32, bfloat16 or float16 expected, got {dtype}")
    rows, rowlen = _pack_view(p.shape, p.axis)
    data, qparams = p.data.contiguous(), p.qparams.contiguous()
    dev = data.device
    if dev.type == "cpu":
        y, codes = _host.unpack_dequant(data, qparams, p.shape, rows, rowlen, p.qmin, p.bits, want_codes)
        y = y if dtype == torch.float32 else y.to(dtype)
        return (y, codes) if want_codes else y
    if dev.type != "cuda":
        raise H.VsiqError(f"packed data is on {dev}: unpack_dequant runs on MI355X (HIP) or on CPU tensors")
    y = torch.empty(p.shape, dtype=dtype, device=dev)
    codes = H.codes_buffer(p.shape, p.qmin, dev) if want_codes else None
    rc = H.lib().vsiq_unpack_dequant(H.ptr(data), H.ptr(y), H.ptr(codes), _i64(rows), _i64(rowlen), H.ptr(qparams),
                                     _i64(qparams.shape[0]), p.qmin, p.bits, H._DT_CODES[dtype], H.stream_of(dev))
    H.check(rc, "vsiq_unpack_dequant")
    return (y, codes) if want_codes else y


# --------------------------------------------------------------------------- AdaRound
def _ada_tensor(t, what, like=None):
    """A contiguous float32 tensor (CPU or CUDA) of ``like``'s shape and device."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: only float32 is supported by the HIP fake-quant path, got {t.dtype}")
    if t.device.type not in ("cpu", "cuda"):
        raise H.VsiqError(f"{what} is on {t.device}: AdaRound runs on MI355X (HIP) or on CPU tensors")
    if like is not None:
        if tuple(t.shape) != tuple(like.shape):
            raise ValueError(f"{what} must be float32 {tuple(like.shape)} like w, got {tuple(t.shape)}")
        if t.device != like.device:
            raise ValueError(f"{what} is on {t.device}, w on {like.device}")
    return t.detach().contiguous()


def adaround_forward(w, V, scale, zero_point, qmin: int, qmax: int, *, axis=None, hard: bool = False,
                     beta=None, zp_round: bool = False, want_y: bool = True):
    """AdaRound's forward (include/vsiq.h, "AdaRound"): y = (clamp(floor(w/s + z) + h(V)) - z) * s
    with the rectified sigmoid h (soft) or h = (V >= 0) (hard), in one launch and one read of
    w and V.  ``beta`` given: also the f64 regulariser R = sum(1 - |2h - 1|^beta) as a 0-dim
    tensor on w's device (no host sync).  axis=None: scalar qparams; axis=0: [C] qparams
    (zero_point None = 0).  Returns (y | None, R | None); want_y=False computes R alone.
    fp32 only; a CPU tensor takes the native host loops."""
    w = _ada_tensor(w, "w")
    V = _ada_tensor(V, "V", w)
    if not want_y and beta is None:
        raise ValueError("adaround_forward: nothing to compute (want_y=False and no beta)")
    if hard and beta is not None:
        raise ValueError("adaround_forward: the regulariser belongs to the soft forward (hard=True with beta)")
    rows, rowlen, nq, s, z = _row_qparams(w, scale, zero_point, axis, "adaround")
    dev = w.device
    y = torch.empty_like(w) if want_y else None
    reg = torch.empty((), dtype=torch.float64, device=dev) if beta is not None else None
    b = float(beta) if beta is not None else 1.0
    if dev.type == "cpu":
        _host.adaround_forward(w, V, y, reg, rows, rowlen, s, z, nq, zp_round, qmin, qmax, hard, b)
        return y, reg
    ws = wsl = cnt = None
    if reg is not None:
        need = int(H.lib().vsiq_adaround_workspace_doubles(_i64(rows), _i64(rowlen)))
        if need < 0:
            H.check(need, "vsiq_adaround_workspace_doubles")
        wk = H.workspace(dev).reserve_doubles(need)
        ws, wsl, cnt = wk.ws, wk.ws_len, wk.counter
    rc = H.lib().vsiq_adaround_fwd_f32(H.ptr(w), H.ptr(V), H.ptr(y), _i64(rows), _i64(rowlen), H.ptr(s), H.ptr(z),
                                       _i64(nq), int(bool(zp_round)), int(qmin), int(qmax), int(bool(hard)), b,
                                       H.ptr(reg), H.ptr(ws), _i64(wsl or 0), H.ptr(cnt), H.stream_of(dev))
    H.check(rc, "vsiq_adaround_fwd_f32")
    return y, reg


def adaround_backward(g, w, V, scale, zero_point, qmin: int, qmax: int, *, axis=None, lam: float = 0.0,
                      beta: float = 2.0, zp_round: bool = False):
    """grad_V of the soft forward plus lam * R(beta) in one launch:
    fp32((g * s * m + lam * dR/dh) * h'(V)) per element (include/vsiq.h, "AdaRound")."""
    w = _ada_tensor(w, "w")
    V = _ada_tensor(V, "V", w)
    g = _ada_tensor(g, "grad_output", w)
    rows, rowlen, nq, s, z = _row_qparams(w, scale, zero_point, axis, "adaround")
    dev = w.device
    gv = torch.empty_like(V)
    if dev.type == "cpu":
        _host.adaround_backward(g, w, V, gv, rows, rowlen, s, z, nq, zp_round, qmin, qmax, lam, beta)
        return gv
    rc = H.lib().vsiq_adaround_bwd_f32(H.ptr(g), H.ptr(w), H.ptr(V), H.ptr(gv), _i64(rows), _i64(rowlen), H.ptr(s),
                                       H.ptr(z), _i64(nq), int(bool(zp_round)), int(qmin), int(qmax), float(lam),
                                       float(beta), H.stream_of(dev))
    H.check(rc, "vsiq_adaround_bwd_f32")
    return gv


class AdaRoundFn(torch.autograd.Function):
    """(y, R) = soft AdaRound forward of (V; w, qparams); V is the only differentiable input.
    The loss is taken as L(y) + lam * R: backward returns dL/dy's chain through y PLUS
    lam * dR/dV from the same launch, so R itself is returned non-differentiable (for
    logging) and must not be added to the loss a second time."""

    @staticmethod
    def forward(ctx, V, w, scale, zero_point, qmin, qmax, axis, lam, beta, zp_round):
        y, reg = adaround_forward(w, V, scale, zero_point, qmin, qmax, axis=axis, beta=beta, zp_round=zp_round)
        ctx.save_for_backward(V, w)
        ctx.args = (scale, zero_point, qmin, qmax, axis, float(lam), float(beta), zp_round)
        ctx.mark_non_differentiable(reg)
        return y, reg

    @staticmethod
    def backward(ctx, gy, _greg):
        V, w = ctx.saved_tensors
        scale, zero_point, qmin, qmax, axis, lam, beta, zp_round = ctx.args
        gv = adaround_backward(gy, w, V, scale, zero_point, qmin, qmax, axis=axis, lam=lam, beta=beta,
                               zp_round=zp_round)
        return gv, None, None, None, None, None, None, None, None, None


# --------------------------------------------------------------------------- MX block scaling
def _mx_format(fmt):
    """(VSIQ_MX_* code, bits, exponent bits, mantissa bits, bias) of an element-format name."""
    try:
        return H.MX_FORMATS[fmt]
    except (KeyError, TypeError):
        raise ValueError(f"unknown MX element format {fmt!r} (one of {sorted(H.MX_FORMATS)})") from None


def _mx_view(shape, axis):
    """The host loops' view of blocks along ``axis`` of a contiguous tensor of ``shape``: (rows,
    rowlen) for the last axis (and for axis 1 of an [N, C] tensor), (outer, channels, inner)
    for axis 1 of an [N, C, ...] tensor; plus the shape of the scales tensor."""
    nd = len(shape)
    if nd == 0:
        return (1, 1), (1,)
    ax = axis + nd if axis < 0 else axis
    n = 1
    for d in shape:
        n *= d
    if n == 0:
        raise ValueError(f"MX fake quant of an empty tensor (shape {tuple(shape)})")
    if ax == nd - 1:
        nb = -(-shape[-1] // 32)
        return (n // shape[-1], shape[-1]), tuple(shape[:-1]) + (nb,)
    if ax == 1 and nd > 2:
        inner = n // (shape[0] * shape[1])
        return (shape[0], shape[1], inner), (shape[0], -(-shape[1] // 32)) + tuple(shape[2:])
    raise NotImplementedError(f"MX blocks run along the last axis or axis 1, got axis {axis} of a {nd}-d tensor")


def _mx_forward(x, fmt, axis, want_codes, want_mask):
    """One MX fake-quant call on a contiguous CPU float32 x (the host loops): (y, codes | None,
    scales | None, mask | None); the mask is one byte per element.  There is no device kernel:
    a CUDA tensor raises (never a quiet copy to the host)."""
    code = _mx_format(fmt)[0]
    if not _host.is_host(x):
        if x.device.type == "cpu":
            raise TypeError(f"x: only float32 is supported by the host (CPU) MX fake quant, got {x.dtype}")
        raise H.VsiqError(f"x is on {x.device}: MX fake quant has no HIP kernel yet and runs on CPU float32 "
                          "tensors only (the native host loops); nothing is copied to the host behind your back")
    view, sshape = _mx_view(x.shape, axis)
    y = torch.empty_like(x)
    codes = torch.empty(x.shape, dtype=torch.uint8) if want_codes else None
    scales = torch.empty(sshape, dtype=torch.uint8) if want_codes else None
    mask = torch.empty(x.shape, dtype=torch.uint8) if want_mask else None
    _host.mx_fake_quant(x, y, codes, scales, mask, view, code)
    return y, codes, scales, mask


class MXFakeQuantFn(torch.autograd.Function):
    """MX fake quant with the straight-through gradient: grad_x = g where rounding stayed on
    the element grid, 0 where it picked the overflow value.  Saves the mask; the backward is
    the existing STE backward with scale 1 ((mask ? g * 1 : 0) / 1 is g exactly)."""

    @staticmethod
    def forward(ctx, x, fmt, axis):
        y, _, _, mask = _mx_forward(x, fmt, axis, False, True)
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, gy):
        (mask,) = ctx.saved_tensors
        return ste_backward(gy.contiguous(), mask, 1.0), None, None


def _is_channels_last(x) -> bool:
    return x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)


def mx_fake_quant(x: torch.Tensor, fmt: str, axis: int = -1, want_codes: bool = False):
    """OCP MX fake quant (include/vsiq.h, "MX block-scaled fake quantization"): blocks of 32
    consecutive elements along ``axis`` share one power-of-two scale and every element is
    rounded to the 4-, 6- or 8-bit float ``fmt`` ("fp4_e2m1", "fp6_e2m3", "fp6_e3m2",
    "fp8_e4m3", "fp8_e5m2").  CPU float32 tensors only, on the native host loops (there is no
    HIP kernel for it yet: a CUDA tensor raises VsiqError).
    axis=-1: rows are everything before the last dim; axis=1 of an [N, C, ...] tensor: blocks
    along the channels (an [N, C] tensor: its rows).  Differentiable in x (MXFakeQuantFn).
    Returns y, or (y, codes uint8 like x, scales uint8: x's shape with ``axis`` cut to its
    block count) with ``want_codes``."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a torch.Tensor, got {type(x).__name__}")
    _mx_format(fmt)
    nd = x.dim()
    if nd and not -nd <= axis < nd:
        raise NotImplementedError(f"MX blocks run along the last axis or axis 1, got axis {axis} of a {nd}-d tensor")
    if axis % max(nd, 1) == 1 and _is_channels_last(x):   # NHWC memory: the channels are its rows
        out = mx_fake_quant(x.permute(0, 2, 3, 1), fmt, -1, want_codes)
        return tuple(t.permute(0, 3, 1, 2) for t in out) if want_codes else out.permute(0, 3, 1, 2)
    x = x.contiguous()
    if want_codes:
        y, codes, scales, _ = _mx_forward(x.detach(), fmt, axis, True, False)
        return y, codes, scales
    if x.requires_grad and torch.is_grad_enabled():
        return MXFakeQuantFn.apply(x, fmt, axis)
    return _mx_forward(x, fmt, axis, False, False)[0]


def mx_dequant(codes: torch.Tensor, scales: torch.Tensor, fmt: str, axis: int = -1, dtype=torch.float32):
    """The inverse of mx_fake_quant(..., want_codes=True): y = table[code] * 2^(scale - 127),
    a 2^bits-entry lookup times the block's power of two (built from its exponent bits, so
    exact), in eager torch (not a hot path).  A scale byte of 255 gives NaN."""
    _, bits, ebits, mbits, bias = _mx_format(fmt)
    dev = codes.device
    c = torch.arange(1 << bits, dtype=torch.int32)
    eb, m = (c >> mbits) & ((1 << ebits) - 1), c & ((1 << mbits) - 1)
    mag = torch.where(eb == 0, m.double() * 2.0 ** (1 - bias - mbits),
                      (1.0 + m.double() / (1 << mbits)) * torch.pow(2.0, (eb - bias).double()))
    table = torch.where((c >> (bits - 1)) == 1, -mag, mag).to(torch.float32).to(dev)
    s = scales.to(torch.int32)
    x2 = torch.where(s == 0, torch.full_like(s, 0x00400000), s << 23).view(torch.float32)   # 2^(s - 127)
    nd = codes.dim()
    ax = axis + nd if axis < 0 else axis
    if not (ax == nd - 1 or (ax == 1 and nd > 2)):
        raise NotImplementedError(f"MX blocks run along the last axis or axis 1, got axis {axis} of a {nd}-d tensor")
    x2 = x2.repeat_interleave(32, dim=ax).narrow(ax, 0, codes.shape[ax])
    nan_block = (s == 255).repeat_interleave(32, dim=ax).narrow(ax, 0, codes.shape[ax])
    y = table[codes.long() & ((1 << bits) - 1)] * x2
    y = torch.where(nan_block, torch.full_like(y, float("nan")), y)
    return y if dtype == torch.float32 else y.to(dtype)
