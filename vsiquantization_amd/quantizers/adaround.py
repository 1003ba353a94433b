"""AdaRoundWeight: the learnable rounding variable of one weight tensor (AdaRound, Nagel et
al. 2020, "Up or Down? Adaptive Rounding for Post-Training Quantization").

Once a weight's clip range (scale, zero point) is fixed, round-to-nearest is replaced by
``floor(w/s + z) + h(V)`` with one learnable ``V`` per weight: ``h`` is the rectified
sigmoid ``clip(1.2 * sigmoid(V) - 0.1, 0, 1)`` while optimising and ``V >= 0`` afterwards.
The forward, the regulariser ``R = sum(1 - |2h - 1|^beta)`` and the gradient of
``loss(y) + lam * R`` with respect to ``V`` are two HIP launches per step
(csrc/k_adaround.hip; CPU tensors: the host loops of the same library).  fp32 weights,
per tensor or per out-channel (axis 0); ``utils/adaround.py`` drives it over a model.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..fakequant import AdaRoundFn, _ada_tensor, _row_qparams, adaround_forward

ZETA, GAMMA = 1.1, -0.1


class AdaRoundWeight(nn.Module):
    """Holds ``V`` for one weight tensor and the grid it rounds on.

    ``init_from(w, s, z, lo, hi)`` fixes the qparams (scalars: per tensor; [C] tensors: per
    out-channel row) and starts ``V`` where the soft rounding reproduces ``w/s + z`` itself.
    ``lam`` / ``beta`` are the regulariser's weight and exponent of the NEXT training
    forward (the driver anneals them); the gradient of ``lam * R`` reaches ``V`` through
    that forward's backward, so the loss is just the reconstruction error."""

    def __init__(self):
        super().__init__()
        self.V = None
        self.lam = 0.0
        self.beta = 20.0
        self.last_regulariser = None
        self._q = None   # (scale f64, zp f64 | None, lo, hi, axis)

    def init_from(self, w, s, z, lo: int, hi: int):
        w = _ada_tensor(w, "w")
        per_channel = any(isinstance(v, torch.Tensor) and v.dim() == 1 and v.numel() > 1 for v in (s, z))
        axis = 0 if per_channel else None
        _, _, _, s64, z64 = _row_qparams(w, s, z, axis, "adaround")
        self._q = (s64, z64, int(lo), int(hi), axis)
        # plain torch, once: frac = t - floor(t) of the forward's own t = RN(RN(w/s) + z).
        # Each fp32 operation is done in f64 and rounded to fp32 (53 >= 2 * 24 + 2 bits: the
        # double rounding is innocuous), so t does not depend on how the device's eager fp32
        # division rounds; frac and V are then exact / f64, and V is rounded to fp32 last
        shape = [-1] + [1] * (w.dim() - 1) if per_channel else []
        sf = s64.to(torch.float32).to(torch.float64).reshape(shape)
        zf = (z64.to(torch.float32).to(torch.float64).reshape(shape) if z64 is not None
              else torch.zeros((), dtype=torch.float64, device=w.device))
        q = (w.to(torch.float64) / sf).to(torch.float32)
        t = (q.to(torch.float64) + zf).to(torch.float32).to(torch.float64)
        frac = t - torch.floor(t)
        v = -torch.log((ZETA - GAMMA) / (frac + (-GAMMA)) - 1.0)
        v = torch.nan_to_num(v, nan=0.0, posinf=30.0, neginf=-30.0)   # non-finite w: any V, the clamp decides
        self.V = nn.Parameter(v.to(torch.float32).contiguous())
        return self

    def _need(self):
        if self._q is None or self.V is None:
            raise RuntimeError("AdaRoundWeight: call init_from(w, s, z, lo, hi) first")
        return self._q

    def forward(self, w):
        s, z, lo, hi, axis = self._need()
        if not self.training:
            return self.harden(w)
        if not (torch.is_grad_enabled() and self.V.requires_grad):
            return adaround_forward(w, self.V, s, z, lo, hi, axis=axis)[0]
        y, reg = AdaRoundFn.apply(self.V, w.detach(), s, z, lo, hi, axis, self.lam, self.beta, False)
        self.last_regulariser = reg
        return y

    def regulariser(self, beta=None):
        """The device scalar R = sum(1 - |2h - 1|^beta) of the current V (f64, 0-dim)."""
        s, z, lo, hi, axis = self._need()
        v = self.V.detach()
        return adaround_forward(v, v, s, z, lo, hi, axis=axis, beta=self.beta if beta is None else beta,
                                want_y=False)[1]

    def harden(self, w):
        """y with the hard rounding h = (V >= 0): what the layer computes after AdaRound."""
        s, z, lo, hi, axis = self._need()
        return adaround_forward(w, self.V.detach(), s, z, lo, hi, axis=axis, hard=True)[0]

    def extra_repr(self):
        q = self._q
        return "uninitialised" if q is None else f"grid=[{q[2]}, {q[3]}], axis={q[4]}, shape={tuple(self.V.shape)}"
