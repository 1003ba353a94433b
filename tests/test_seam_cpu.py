"""What a CPU tensor the host loops cannot serve raises, per public entry point.

CPU float32 tensors run the native host loops; every other CPU tensor must fail the way it
always did, whichever module takes the host / device decision.  The table pins the exception
class (not the message) of every entry point that reaches a per-tensor or per-channel op, for
CPU float64 / bfloat16 / float16 tensors, empty float32 tensors and qparams / running state of
the wrong channel count.  ``None``: the call succeeds.  Runs without a GPU.
"""
import pytest
import torch

import vsiquantization_amd as V
from vsiquantization_amd._hip import VsiqError

C = 3
PC_OBSERVER = torch.quantization.MovingAveragePerChannelMinMaxObserver


def _good(shape):
    n = 1
    for d in shape:
        n *= d
    return (torch.arange(n, dtype=torch.float32).reshape(shape) - n / 2) / 4


def _case_tensor(case, shape):
    """The tensor of a case: the entry's good tensor in another dtype, or emptied."""
    if case in ("float64", "bfloat16", "float16"):
        return _good(shape).to(getattr(torch, case))
    if case == "empty_rows":     # the channels are there, each holds nothing
        return torch.empty(shape[:-1] + (0,), dtype=torch.float32)
    if case == "empty_channels":
        return torch.empty((0,) + shape[1:], dtype=torch.float32)
    return _good(shape)          # "wrong_channels": the entry gets C + 1 qparams / state instead


def _qparams(case, grad=False):
    n = C + 1 if case == "wrong_channels" else C
    s = torch.full((n,), 0.05, dtype=torch.float64)
    return (torch.nn.Parameter(s) if grad else s), torch.zeros(n, dtype=torch.float64)


def _grad(x, grad):
    return x.requires_grad_(True) if grad and x.is_floating_point() else x


# --------------------------------------------------------------------------- entry points
def uq_fixed(case, grad):
    x = _grad(_case_tensor(case, (C, 5)), grad)
    return V.UniformQuantizer(8, True).quantize(x, 0.05, 0, False)


def uq_learn(case, grad):
    x = _grad(_case_tensor(case, (C, 5)), grad)
    s = torch.nn.Parameter(torch.tensor(0.05, dtype=torch.float64))
    return V.UniformQuantizer(8, True).quantize(x, s, 0, True)


def pcq_fixed(case, grad):
    x = _grad(_case_tensor(case, (C, 5)), grad)
    s, z = _qparams(case)
    return V.PerChannelUniformQuantizer(8, True).quantize(x, s, z, False)


def pcq_learn(case, grad):
    x = _grad(_case_tensor(case, (C, 5)), grad)
    s, z = _qparams(case, grad=True)
    return V.PerChannelUniformQuantizer(8, True).quantize(x, s, z, True)


def _lsq_module(learn, case):
    """LSQFakeQuantize (per channel, dim 1) calibrated on a good tensor, observer off: the
    next forward is the fake quant alone."""
    fq = V.LSQFakeQuantize(learn_scale=learn, observer=PC_OBSERVER, quant_min=0, quant_max=255, dtype=torch.quint8,
                           qscheme=torch.per_channel_affine, ch_axis=1)
    fq(_good((2, C + 1 if case == "wrong_channels" else C, 4)))
    fq.disable_observer()
    return fq


def _lsq_tensor(case):
    if case == "empty_channels":
        return torch.empty((2, 0, 4), dtype=torch.float32)
    return _case_tensor(case, (2, C, 4))


def lsqm_fixed(case, grad):
    return _lsq_module(False, case)(_grad(_lsq_tensor(case), grad))


def lsqm_learn(case, grad):
    return _lsq_module(True, case)(_grad(_lsq_tensor(case), grad))


def _pc_observer(cls, case):
    obs = cls(True, 4)
    if case == "wrong_channels":   # a stale state: the observer starts a fresh one
        obs.run_min, obs.run_max = torch.zeros(C + 1), torch.zeros(C + 1)
    return obs


def pcmm_observe(case, grad):
    return _pc_observer(V.PerChannelMinMaxObserver, case).observe(_case_tensor(case, (C, 5)))


def pcmm_observe_quantize(case, grad):
    x = _grad(_case_tensor(case, (C, 5)), grad)
    return _pc_observer(V.PerChannelMinMaxObserver, case).observe_quantize(x, V.PerChannelUniformQuantizer(4, True))


def pcmse_observe(case, grad):
    return _pc_observer(V.PerChannelMSEObserver, case).observe(_case_tensor(case, (C, 5)))


def pcmse_observe_quantize(case, grad):
    x = _grad(_case_tensor(case, (C, 5)), grad)
    return _pc_observer(V.PerChannelMSEObserver, case).observe_quantize(x, V.PerChannelUniformQuantizer(4, True))


def minmax(case, grad):
    return V.MinMaxObserver(True, 8).forward(_case_tensor(case, (C, 5)))


def pack(case, grad):
    s, z = _qparams(case)
    return V.quantize_pack(_case_tensor(case, (C, 5)), s, z, -8, 7, axis=0)


def unpack(case, grad):
    """The dtype cases ask for that output dtype; the others build the PackedTensor by hand."""
    if case in ("float64", "bfloat16", "float16", "good"):
        s, z = _qparams(case)
        dtype = torch.float32 if case == "good" else getattr(torch, case)
        return V.unpack_dequant(V.quantize_pack(_good((C, 5)), s, z, -8, 7, axis=0), dtype=dtype)
    shape = {"empty_rows": (C, 0), "empty_channels": (0, 5), "wrong_channels": (C, 5)}[case]
    nq = C + 1 if case == "wrong_channels" else shape[0]
    p = V.PackedTensor(torch.zeros((shape[0], 4), dtype=torch.uint8), shape, 4, -8, 7, torch.ones(nq, 2), axis=0)
    return V.unpack_dequant(p)


def adaround(case, grad):
    w = _case_tensor(case, (C, 5))
    s, z = _qparams(case)
    return V.adaround_forward(w, torch.zeros_like(w), s, z, -8, 7, axis=0, beta=2.0)


# --------------------------------------------------------------------------- the table
CASES = ("float64", "bfloat16", "float16", "empty_rows", "empty_channels", "wrong_channels")

# entry: the class of each case in CASES' order; a pair is (without, with) a gradient-requiring x
TABLE = {
    uq_fixed: (VsiqError, (TypeError, VsiqError), (TypeError, VsiqError), None, None, None),
    uq_learn: (VsiqError, VsiqError, VsiqError, ZeroDivisionError, ZeroDivisionError, None),
    pcq_fixed: (VsiqError, VsiqError, VsiqError, RuntimeError, ValueError, ValueError),
    pcq_learn: (VsiqError, VsiqError, VsiqError, ZeroDivisionError, ZeroDivisionError, RuntimeError),
    lsqm_fixed: (TypeError, TypeError, TypeError, RuntimeError, RuntimeError, RuntimeError),
    lsqm_learn: (TypeError, TypeError, TypeError, ZeroDivisionError, ZeroDivisionError, RuntimeError),
    pcmm_observe: (VsiqError, VsiqError, VsiqError, RuntimeError, RuntimeError, None),
    pcmm_observe_quantize: (VsiqError, VsiqError, VsiqError, RuntimeError, RuntimeError, None),
    pcmse_observe: (VsiqError, VsiqError, VsiqError, RuntimeError, RuntimeError, None),
    pcmse_observe_quantize: (VsiqError, VsiqError, VsiqError, RuntimeError, RuntimeError, None),
    minmax: (VsiqError, TypeError, TypeError, RuntimeError, RuntimeError, None),
    pack: (TypeError, TypeError, TypeError, ValueError, ValueError, RuntimeError),
    unpack: (TypeError, None, None, ValueError, ValueError, ValueError),
    adaround: (TypeError, TypeError, TypeError, ValueError, ValueError, RuntimeError),
}


def outcome(entry, case, grad):
    try:
        entry(case, grad)
    except Exception as e:   # the class is the result
        return type(e)
    return None


@pytest.mark.parametrize("grad", [False, True], ids=["nograd", "grad"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("entry", list(TABLE), ids=lambda f: f.__name__)
def test_cpu_tensor_outcome(entry, case, grad):
    want = TABLE[entry][CASES.index(case)]
    if isinstance(want, tuple):
        want = want[int(grad)]
    got = outcome(entry, case, grad)
    assert got is want, f"{entry.__name__} / {case} / grad={grad}: {got} (expected {want})"


def test_good_tensors_pass():
    """Every entry serves its good CPU float32 tensor (the table's cases fail for their own reason)."""
    for entry in TABLE:
        for grad in (False, True):
            assert outcome(entry, "good", grad) is None, entry.__name__
