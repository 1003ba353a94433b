"""Hadamard-rotated MX fake quantization without a GPU: the entry points (csrc/k_mx_rot.hip) are exported, declared
alike in the header and the binding and check their arguments before any launch; the CPU-tensor route (the host
loops composed) equals the numpy restatement; the registry name resolves."""
import os
import re

import numpy as np
import pytest
import torch

import vsiquantization_amd as V
from tests import mx_common as M
from tests import rot_common as R
from vsiquantization_amd import _hip as H

NAMES = ("vsiq_mx_rot_fq_fwd_f32", "vsiq_mx_rot_fq_fwd_cols_f32", "vsiq_mx_rot_ste_bwd_f32",
         "vsiq_mx_rot_ste_bwd_cols_f32")
CTYPES = {"const float *": H.c_p, "float *": H.c_p, "uint8_t *": H.c_p, "uint64_t *": H.c_p, "const uint64_t *": H.c_p,
          "void *": H.c_p, "int64_t": H.c_i64, "int": H.c_int}


@pytest.mark.parametrize("name", NAMES)
def test_entries_are_exported_and_declared_alike_in_header_and_binding(name):
    assert name in H.EXPORTED and hasattr(H.lib(), name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vsiq.h")).read()
    args = re.search(r"\bint %s\(([^)]*)\);" % name, header).group(1)
    types = [re.sub(r"\s*\w+$", "", " ".join(a.split())) for a in args.split(",")]
    assert ([CTYPES[t] for t in types], H.c_int) == H._SIGS[name]


def test_arguments_are_checked_before_any_launch():
    lib = H.lib()
    fr, fc, br, bc = (getattr(lib, n) for n in NAMES)
    assert fr(16, 32, None, None, None, None, 2, 33, 0, None) == -1         # length 33
    assert fc(16, 32, None, None, None, None, 1, 33, 8, 0, None) == -1
    assert br(16, 8, 32, 2, 33, None) == -1 and bc(16, 8, 32, 1, 33, 8, None) == -1
    assert fr(16, 32, None, None, None, None, 2, 32, 9, None) == -1         # format 9
    assert fc(16, 32, None, None, None, None, 1, 32, 8, 9, None) == -1
    for r, n in ((0, 32), (2, 0), (1 << 40, 1 << 40), (1 << 31, 256)):      # sizes, overflow, 2^31 chunks
        assert fr(16, 32, None, None, None, None, r, n, 0, None) == -1 and br(16, 8, 32, r, n, None) == -1
    assert fc(16, 32, None, None, None, None, 1 << 31, 32, 256, 0, None) == -1
    assert fr(None, 32, None, None, None, None, 2, 32, 0, None) == -1       # no x; outputs without y
    assert fr(16, None, 48, None, None, None, 2, 32, 0, None) == -1
    assert fc(16, None, None, 48, None, None, 1, 32, 8, 0, None) == -1
    assert br(16, None, 32, 2, 32, None) == -1 and bc(16, 8, None, 1, 32, 8, None) == -1   # no mask, no gx
    assert fr(16, 32, None, None, None, 12, 2, 32, 0, None) == -2           # mask not 8-byte aligned
    assert fc(16, 32, None, None, None, 12, 1, 32, 8, 0, None) == -2
    assert br(16, 12, 32, 2, 32, None) == -2 and bc(16, 12, 32, 1, 32, 8, None) == -2


@pytest.mark.parametrize("fmt", ["fp4_e2m1", "fp8_e4m3"])
@pytest.mark.parametrize("shape", [(3, 96), (2, 64, 5)], ids=["rows", "columns"])
def test_cpu_tensors_equal_the_numpy_restatement(shape, fmt):
    cols = len(shape) == 3
    n = int(np.prod(shape))
    x, g = (R.inputs(1, n, s).reshape(shape) for s in (5, 6))
    rows = lambda t: np.ascontiguousarray(t.numpy().transpose(0, 2, 1) if cols else t.numpy())   # noqa: E731
    back = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1) if cols else a)                    # noqa: E731
    yr, codes, scales, mask = M.ref_rows(R.hadamard_np(rows(x), 32).reshape(-1, shape[1]), fmt)
    want = back(R.hadamard_np(yr, 32).reshape(rows(x).shape))
    assert (mask == 0).any() and (mask == 1).any()
    xt = x.clone().requires_grad_(True)
    axis = 1 if cols else -1
    y = V.mx_rot_fake_quant(xt, fmt, axis=axis)
    assert np.array_equal(M.bits(y.detach().numpy()), M.bits(want))
    y2, c2, s2 = V.mx_rot_fake_quant(x, fmt, axis=axis, want_codes=True)
    assert np.array_equal(M.bits(y2.numpy()), M.bits(want))
    assert np.array_equal(c2.numpy(), back(codes.reshape(rows(x).shape)))
    assert np.array_equal(s2.numpy(), back(scales.reshape(rows(x).shape[:-1] + (-1,))))
    y.backward(g)
    keep = np.where(mask.reshape(rows(x).shape) == 1, R.hadamard_np(rows(g), 32), np.float32(0))
    assert np.array_equal(M.bits(xt.grad.numpy()), M.bits(back(R.hadamard_np(keep, 32))))
    with pytest.raises(ValueError, match="multiple of 32"):
        V.mx_rot_fake_quant(torch.zeros(4, 40), fmt)


def test_the_registry_name_resolves_to_a_self_scaled_mx_quantizer():
    q = V.CLASS_REGISTRY["RotatedMXQuantizer"](4, True)
    assert type(q) is V.RotatedMXQuantizer and isinstance(q, V.MXQuantizer) and q.self_scaled
    assert q.elem_format == "fp4_e2m1" and q.block_axis == -1
    m = V.QuantizationManager("RotatedMXQuantizer", "MinMaxObserver", 4, True, is_learning_scale=False)
    x = R.inputs(2, 64, 1)
    codes, scales, fmt = m.export_mx(x)
    assert torch.equal(V.hadamard_transform(V.mx_dequant(codes, scales, fmt), 32), m.quantize(x))
    with pytest.raises(NotImplementedError):
        m.export_packed(x)
