"""The typed (bf16 / fp16) entry points of ABI 12 without a GPU: they are exported and
bound, the header and the ctypes binding declare the same signatures, and bad arguments
are rejected on the host before any launch.  The host (CPU) path stays float32-only."""
import os
import re

import pytest
import torch

from vsiquantization_amd import _hip as H
from vsiquantization_amd import fakequant as FQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vsiq.h")
TYPED = ("vsiq_act_fq_fwd_t", "vsiq_act_ste_bwd_t", "vsiq_act_lsq_bwd_t", "vsiq_act_observe_t")

_CTYPE = {"int": H.c_int, "int64_t": H.c_i64, "double": H.c_d}


def header_signatures():
    """name -> [ctypes argument types] of every typed function the header declares."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sigs = {}
    for ret, name, args in re.findall(r"\b(int|int64_t)\s+(vsiq_\w+_t)\s*\(([^)]*)\)\s*;", text):
        assert ret == "int", name
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            types.append(H.c_p if "*" in a else _CTYPE[a.replace("const ", "").rsplit(" ", 1)[0]])
        sigs[name] = types
    return sigs


def test_symbols_exist_and_are_bound():
    lib = H.lib()
    for name in TYPED:
        assert name in H.EXPORTED, name
        assert getattr(lib, name).restype is H.c_int
    assert H.ABI_VERSION >= 12 and lib.vsiq_abi_version() == H.ABI_VERSION
    hdr = open(HEADER).read()
    for name, val in (("F32", H.DT_F32), ("BF16", H.DT_BF16), ("F16", H.DT_F16)):
        assert int(re.search(rf"#define VSIQ_DT_{name} (\d+)", hdr).group(1)) == val


def test_header_and_binding_declare_the_same_signatures():
    sigs = header_signatures()
    assert sorted(sigs) == sorted(TYPED)
    for name, types in sigs.items():
        assert H._SIGS[name][0] == types, name
        assert H._SIGS[name][1] is H.c_int


def _calls(lib, n, dtype, ptr):
    """The four typed entry points on `n` elements of `dtype` with every tensor = ptr."""
    p = ptr
    return {
        "fq": lib.vsiq_act_fq_fwd_t(p, p, None, None, n, dtype, 0, None, None, 1.0, None, 0.0, 0, 0, -128, 127, None),
        "ste": lib.vsiq_act_ste_bwd_t(p, 16 if p else None, None, p, n, dtype, 0, None, 0, 1.0, None),
        "lsq": lib.vsiq_act_lsq_bwd_t(p, p, p, n, dtype, 0, None, 1.0, None, 0.0, 0, -128, 127, 1.0, 16, 16, 1 << 20,
                                      16, None),
        "obs": lib.vsiq_act_observe_t(p, n, dtype, 0, None, None, None, 1, 127.0, 1e-8, 16, 1 << 20, 16, None),
    }


@pytest.mark.parametrize("dtype", [7, -1, 3])
def test_bad_dtype_is_rejected(dtype):
    for n in (0, 16):
        assert set(_calls(H.lib(), n, dtype, 16).values()) == {-1}, n


@pytest.mark.parametrize("dtype", [H.DT_F32, H.DT_BF16, H.DT_F16])
def test_empty_and_null_tensors(dtype):
    lib = H.lib()
    assert set(_calls(lib, 0, dtype, None).values()) == {0}      # n == 0: a no-op
    assert set(_calls(lib, 16, dtype, None).values()) == {-1}    # null tensors
    assert set(_calls(lib, -4, dtype, 16).values()) == {-1}


def test_typed_entries_check_like_their_f32_counterparts():
    lib = H.lib()
    for dt in (H.DT_F32, H.DT_BF16, H.DT_F16):
        # misaligned mask, bad activation, qmin > qmax, workspace too small
        assert lib.vsiq_act_fq_fwd_t(16, 16, None, 12, 16, dt, 0, None, None, 1.0, None, 0.0, 0, 0, -128, 127,
                                     None) == -2
        assert lib.vsiq_act_fq_fwd_t(16, 16, None, None, 16, dt, 3, None, None, 1.0, None, 0.0, 0, 0, -128, 127,
                                     None) == -1
        assert lib.vsiq_act_fq_fwd_t(16, 16, None, None, 16, dt, 0, None, None, 1.0, None, 0.0, 0, 0, 5, 1,
                                     None) == -1
        assert lib.vsiq_act_ste_bwd_t(16, 12, None, 16, 16, dt, 0, None, 0, 1.0, None) == -2
        assert lib.vsiq_act_ste_bwd_t(16, 16, None, 16, 16, dt, 1, None, 0, 1.0, None) == -1   # relu without c
        assert lib.vsiq_act_lsq_bwd_t(16, 16, 16, 16, dt, 0, None, 1.0, None, 0.0, 0, -128, 127, 1.0, 16, 16, 7, 16,
                                      None) == -3
        assert lib.vsiq_act_observe_t(16, 1 << 20, dt, 0, None, None, None, 1, 127.0, 1e-8, 16, 7, 16, None) == -3
    # per-row scales: fp32 only
    for dt in (H.DT_BF16, H.DT_F16):
        assert lib.vsiq_act_ste_bwd_t(16, 16, None, 16, 16, dt, 0, 16, 4, 0.0, None) == -1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_host_path_stays_float32_only(dtype):
    x = torch.randn(64).to(dtype)
    with pytest.raises(TypeError, match=str(dtype).replace("torch.", "")):
        FQ.fake_quant(x, 0.05, 0, -128, 127)
    with pytest.raises(TypeError):
        H.require_device_float(x)
    with pytest.raises(TypeError):
        FQ.observe_tensor(x, symmetric=True)
