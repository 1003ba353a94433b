"""The typed records-only learnable backward of ABI 13 (K4d, vsiq_act_lsq_bwd_part_t)
without a GPU: it is exported and bound, the header and the ctypes binding declare the
same signature, and bad arguments get the code vsiq_act_lsq_bwd_part_f32 gives them, on
the host, before any launch."""
import os
import re

import pytest
import torch

from vsiquantization_amd import _hip as H
from vsiquantization_amd.quantizers import deferred as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vsiq.h")
NAME = "vsiq_act_lsq_bwd_part_t"
E_ARG, E_WS = -1, -3

_CTYPE = {"int": H.c_int, "int64_t": H.c_i64, "double": H.c_d}


def header_signatures():
    """name -> [ctypes argument types] of every typed function the header declares
    (tests/test_half_cpu.py's parser, which also drops line comments)."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    sigs = {}
    for ret, name, args in re.findall(r"\b(int|int64_t)\s+(vsiq_\w+_t)\s*\(([^)]*)\)\s*;", text):
        assert ret == "int", name
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            types.append(H.c_p if "*" in a else _CTYPE[a.replace("const ", "").rsplit(" ", 1)[0]])
        sigs[name] = types
    return sigs


def test_symbol_is_exported_and_bound():
    lib = H.lib()
    assert NAME in H.EXPORTED
    assert getattr(lib, NAME).restype is H.c_int
    assert H.ABI_VERSION == 13 == lib.vsiq_abi_version()
    hdr = open(HEADER).read()
    assert int(re.search(r"#define VSIQ_ABI_VERSION (\d+)", hdr).group(1)) == 13


def test_header_and_binding_declare_the_same_signature():
    sigs = header_signatures()
    assert NAME in sigs
    for name, types in sigs.items():      # the ABI 12 entries too, through this parser
        assert H._SIGS[name][0] == types, name
        assert H._SIGS[name][1] is H.c_int
    # dtype sits right after n, everything else is the _f32 entry's argument list
    f32 = list(H._SIGS["vsiq_act_lsq_bwd_part_f32"][0])
    assert sigs[NAME] == f32[:4] + [H.c_int] + f32[4:]
    assert list(getattr(H.lib(), NAME).argtypes) == sigs[NAME]


def _typed(lib, dtype, g=16, c=16, gc=16, n=16, act=0, zp_learn=0, qmin=-8, qmax=7, rec=16, rec_len=2):
    return lib.vsiq_act_lsq_bwd_part_t(g, c, gc, n, dtype, act, None, 1.0, None, 0.0, zp_learn, qmin, qmax, rec,
                                       rec_len, None)


def _f32(lib, g=16, c=16, gc=16, n=16, act=0, zp_learn=0, qmin=-8, qmax=7, rec=16, rec_len=2):
    return lib.vsiq_act_lsq_bwd_part_f32(g, c, gc, n, act, None, 1.0, None, 0.0, zp_learn, qmin, qmax, rec, rec_len,
                                         None)


@pytest.mark.parametrize("dtype", [7, -1, 3])
def test_bad_dtype_is_rejected(dtype):
    for n in (0, 16):
        assert _typed(H.lib(), dtype, n=n) == E_ARG


# every one of these is rejected before a launch: the pointers are never dereferenced
BAD = {
    "null g": (dict(g=None), E_ARG),
    "null c": (dict(c=None), E_ARG),
    "null gc": (dict(gc=None), E_ARG),
    "null records": (dict(rec=None), E_ARG),
    "negative n": (dict(n=-4), E_ARG),
    "short records": (dict(rec_len=1), E_WS),
    "short records, several workgroups": (dict(n=4097, rec_len=2 * 3 - 1), E_WS),
    "qmin > qmax": (dict(qmin=5, qmax=1), E_ARG),
    "bad act": (dict(act=3), E_ARG),
    "zp_learn 2": (dict(zp_learn=2), E_ARG),
    "zp_learn -1": (dict(zp_learn=-1), E_ARG),
    # the order of the checks: the workspace before zp_learn, the arguments before both
    "short records and zp_learn 2": (dict(rec_len=1, zp_learn=2), E_WS),
    "bad act and short records": (dict(act=3, rec_len=1), E_ARG),
}


@pytest.mark.parametrize("dtype", [H.DT_F32, H.DT_BF16, H.DT_F16])
@pytest.mark.parametrize("case", sorted(BAD))
def test_return_codes_are_the_f32_entry_s(dtype, case):
    lib = H.lib()
    kw, code = BAD[case]
    assert _f32(lib, **kw) == code
    assert _typed(lib, dtype, **kw) == code


@pytest.mark.parametrize("dtype", [H.DT_F32, H.DT_BF16, H.DT_F16])
def test_empty_tensor_is_a_no_op(dtype):
    lib = H.lib()
    assert _typed(lib, dtype, n=0) == 0
    assert _typed(lib, dtype, g=None, c=None, gc=None, rec=None, rec_len=0, n=0) == 0


def test_record_count_depends_on_n_only():
    lib = H.lib()
    assert lib.vsiq_lsq_part_records(4097) == 3      # what the E_WS case above stands on
    assert lib.vsiq_lsq_part_records(2048) == 1 and lib.vsiq_lsq_part_records(2049) == 2


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cpu_half_tensor_is_a_type_error(dtype):
    x = torch.randn(64).to(dtype)
    records = torch.empty(2, dtype=torch.float64)
    with pytest.raises(TypeError, match=str(dtype).replace("torch.", "")):
        D.lsq_backward_part(x, x, 0.05, 0, -128, 127, False, None, records)
    with pytest.raises(TypeError):
        D.DeferredLearnFn.apply(x, 0.05, 0, -128, 127, 1.0, False, None)
