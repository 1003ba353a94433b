"""The export format on the host (no GPU): vsiq_host_quantize_pack_f32 and
vsiq_host_unpack_dequant_f32 through fakequant.quantize_pack / unpack_dequant on CPU
tensors, against the numpy restatement of the layout (tests/pack_common.py) and against
the host fake quant.  Every comparison is exact."""
import io

import numpy as np
import pytest
import torch

import vsiquantization_amd as V
from tests import pack_common as P
from vsiquantization_amd import _hip as H
from vsiquantization_amd import host
from vsiquantization_amd.fakequant import PackedTensor, pack_bits_for, quantize_pack, unpack_dequant

SHAPES = ((1, 1), (1, 3), (3, 17), (3, 27), (2, 64), (3, 65), (1, 257), (5, 100))


def test_symbols_and_abi():
    for name in ("vsiq_quantize_pack_f32", "vsiq_unpack_dequant", "vsiq_packed_row_bytes",
                 "vsiq_host_quantize_pack_f32", "vsiq_host_unpack_dequant_f32"):
        assert name in H.EXPORTED
        assert hasattr(H.lib(), name)
    assert H.ABI_VERSION == 13 and H.lib().vsiq_abi_version() == 13
    assert V.PackedTensor is PackedTensor and V.quantize_pack is quantize_pack and V.unpack_dequant is unpack_dequant


@pytest.mark.parametrize("bits", P.BITS)
def test_row_bytes(bits):
    for rowlen in (1, 3, 15, 16, 17, 27, 64, 65, 1152):
        assert H.lib().vsiq_packed_row_bytes(rowlen, bits) == P.row_bytes(rowlen, bits)
    assert H.lib().vsiq_packed_row_bytes(16, 3) == -1


def test_numpy_packers_agree():
    rng = np.random.default_rng(3)
    for bits in P.BITS:
        qmin, qmax = P.grid(bits, True)
        codes = rng.integers(qmin, qmax + 1, size=(3, 29))
        a, b = P.pack_np(codes, qmin, bits), P.pack_np_fast(codes, qmin, bits)
        assert P.same_bits(a, b)
        assert (P.unpack_np(a, 29, qmin, bits) == codes).all()
        assert not (a & P.padding_mask(29, bits)).any()


@pytest.mark.parametrize("bits", P.BITS)
@pytest.mark.parametrize("symmetric", (True, False))
@pytest.mark.parametrize("per_row", (False, True))
def test_host_pack_matches_numpy_and_fake_quant(bits, symmetric, per_row):
    qmin, qmax = P.grid(bits, symmetric)
    for i, (rows, rowlen) in enumerate(SHAPES):
        x = P.make_x(rows, rowlen, seed=10 * bits + i)
        scale, zp = P.make_qparams(rows, bits, symmetric, per_row, seed=i)
        zp_round = not symmetric
        tag = (bits, symmetric, per_row, rows, rowlen)
        if per_row:
            p = quantize_pack(x, scale, zp, qmin, qmax, bits=bits, axis=0, zp_round=zp_round)
        else:
            p = quantize_pack(x.reshape(-1), scale, zp, qmin, qmax, bits=bits, zp_round=zp_round)
        x2 = x if per_row else x.reshape(1, -1)
        codes_ref, y_ref = P.check_packed(p, x2, scale, zp, qmin, qmax, bits, per_row, zp_round, tag)
        assert p.bits == bits and (p.qmin, p.qmax) == (qmin, qmax) and p.axis == (0 if per_row else None)
        y, codes = unpack_dequant(p, want_codes=True)
        assert codes.dtype == (torch.int8 if qmin < 0 else torch.uint8) and codes.shape == p.shape
        assert (codes.reshape(x2.shape).numpy().astype(np.int64) == codes_ref).all(), tag
        assert (P.unpack_np(p.data.numpy(), x2.shape[1], qmin, bits) == codes_ref).all(), tag
        assert P.same_bits(y.reshape(x2.shape), y_ref), tag
        # against the host fake quant, row by row with the row's f64 qparams
        for r in range(x2.shape[0]):
            s_r = scale[r] if per_row else scale
            z_r = zp[r] if per_row else zp
            yh, _, ch = host.fake_quant(x2[r].contiguous(), s_r, z_r, qmin, qmax, zp_round=zp_round, want_codes=True)
            assert torch.equal(codes.reshape(x2.shape)[r], ch), tag
            assert P.same_bits_but_neg_zero(y.reshape(x2.shape)[r], yh), tag
        if per_row:
            yh, _ = host.pc_fake_quant(x, scale, zp, qmin, qmax, zp_round=zp_round)
            assert P.same_bits_but_neg_zero(y, yh), tag


def test_default_bits_and_zero_point_none():
    assert [pack_bits_for(*P.grid(b, s)) for b in (2, 3, 4, 5, 8) for s in (True, False)] == [2, 2, 4, 4, 4, 4, 8, 8,
                                                                                               8, 8]
    x = P.make_x(3, 20, seed=5)
    s = torch.tensor([0.5, 0.25, 1.0], dtype=torch.float64)
    p = quantize_pack(x, s, None, -2, 1, axis=0)
    assert p.bits == 2
    P.check_packed(p, x, s, None, -2, 1, 2, True, False, "zp none")
    p3 = quantize_pack(x, s, None, -4, 3, axis=0)   # a 3-bit grid in 4-bit fields
    assert p3.bits == 4
    codes, y = P.check_packed(p3, x, s, None, -4, 3, 4, True, False, "3 in 4")
    assert P.same_bits(unpack_dequant(p3), y.reshape(x.shape))


@pytest.mark.parametrize("bits", P.BITS)
def test_special_values(bits):
    """NaN -> code 0, +-inf -> the edge codes, ties to even, denormals, beyond both edges."""
    x = P.special_x()
    for symmetric in (True, False):
        qmin, qmax = P.grid(bits, symmetric)
        zp = 0.0 if symmetric else float((qmin + qmax + 1) // 2)
        p = quantize_pack(x, 1.0, zp, qmin, qmax, bits=bits)
        P.check_packed(p, x.reshape(1, -1), 1.0, zp, qmin, qmax, bits, False, False, (bits, symmetric))
        _, codes = unpack_dequant(p, want_codes=True)
        c = codes.to(torch.int64)
        z = int(zp)
        clamp = lambda v: min(max(v, qmin), qmax)   # noqa: E731
        assert int(c[0]) == 0                              # NaN
        assert int(c[1]) == qmax and int(c[2]) == qmin     # +-inf
        assert int(c[3]) == clamp(z) and int(c[4]) == clamp(z)   # denormals
        assert [int(v) for v in c[7:13]] == [clamp(z + k) for k in (0, 2, 2, 0, -2, -2)]   # ties to even
        assert int(c[13]) == qmax and int(c[14]) == qmin   # beyond both edges
        _, _, ch = host.fake_quant(x, 1.0, zp, qmin, qmax, want_codes=True)
        assert torch.equal(codes, ch)


def test_argument_errors():
    x = P.make_x(4, 20, seed=1)
    s4 = torch.full((4,), 0.5, dtype=torch.float64)
    with pytest.raises(ValueError):
        quantize_pack(x, 0.5, 0, -8, 7, bits=3)
    with pytest.raises(ValueError):
        quantize_pack(x, 0.5, 0, -8, 7, bits=2)           # a 4-bit grid in 2-bit fields
    with pytest.raises(ValueError):
        quantize_pack(x, 0.5, 0, -200, 200)               # wider than 8 bits
    with pytest.raises(RuntimeError, match="per-channel scale has 3 entries, the tensor has 4 channels"):
        quantize_pack(x, s4[:3], None, -8, 7, axis=0)
    with pytest.raises(RuntimeError, match="per-channel zero point has 2 entries, the tensor has 4 channels"):
        quantize_pack(x, s4, s4[:2], -8, 7, axis=0)
    with pytest.raises(TypeError):
        quantize_pack(x.double(), 0.5, 0, -8, 7)
    with pytest.raises(TypeError):
        quantize_pack(x.t(), 0.5, 0, -8, 7)               # not contiguous
    with pytest.raises(ValueError):
        quantize_pack(x, 0.5, 0, -8, 7, axis=1)
    with pytest.raises(TypeError):
        unpack_dequant(quantize_pack(x, 0.5, 0, -8, 7), torch.float64)
    # the C entries reject the same before touching memory
    lib, null = H.lib(), None
    buf = torch.zeros(64, dtype=torch.uint8)
    qp = torch.zeros(8, dtype=torch.float32)
    sc = torch.ones(4, dtype=torch.float64)
    for bits, qmin, qmax, nq in ((3, -4, 3, 1), (2, -8, 7, 1), (4, -8, 8, 1), (4, -8, 7, 2), (4, 7, -8, 1)):
        assert lib.vsiq_host_quantize_pack_f32(H.ptr(x), H.ptr(buf), H.ptr(qp), 4, 20, H.ptr(sc), null, nq, 0, qmin,
                                               qmax, bits) == -1
        assert lib.vsiq_quantize_pack_f32(H.ptr(x), H.ptr(buf), H.ptr(qp), 4, 20, H.ptr(sc), null, nq, 0, qmin,
                                          qmax, bits, null) == -1
    assert lib.vsiq_host_unpack_dequant_f32(H.ptr(buf), null, null, 4, 20, H.ptr(qp), 1, -8, 5) == -1
    assert lib.vsiq_unpack_dequant(H.ptr(buf), null, null, 4, 20, H.ptr(qp), 1, -8, 5, 0, null) == -1
    assert lib.vsiq_unpack_dequant(H.ptr(buf), null, null, 4, 20, H.ptr(qp), 3, -8, 4, 0, null) == -1
    assert lib.vsiq_unpack_dequant(H.ptr(buf), null, null, 4, 20, H.ptr(qp), 1, -8, 4, 7, null) == -1


def test_state_round_trip():
    x = P.make_x(6, 27, seed=2)
    s, z = P.make_qparams(6, 4, False, True, seed=2)
    for p in (quantize_pack(x, s, z, 0, 15, axis=0, zp_round=True), quantize_pack(x, 0.3, 0, -2, 1)):
        f = io.BytesIO()
        torch.save(p.state(), f)
        f.seek(0)
        q = PackedTensor.from_state(torch.load(f, weights_only=True))
        assert (q.shape, q.bits, q.qmin, q.qmax, q.axis) == (p.shape, p.bits, p.qmin, p.qmax, p.axis)
        assert P.same_bits(q.data, p.data) and P.same_bits(q.qparams, p.qparams)
        assert P.same_bits(unpack_dequant(q), unpack_dequant(p))
    st = p.state()
    st["data"] = st["data"][:, :-1]
    with pytest.raises(ValueError):
        PackedTensor.from_state(st)


def test_manager_export_on_host():
    """QuantizationManager.export_packed on CPU tensors: the eval quantize's values, no side effects."""
    w = P.make_x(8, 27, seed=9, spread=1.0)
    m = V.QuantizationManager("UniformQuantizer", "MinMaxObserver", 4, True, is_learning_scale=False)
    with pytest.raises(RuntimeError, match="neither observed nor learned"):
        m.export_packed(w)
    y = m.quantize(w)
    before = (float(m.scale), float(m.zero_point), m.observer.min_val, m.observer.max_val, list(m.mean_abs_x))
    p = m.export_packed(w)
    assert (float(m.scale), float(m.zero_point), m.observer.min_val, m.observer.max_val, list(m.mean_abs_x)) == before
    assert p.bits == 4 and p.axis is None and torch.equal(unpack_dequant(p), y)
    m2 = V.QuantizationManager("UniformQuantizer", "MinMaxObserver", 4, True)
    m2.quantizer = object()
    with pytest.raises(NotImplementedError, match="object"):
        m2.export_packed(w)
