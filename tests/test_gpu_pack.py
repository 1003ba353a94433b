"""The export kernels on the GPU: vsiq_quantize_pack_f32 / vsiq_unpack_dequant against the
numpy restatement of the layout (tests/pack_common.py) and against the host loops, at the
seams of the slot grid (16 elements per lane, 256 lanes per workgroup), then the manager,
layer and model level.  Every comparison is exact."""
import io

import numpy as np
import pytest
import torch
import torch.nn as nn

import vsiquantization_amd as V
from tests import pack_common as P
from vsiquantization_amd.fakequant import (PackedTensor, fake_quant, per_channel_fake_quant, quantize_pack,
                                           unpack_dequant)
from vsiquantization_amd.modules import FuseConfig, create_fuse_config_manager, fuse_modules_unified
from vsiquantization_amd.utils.export import export_packed_state, packed_state_weights
from vsiquantization_amd.utils.quantize_manager import (activate_learning_qparam, activate_quantizer,
                                                        calibrate_qat_model, data_calib)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ROWLENS = (1, 3, 15, 16, 17, 27, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1152)
ROWS = (1, 3, 64)


def _dev(v):
    return v.to(DEV) if isinstance(v, torch.Tensor) else v


def _check_case(x, scale, zp, qmin, qmax, bits, per_row, zp_round, tag):
    """One tensor: device pack == numpy == host pack; device unpack == numpy == device fake quant."""
    xd = x.to(DEV)
    axis = 0 if per_row else None
    p = quantize_pack(xd, _dev(scale), _dev(zp), qmin, qmax, bits=bits, axis=axis, zp_round=zp_round)
    x2 = x if per_row else x.reshape(1, -1)
    codes_ref, y_ref = P.check_packed(p, x2, scale, zp, qmin, qmax, bits, per_row, zp_round, tag)
    ph = quantize_pack(x, scale, zp, qmin, qmax, bits=bits, axis=axis, zp_round=zp_round)
    assert P.same_bits(p.data, ph.data) and P.same_bits(p.qparams, ph.qparams), tag
    y, codes = unpack_dequant(p, want_codes=True)
    assert (codes.cpu().reshape(x2.shape).numpy().astype(np.int64) == codes_ref).all(), tag
    assert P.same_bits(y.reshape(x2.shape), y_ref), tag
    yh, ch = unpack_dequant(ph, want_codes=True)
    assert P.same_bits(y, yh) and P.same_bits(codes, ch), tag
    if per_row:
        yf, _, cf = per_channel_fake_quant(xd, _dev(scale), _dev(zp), qmin, qmax, zp_round=zp_round, want_codes=True)
    else:
        yf, _, cf = fake_quant(xd, scale, zp, qmin, qmax, zp_round=zp_round, want_codes=True)
    assert torch.equal(codes, cf), tag
    assert P.same_bits_but_neg_zero(y, yf), tag
    return p


@pytest.mark.parametrize("bits", P.BITS)
@pytest.mark.parametrize("rows", ROWS)
def test_seams(bits, rows):
    """Every rowlen seam, symmetric and asymmetric, nq = 1 and nq = rows."""
    for i, rowlen in enumerate(ROWLENS):
        x = P.make_x(rows, rowlen, seed=100 * bits + 10 * rows + i)
        for symmetric in (True, False):
            qmin, qmax = P.grid(bits, symmetric)
            s, z = P.make_qparams(rows, bits, symmetric, True, seed=i)
            _check_case(x, s, z, qmin, qmax, bits, True, not symmetric, (bits, rows, rowlen, symmetric, "rows"))
        # nq = 1 on the same elements as one row (per tensor)
        symmetric = i % 2 == 0
        qmin, qmax = P.grid(bits, symmetric)
        s, z = P.make_qparams(rows, bits, symmetric, False, seed=i)
        _check_case(x.reshape(-1), s, z, qmin, qmax, bits, False, not symmetric, (bits, rows, rowlen, symmetric, "one"))


@pytest.mark.parametrize("bits", P.BITS)
def test_per_tensor_several_workgroups(bits):
    """~70 000 elements in one row: 18 workgroups and a ragged tail (n % 16 = 13, n % 4 = 1)."""
    n = 70_013
    x = P.make_x(1, n, seed=bits).reshape(-1)
    for symmetric in (True, False):
        qmin, qmax = P.grid(bits, symmetric)
        s, z = P.make_qparams(1, bits, symmetric, False, seed=bits)
        _check_case(x, s, z, qmin, qmax, bits, False, not symmetric, (bits, symmetric, n))


def test_unaligned_rows_view():
    """A tensor whose storage is not 16-byte aligned takes the scalar-load path: same bytes."""
    base = P.make_x(1, 64 * 40 + 1, seed=4).reshape(-1)
    x = base[1:].reshape(64, 40)
    xd = base.to(DEV)[1:].reshape(64, 40)
    assert xd.data_ptr() % 16 != 0 and xd.is_contiguous()
    s, z = P.make_qparams(64, 4, False, True, seed=4)
    p = quantize_pack(xd, s.to(DEV), z.to(DEV), 0, 15, axis=0, zp_round=True)
    P.check_packed(p, x.contiguous(), s, z, 0, 15, 4, True, True, "unaligned")


@pytest.mark.parametrize("bits", P.BITS)
def test_special_values(bits):
    x = P.special_x()
    for symmetric in (True, False):
        qmin, qmax = P.grid(bits, symmetric)
        zp = 0.0 if symmetric else float((qmin + qmax + 1) // 2)
        p = quantize_pack(x.to(DEV), 1.0, zp, qmin, qmax, bits=bits)
        codes_ref, _ = P.check_packed(p, x.reshape(1, -1), 1.0, zp, qmin, qmax, bits, False, False, (bits, symmetric))
        assert codes_ref[0, 0] == 0 and codes_ref[0, 1] == qmax and codes_ref[0, 2] == qmin
        _, codes = unpack_dequant(p, want_codes=True)
        assert (codes.cpu().numpy().astype(np.int64) == codes_ref[0]).all()
        assert torch.equal(codes, fake_quant(x.to(DEV), 1.0, zp, qmin, qmax, want_codes=True)[2])


@pytest.mark.parametrize("bits", P.BITS)
def test_padding_bits_are_zero(bits, monkeypatch):
    """The kernel writes every byte of `packed`, padding as 0, whatever the buffer held."""
    real_empty = torch.empty

    def dirty_empty(*a, **k):
        t = real_empty(*a, **k)
        if t.dtype == torch.uint8:
            t.fill_(0xFF)
        return t

    import vsiquantization_amd.fakequant as FQ
    monkeypatch.setattr(FQ.torch, "empty", dirty_empty)
    qmin, qmax = P.grid(bits, True)
    for rows, rowlen in ((3, 1), (3, 17), (64, 27), (3, 65), (1, 1025), (3, 1152)):
        x = P.make_x(rows, rowlen, seed=rowlen)
        s, z = P.make_qparams(rows, bits, True, True, seed=rowlen)
        p = quantize_pack(x.to(DEV), s.to(DEV), None, qmin, qmax, bits=bits, axis=0)
        data = p.data.cpu().numpy()
        assert not (data & P.padding_mask(rowlen, bits)[None, :]).any(), (bits, rows, rowlen)
        P.check_packed(p, x, s, None, qmin, qmax, bits, True, False, (bits, rows, rowlen))


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16))
def test_16_bit_output(dtype):
    for bits, (rows, rowlen) in zip(P.BITS, ((64, 27), (3, 1152), (3, 257))):
        qmin, qmax = P.grid(bits, False)
        x = P.make_x(rows, rowlen, seed=bits)
        s, z = P.make_qparams(rows, bits, False, True, seed=bits)
        p = quantize_pack(x.to(DEV), s.to(DEV), z.to(DEV), qmin, qmax, axis=0, zp_round=True)
        y32 = unpack_dequant(p)
        y16, codes = unpack_dequant(p, dtype, want_codes=True)
        assert y16.dtype == dtype and P.same_bits(y16.view(torch.int16), y32.to(dtype).view(torch.int16))
        assert torch.equal(codes, unpack_dequant(p, want_codes=True)[1])


# ------------------------------------------------------------------------------- manager
def _snapshot(m):
    def val(v):
        return v.detach().clone() if isinstance(v, torch.Tensor) else v
    obs = m.observer
    return dict(scale=val(m.scale), zp=val(m.zero_point), mn=val(getattr(obs, "min_val", None)),
                mx=val(getattr(obs, "max_val", None)), stats=(list(m.mean_abs_x), list(m.mean_x), list(m.std)),
                flags=(m.is_learning_scale, m.is_quantize, m.is_observer_qparam))


def _same_snapshot(a, b):
    for k in a:
        u, v = a[k], b[k]
        if isinstance(u, torch.Tensor):
            if not (isinstance(v, torch.Tensor) and u.dtype == v.dtype and torch.equal(u, v)):
                return False
        elif u != v:
            return False
    return True


MANAGERS = (("UniformQuantizer", "MinMaxObserver", 4, True), ("UniformQuantizer", "MinMaxObserver", 8, False),
            ("LSQQuantizer", "MinMaxObserver", 4, False), ("PerChannelUniformQuantizer", "PerChannelMinMaxObserver", 2, True),
            ("PerChannelUniformQuantizer", "PerChannelMinMaxObserver", 4, False))


# (the reference UniformQuantizer cannot learn an integer zero point: asymmetric + learnable is LSQQuantizer's)
MANAGER_CASES = [(*m, learn) for m in MANAGERS for learn in (False, True)
                 if not (learn and m[0] == "UniformQuantizer" and not m[3])]


@pytest.mark.parametrize("quantizer,observer,bits,symmetric,learn", MANAGER_CASES)
def test_manager_export_no_side_effects(quantizer, observer, bits, symmetric, learn):
    w = (P.make_x(16, 27, seed=bits, spread=0.5) + (0.0 if symmetric else 0.3)).to(DEV)
    m = V.QuantizationManager(quantizer, observer, bits, symmetric, is_learning_scale=False).to(DEV)
    with pytest.raises(RuntimeError):
        m.export_packed(w)
    m.quantize(w)   # calibrate
    if learn:
        m.is_learning_scale = True
        m.make_learn_qparameter()
        with torch.no_grad():   # a learned, off-grid state: scale moved, zero point not an integer
            m.scale.mul_(1.07)
            if isinstance(m.zero_point, torch.Tensor) and m.zero_point.requires_grad:
                m.zero_point.add_(0.37)
    m.eval()
    with torch.no_grad():
        y = m.quantize(w)
    before = _snapshot(m)
    p = m.export_packed(w)
    assert _same_snapshot(before, _snapshot(m))
    per_channel = quantizer.startswith("PerChannel")
    assert p.axis == (0 if per_channel else None) and p.qparams.shape[0] == (16 if per_channel else 1)
    assert (p.qmin, p.qmax) == (m.quantizer.qmin, m.quantizer.qmax) and p.bits == bits
    assert torch.equal(unpack_dequant(p), y)
    with torch.no_grad():
        assert torch.equal(m.quantize(w), y)   # and the manager still computes the same


def test_manager_rejects_other_quantizers():
    m = V.QuantizationManager("UniformQuantizer", "MinMaxObserver", 4, True).to(DEV)

    class Other(V.UniformQuantizer):
        pass

    m.quantizer = Other(4, True)
    m.scale = 0.1
    with pytest.raises(NotImplementedError, match="Other"):
        m.export_packed(torch.zeros(4, 4, device=DEV))


# --------------------------------------------------------------------------------- model
def _model():
    torch.manual_seed(0)
    m = nn.Sequential(nn.Conv2d(3, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8), nn.ReLU(), nn.Flatten(),
                      nn.Linear(8 * 8 * 8, 10))
    bn = m[1]
    bn.running_mean.uniform_(-0.3, 0.3)
    bn.running_var.uniform_(0.5, 2.0)
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.uniform_(-0.2, 0.2)
    cfg = create_fuse_config_manager(FuseConfig(bits_w=2, bits_a=4))
    return fuse_modules_unified(m, [["conv", "bn", "relu"], ["linear"]], is_trace=False, config_manager=cfg).to(DEV)


def _loader():
    g = torch.Generator().manual_seed(5)
    return [(torch.randint(0, 256, (2, 3, 8, 8), generator=g, dtype=torch.uint8), None) for _ in range(2)]


@pytest.mark.parametrize("learn", (False, True))
def test_model_export_round_trip(learn):
    model = _model()
    calibrate_qat_model(model, _loader(), data_calib, DEV)
    if learn:
        activate_learning_qparam(model)
    activate_quantizer(model)
    model.eval()
    layers = {n: l for n, l in model.named_modules() if isinstance(l, V.FakeQuantize)}
    assert sorted(layers) == ["0", "4"]
    assert isinstance(layers["0"], V.modules.ConvBnReLU) and (layers["0"].bits_w, layers["0"].bits_a) == (2, 4)
    state = export_packed_state(model)
    f = io.BytesIO()
    torch.save(state, f)
    f.seek(0)
    loaded = torch.load(f, weights_only=True)
    assert sorted(loaded) == ["0", "4"]
    weights = packed_state_weights(loaded, device=DEV)
    for name, layer in layers.items():
        w, b = layer.get_weight_bias()
        with torch.no_grad():
            ref = layer.quantize_weights(w)
        assert loaded[name]["weight"]["bits"] == 2 and weights[name].shape == w.shape
        assert torch.equal(weights[name], ref), name
        if b is None:
            assert loaded[name]["bias"] is None
        else:
            assert torch.equal(loaded[name]["bias"].to(DEV), b.detach())
    p, _ = layers["0"].export_packed_weight()
    assert isinstance(p, PackedTensor) and P.same_bits(p.data, loaded["0"]["weight"]["data"])


# --------------------------------------------------------------------------------- graph
def test_graph_capture():
    x = P.make_x(64, 27, seed=8).to(DEV)
    s, z = (t.to(DEV) for t in P.make_qparams(64, 4, False, True, seed=8))
    eager = quantize_pack(x, s, z, 0, 15, axis=0, zp_round=True)
    y_eager = unpack_dequant(eager, torch.bfloat16)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        quantize_pack(x, s, z, 0, 15, axis=0, zp_round=True)   # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(st)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        p = quantize_pack(x, s, z, 0, 15, axis=0, zp_round=True)
        y = unpack_dequant(p, torch.bfloat16)
    p.data.zero_()
    p.qparams.zero_()
    y.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert P.same_bits(p.data, eager.data) and P.same_bits(p.qparams, eager.qparams)
    assert P.same_bits(y.view(torch.int16), y_eager.view(torch.int16))
