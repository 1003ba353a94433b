"""Shared by tests/test_pack_cpu.py and tests/test_gpu_pack.py: a numpy restatement of the
export's packed layout (include/vsiq.h, "Packed codes") -- codes from the oracle's fq_codes
row by row (NaN -> code 0), fields placed with plain integer shifts, an independent
unpacker -- the input builders and the comparisons.  Nothing here touches a GPU."""
import numpy as np
import torch

from oracle.fakequant_np import fq_codes

F32 = np.float32
BITS = (2, 4, 8)


def grid(bits, symmetric):
    """The integer grid of a `bits`-wide quantizer."""
    return (-(2 ** (bits - 1)), 2 ** (bits - 1) - 1) if symmetric else (0, 2 ** bits - 1)


def row_bytes(rowlen, bits):
    return 4 * ((rowlen * bits + 31) // 32)


def f32_qparams(scale, zp, nq, qmin, qmax, zp_round):
    """fp32 [nq, 2]: the (s, z) the kernel must use and export -- fp32(scale), and fp32 of the
    zero point after clamp(rint(zp), qmin, qmax) in f64 when zp_round."""
    s = np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1), (nq,))
    z = np.broadcast_to(np.asarray(0.0 if zp is None else zp, dtype=np.float64).reshape(-1), (nq,))
    if zp_round:
        z = np.clip(np.rint(z), qmin, qmax)
    return np.stack([s.astype(F32), z.astype(F32)], axis=1)


def codes_np(x2, qp, qmin, qmax):
    """int64 [rows, rowlen]: the oracle's code of every element, NaN -> 0; row r with qp[r]
    (or qp[0] when there is one pair)."""
    out = np.empty(x2.shape, dtype=np.int64)
    for r in range(x2.shape[0]):
        s, z = qp[r if qp.shape[0] > 1 else 0]
        with np.errstate(all="ignore"):
            q, _ = fq_codes(x2[r], s, z, qmin, qmax)
        out[r] = np.where(np.isnan(q), 0, q).astype(np.int64)
    return out


def pack_np(codes, qmin, bits):
    """uint8 [rows, row_bytes]: field code - qmin of element e in byte e*bits/8 at bit offset
    (e % (8/bits)) * bits; padding 0."""
    rows, rowlen = codes.shape
    per = 8 // bits
    out = np.zeros((rows, row_bytes(rowlen, bits)), dtype=np.uint8)
    for r in range(rows):
        for e in range(rowlen):
            f = int(codes[r, e]) - qmin
            assert 0 <= f < 2 ** bits
            out[r, (e * bits) // 8] |= f << ((e % per) * bits)
    return out


def pack_np_fast(codes, qmin, bits):
    """pack_np vectorised (the same shifts), for the larger cases."""
    rows, rowlen = codes.shape
    per = 8 // bits
    f = (codes - qmin).astype(np.uint8)
    padded = np.zeros((rows, row_bytes(rowlen, bits) * per), dtype=np.uint8)
    padded[:, :rowlen] = f
    padded = padded.reshape(rows, -1, per)
    out = np.zeros(padded.shape[:2], dtype=np.uint8)
    for k in range(per):
        out |= padded[:, :, k] << (k * bits)
    return out


def unpack_np(data, rowlen, qmin, bits):
    """int64 [rows, rowlen] codes out of a packed buffer (independent of pack_np: it reads
    the row as one little-endian integer)."""
    rows = data.shape[0]
    out = np.empty((rows, rowlen), dtype=np.int64)
    fm = (1 << bits) - 1
    for r in range(rows):
        big = int.from_bytes(data[r].tobytes(), "little")
        for e in range(rowlen):
            out[r, e] = ((big >> (e * bits)) & fm) + qmin
    return out


def dequant_np(codes, qp):
    """fp32 y = (float(q) - z) * s, row r with qp[r] (or qp[0])."""
    s = qp[:, 0:1] if qp.shape[0] > 1 else qp[0, 0]
    z = qp[:, 1:2] if qp.shape[0] > 1 else qp[0, 1]
    with np.errstate(all="ignore"):
        return ((codes.astype(F32) - z).astype(F32) * s).astype(F32)


def padding_mask(rowlen, bits):
    """uint8 [row_bytes]: the bits of a packed row that hold no element."""
    n = row_bytes(rowlen, bits)
    used = (1 << (rowlen * bits)) - 1
    return np.frombuffer((((1 << (8 * n)) - 1) ^ used).to_bytes(n, "little"), dtype=np.uint8)


def same_bits(a, b):
    a = a.detach().cpu().contiguous().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    b = b.detach().cpu().contiguous().numpy() if isinstance(b, torch.Tensor) else np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_bits_but_neg_zero(y, ref):
    """y == ref bit for bit wherever ref is not -0.0, and torch.equal overall."""
    y, ref = y.detach().cpu().reshape(-1), ref.detach().cpu().reshape(-1)
    if not torch.equal(y, ref):
        return False
    yi, ri = y.view(torch.int32), ref.view(torch.int32)
    keep = ri != torch.tensor(-2 ** 31, dtype=torch.int32)
    return bool((yi[keep] == ri[keep]).all())


# ------------------------------------------------------------------------------- inputs
def make_x(rows, rowlen, seed, spread=3.0):
    """fp32 CPU [rows, rowlen]: normal values wide enough to reach both clamp edges, a few
    exact grid points and ties."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, rowlen, generator=g) * spread
    flat = x.reshape(-1)
    n = flat.numel()
    if n >= 4:
        flat[0::7] = torch.round(flat[0::7])          # on-grid for scale 1
        flat[3::11] = torch.round(flat[3::11]) + 0.5  # exact ties for scale 1
    return x.contiguous()


def make_qparams(rows, bits, symmetric, per_row, seed):
    """(scale, zp): f64 CPU tensors [rows] (per_row) or Python numbers; the zero point is 0
    for a symmetric grid, else inside the grid and not an integer (so zp_round matters)."""
    g = torch.Generator().manual_seed(seed + 1000)
    qmin, qmax = grid(bits, symmetric)
    width = qmax - qmin
    s = (6.0 / width) * (0.5 + torch.rand(rows, generator=g, dtype=torch.float64))
    z = torch.zeros(rows, dtype=torch.float64) if symmetric else (
        qmin + width * (0.3 + 0.4 * torch.rand(rows, generator=g, dtype=torch.float64)))
    if per_row:
        return s, z
    return float(s[0]), float(z[0])


def special_x():
    """NaN, +-inf, denormals, exact .5 ties (scale 1) and values beyond both clamp edges."""
    return torch.tensor([float("nan"), float("inf"), float("-inf"), 1e-42, -1e-42, 0.0, -0.0, 0.5, 1.5, 2.5, -0.5,
                         -1.5, -2.5, 1e9, -1e9, 3.0, -3.0, 0.25, -0.25, 1e-30], dtype=torch.float32)


def expected(x2, scale, zp, qmin, qmax, bits, per_row, zp_round):
    """(data uint8 [rows, row_bytes], qparams fp32 [nq, 2], codes int64, y fp32) of the
    numpy restatement for a CPU [rows, rowlen] tensor."""
    v = x2.numpy()
    nq = v.shape[0] if per_row else 1
    to_np = lambda t: t.numpy() if isinstance(t, torch.Tensor) else t   # noqa: E731
    qp = f32_qparams(to_np(scale), None if zp is None else to_np(zp), nq, qmin, qmax, zp_round)
    codes = codes_np(v, qp, qmin, qmax)
    return pack_np_fast(codes, qmin, bits), qp, codes, dequant_np(codes, qp)


def check_packed(p, x2, scale, zp, qmin, qmax, bits, per_row, zp_round, tag):
    """A PackedTensor against the numpy restatement: data byte for byte, qparams bit for
    bit; returns the expected (codes, y)."""
    data, qp, codes, y = expected(x2, scale, zp, qmin, qmax, bits, per_row, zp_round)
    assert same_bits(p.qparams, qp), (tag, "qparams")
    assert same_bits(p.data, data), (tag, "data")
    return codes, y
