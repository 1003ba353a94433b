"""numpy restatement of MX block-scaled fake quantization (OCP Microscaling v1.0, as
include/vsiq.h states it) and the inputs that pin it, for test_mx_cpu.py.

Written differently from the library's element code (csrc/k_mx.cuh) on purpose: every format's non-negative
grid, extended by the overflow value, is enumerated as float64; an element is the grid point
of the smallest |a - g| (ties to the even code), then saturated and rescaled with np.ldexp.
No rounding trick, no bit arithmetic on the value.
"""
import numpy as np

# name -> (VSIQ_MX_* code, bits, exponent bits, mantissa bits, bias, emax, max normal, overflow value)
FORMATS = {
    "fp4_e2m1": (0, 4, 2, 1, 1, 2, 6.0, 8.0),
    "fp6_e2m3": (1, 6, 2, 3, 1, 2, 7.5, 8.0),
    "fp6_e3m2": (2, 6, 3, 2, 3, 4, 28.0, 32.0),
    "fp8_e4m3": (3, 8, 4, 3, 7, 8, 448.0, 480.0),
    "fp8_e5m2": (4, 8, 5, 2, 15, 15, 57344.0, 65536.0),
}
NAMES = tuple(FORMATS)
NAN_BITS = 0x7FC00000

ROW_SHAPES = [(1, 1), (1, 31), (1, 32), (1, 33), (3, 27), (2, 64), (3, 144), (5, 100), (1, 257)]
COL_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 32, 1), (2, 33, 7), (1, 64, 65)]


def grid(fmt):
    """The format's non-negative values in code order (index == magnitude code), then the
    overflow value, as float64."""
    _, _, ebits, mbits, bias, _, maxn, ovf = FORMATS[fmt]
    vals = []
    for eb in range(1 << ebits):
        for m in range(1 << mbits):
            v = m * 2.0 ** (1 - bias - mbits) if eb == 0 else (1 + m / (1 << mbits)) * 2.0 ** (eb - bias)
            if v <= maxn:   # e4m3's S.1111.111 and e5m2's top exponent are NaN / Inf, not values
                vals.append(v)
    assert vals == sorted(set(vals)) and vals[-1] == maxn
    return np.array(vals + [ovf], dtype=np.float64)


def _nearest(a, g):
    """Index of the grid point nearest each a (float64); a tie goes to the even index."""
    d = np.abs(a[:, None] - g[None, :])
    i = np.argmin(d, axis=1)   # the first minimum: the lower neighbour of a tie
    nxt = np.minimum(i + 1, len(g) - 1)
    rows = np.arange(len(a))
    tie = (nxt != i) & (d[rows, nxt] == d[rows, i])
    return np.where(tie & (i % 2 == 1), nxt, i)


def ref_rows(x, fmt):
    """x float32 [rows, rowlen] -> (y float32, codes uint8, scales uint8 [rows, blocks],
    mask uint8), blocks of 32 along each row."""
    _, bits, _, _, _, emax, _, _ = FORMATS[fmt]
    g = grid(fmt)
    top = len(g) - 2   # code of max normal
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, rowlen = x.shape
    nb = -(-rowlen // 32)
    y = np.empty_like(x)
    codes = np.zeros(x.shape, np.uint8)
    mask = np.zeros(x.shape, np.uint8)
    scales = np.zeros((rows, nb), np.uint8)
    for r in range(rows):
        for b in range(nb):
            sl = slice(32 * b, min(32 * b + 32, rowlen))
            v = x[r, sl]
            if not np.all(np.isfinite(v)):
                y[r, sl] = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
                scales[r, b] = 255
                continue
            mag = np.abs(v.astype(np.float64))
            amax = mag.max()
            E = -127 if amax == 0 else int(np.clip(np.frexp(amax)[1] - 1 - emax, -127, 127))
            idx = _nearest(np.ldexp(mag, -E), g)
            mask[r, sl] = idx <= top
            idx = np.minimum(idx, top)
            q = np.ldexp(g[idx], E)
            y32 = q.astype(np.float32)
            assert np.array_equal(y32.astype(np.float64), q), "y must be exact in fp32"
            neg = np.signbit(v)
            y[r, sl] = np.where(neg, -y32, y32)
            codes[r, sl] = idx | (neg.astype(np.int64) << (bits - 1))
            scales[r, b] = E + 127
    return y, codes, scales, mask


def ref_cols(x, fmt):
    """x float32 [outer, C, inner], blocks of 32 along C -> (y, codes, scales uint8 [outer,
    blocks, inner], mask): the row restatement on the [outer * inner, C] transpose."""
    o, c, n = x.shape
    y, codes, scales, mask = ref_rows(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(o * n, c), fmt)
    back = lambda t: np.ascontiguousarray(t.reshape(o, n, -1).transpose(0, 2, 1))   # noqa: E731
    return back(y), back(codes), back(scales), back(mask)


PIN_EXPONENTS = (-127, 0, 100)


def scaled_values(fmt):
    """The scaled magnitudes a that pin the rounding, float64 (all exact in fp32): every grid
    point, every midpoint between neighbours (the one below the overflow value included),
    values in (max normal, 2^(emax + 1)) and 0."""
    emax, maxn = FORMATS[fmt][5], FORMATS[fmt][6]
    g = grid(fmt)
    mids = (g[:-1] + g[1:]) / 2
    top = 2.0 ** (emax + 1)
    over = maxn + (top - maxn) * np.array([0.03125, 0.25, 0.5, 0.75, 0.96875])
    return g[:-1], mids, over[over < top]


def builder_blocks(fmt, k):
    """float32 [blocks, 32]: one pin of magnitude 2^(k + emax) per block, which fixes E = k, and
    31 test values beside it: scaled_values * 2^k, the fp32 neighbours either side of every
    scaled midpoint, both signs, +-0."""
    emax = FORMATS[fmt][5]
    pts, mids, over = scaled_values(fmt)
    f32 = lambda a: np.ldexp(a, k).astype(np.float32)   # noqa: E731
    m32 = f32(mids)
    vals = np.concatenate([f32(pts), m32, np.nextafter(m32, np.float32(np.inf)), np.nextafter(m32, np.float32(0)),
                           f32(over), np.zeros(1, np.float32)])
    vals = np.concatenate([vals, -vals])
    pad = (-len(vals)) % 31
    vals = np.concatenate([vals, np.zeros(pad, np.float32)]).reshape(-1, 31)
    pin = np.full((len(vals), 1), np.ldexp(1.0, k + emax), np.float32)
    pin[1::2] *= -1
    return np.ascontiguousarray(np.concatenate([vals[:, :7], pin, vals[:, 7:]], axis=1))


def builder(fmt):
    """Every pinned block of the format: [blocks, 32] float32, E in PIN_EXPONENTS."""
    return np.concatenate([builder_blocks(fmt, k) for k in PIN_EXPONENTS])


def special_blocks():
    """[blocks, 32] float32: all-zero blocks of both signs, a block of fp32 denormals only, a
    block at 3e38, blocks holding one NaN, one +Inf, one -Inf."""
    rng = np.random.default_rng(7)
    z = np.zeros(32, np.float32)
    den = (rng.integers(1, 1 << 23, 32).astype(np.uint32)).view(np.float32) * np.where(rng.random(32) < 0.5, -1, 1)
    big = (rng.uniform(-1, 1, 32) * 3e38).astype(np.float32)
    big[5] = 3e38
    out = [z, -z, np.where(np.arange(32) % 3 == 0, -z, z), den.astype(np.float32), big]
    for bad in (np.nan, np.inf, -np.inf):
        b = rng.standard_normal(32).astype(np.float32)
        b[11] = bad
        out.append(b)
    return np.stack(out).astype(np.float32)


def ragged_rows():
    """[2, 40] float32: the last block of a row is 8 long and its maximum sits in its final element."""
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 40)).astype(np.float32)
    x[:, 39] = (-1000.0, 517.0)
    return x


def gaussian(shape, seed):
    """Seeded Gaussians whose rows differ in scale by many binades (some elements overflow)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    x *= np.exp2(rng.integers(-20, 20, shape[:1] + (1,) * (len(shape) - 1)).astype(np.float64))
    return x.astype(np.float32)


def fill(shape, fmt):
    """``shape`` filled from the builder's stream of values (cycled): the pinned roundings at
    every row length, with whatever block maxima the cut produces."""
    return np.resize(builder(fmt).reshape(-1), shape).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

