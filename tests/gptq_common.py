"""Shared by test_gptq_cpu.py and test_gpu_gptq.py: vsiq_pg_gptq_f32's contract (include/vsiq.h)
as a float64 numpy loop, and the inputs (the same fp32 U for every path).  A rounding that flips
between fp32 and f64 cascades down its row: the seeds were chosen once, on the CPU, as ones where
the host loops have no flip against the reference."""
import functools

import numpy as np

from oracle import fakequant_np as O

# (rows, rowlen, G, symmetric, bits, seed).  rows 67: a partial second tile; rowlen == G: one group,
# no trailing update (32 and 64: a block narrower than 128); 256: one trailing update; 384: columns
# updated by two successive blocks.
CASES = ((1, 32, 32, True, 4, 0), (5, 64, 64, False, 4, 0), (1, 128, 128, False, 3, 0), (5, 256, 64, True, 4, 0),
         (67, 256, 32, False, 2, 0), (5, 384, 32, True, 3, 0), (67, 384, 128, False, 4, 0),
         (67, 384, 64, True, 4, 0))
IDS = ["r{}x{}g{}{}{}".format(r, n, g, "s" if s else "a", b) for r, n, g, s, b, _ in CASES]

# MEASURED: the largest relative difference of y and of scale between the host loops and the f64
# reference over CASES, on the CPU.  8x for seed-to-seed variation; the GPU adds none.
MEASURED = 1.17e-6   # y 1.161e-6, scale 1.162e-6 (case r67x384g64s4)
RTOL = 8 * MEASURED


@functools.lru_cache(maxsize=None)
def inputs(rows, rowlen, seed):
    """(w fp32, U fp32 upper, H f64): X = Z A with a random mixing A and n = 2 rowlen samples, H =
    X^T X / n damped by 1 %, U the upper Cholesky factor of H^-1 in f64, rounded to fp32 once."""
    rng = np.random.default_rng(1000 * rowlen + 10 * rows + seed)
    w = (rng.standard_normal((rows, rowlen)) * 0.05).astype(np.float32)
    X = rng.standard_normal((2 * rowlen, rowlen)) @ rng.standard_normal((rowlen, rowlen))
    H = X.T @ X / X.shape[0]
    H += 0.01 * np.mean(np.diag(H)) * np.eye(rowlen)
    U = np.linalg.cholesky(np.linalg.inv(H)).T   # Hinv = U^T U
    return w, np.ascontiguousarray(U.astype(np.float32)), H


@functools.lru_cache(maxsize=None)
def reference(rows, rowlen, G, symmetric, bits, seed):
    """The contract in float64: dict(y, scale, zp, codes)."""
    w, U32, _ = inputs(rows, rowlen, seed)
    U = U32.astype(np.float64)
    qmin, qmax = O.qrange(bits, symmetric)
    v = w.astype(np.float64)
    y, codes = np.empty_like(v), np.empty_like(v)
    scale, zp = np.empty((rows, rowlen // G)), np.empty((rows, rowlen // G))
    for i in range(rowlen):
        j = i // G
        if i % G == 0:
            for r in range(rows):
                g = v[r, i:i + G]
                scale[r, j], zp[r, j] = O.minmax_qparams(min(0.0, g.min()), max(0.0, g.max()), symmetric, bits)
        codes[:, i] = np.clip(np.rint(v[:, i] / scale[:, j] + zp[:, j]), qmin, qmax)
        y[:, i] = (codes[:, i] - zp[:, j]) * scale[:, j]
        e = (v[:, i] - y[:, i]) / U[i, i]
        v[:, i + 1:] -= e[:, None] * U[i, i + 1:]
    return dict(y=y, scale=scale, zp=zp, codes=codes)


def check_against_reference(got, case):
    """Codes (recovered as rint(y / scale + zp)) and zero points equal at every element, y and
    scale within RTOL.  ``got``: per_group_gptq's dict."""
    rows, rowlen, G = case[:3]
    ref = reference(*case)
    y = got["y"].detach().cpu().numpy().astype(np.float64).reshape(rows, rowlen)
    s = got["scale"].cpu().numpy()
    z = got["zp"].cpu().numpy()
    codes = np.rint(y / np.repeat(s, G, axis=1) + np.repeat(z, G, axis=1))
    assert np.array_equal(codes, ref["codes"]), f"{int((codes != ref['codes']).sum())} codes differ"
    assert np.array_equal(z, ref["zp"])
    nz = ref["y"] != 0
    dy = float(np.max(np.abs(y[nz] - ref["y"][nz]) / np.abs(ref["y"][nz]), initial=0.0))
    ds = float(np.max(np.abs(s - ref["scale"]) / ref["scale"]))
    print(f"gptq vs f64 reference: max rel diff y {dy:.3e}, scale {ds:.3e}")
    assert dy <= RTOL and ds <= RTOL, (dy, ds, RTOL)


def run(case, device="cpu", want_codes=False):
    import torch

    import vsiquantization_amd as V
    rows, rowlen, G, symmetric, bits, seed = case
    w, U, _ = inputs(rows, rowlen, seed)
    qmin, qmax = O.qrange(bits, symmetric)
    return V.per_group_gptq(torch.from_numpy(w).to(device), torch.from_numpy(U).to(device), group_size=G,
                            symmetric=symmetric, qmin=qmin, qmax=qmax, obs_bits=bits, want_codes=want_codes)


def proxy_loss(w, y, H):   # tr((W - Y) H (W - Y)^T) in f64
    d = np.asarray(w, np.float64) - np.asarray(y, np.float64)
    return float(np.sum((d @ H) * d))


# --------------------------------------------------------------------------- layer level
def make_layer(kind, device="cpu", group=32, wq="PerGroupUniformQuantizer", wobs="PerGroupMinMaxObserver",
               in_features=64, conv=None, fuse_bn=True):
    """(fused layer with 4-bit group-wise weights, correlated input batch) on ``device``."""
    import torch
    import torch.nn as nn
    from vsiquantization_amd.modules.fused import Conv, ConvBn, Linear
    torch.manual_seed(7)
    names = (wobs, wq, "MinMaxObserver", "UniformQuantizer")
    if kind == "linear":
        layer = Linear(nn.Linear(in_features, 24), *names, True, True, 4, 8)
        x = torch.randn(192, in_features) @ torch.randn(in_features, in_features)
    else:
        cv = conv or nn.Conv2d(8, 6, 2, padding=1)   # rows of 8 * 2 * 2 = 32 elements
        layer = (ConvBn(cv, nn.BatchNorm2d(cv.out_channels), *names, True, True, fuse_bn, 4, 8) if kind == "convbn"
                 else Conv(cv, *names, True, True, 4, 8))
        x = torch.einsum("nchw,cd->ndhw", torch.randn(24, 8, 6, 6), torch.randn(8, 8))
    mgr = layer.weight_quantizer
    mgr.quantizer.group_size = group
    mgr.observer.num_bits = 4
    mgr.is_learning_scale = False
    layer.quantize_out = False
    return layer.to(device).eval(), x.to(device)


def check_layer(kind, device):
    """GPTQ beats round-to-nearest on the layer's output; the eval forward's quantized weight is
    per_group_gptq's y bit for bit, twice.  One bit is not y's: the element function returns -0.0
    for a small negative weight of code 0 and +0.0 for that -0.0, hence y + 0.0."""
    import torch
    import vsiquantization_amd as V
    layer, x = make_layer(kind, device)
    q, obs = layer.weight_quantizer.quantizer, layer.weight_quantizer.observer
    w = layer.get_weight_bias()[0]
    y = V.per_group_gptq(w.detach(), V.gptq_factor(V.gptq_hessian(layer, x)), group_size=32, symmetric=True,
                         qmin=q.qmin, qmax=q.qmax, obs_bits=obs.num_bits, eps=obs.eps)["y"]
    rec = V.gptq_layer(layer, x)
    print(rec)
    assert rec["mse_gptq"] < rec["mse_nearest"]
    for _ in range(2):
        layer(x)
        assert torch.equal(layer.quantize_weights(w).view(torch.int32), (y + 0.0).view(torch.int32))


def check_model(device):
    """gptq_model: a refused layer (group_size 256) is listed under ``skipped``, the rest is done."""
    import pytest
    import torch.nn as nn
    import vsiquantization_amd as V
    l1, x = make_layer("linear", device)
    l2, _ = make_layer("linear", device, group=256, in_features=24)
    with pytest.warns(RuntimeWarning, match="group_size 256"):
        out = V.gptq_model(nn.Sequential(l1, l2), [x[:96], x[96:]])
    assert list(out["layers"]) == ["0"] and list(out["skipped"]) == ["1"]
