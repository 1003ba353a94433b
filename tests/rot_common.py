"""Shared by test_rot_cpu.py and test_gpu_rot.py: hadamard_G (include/vsiq.h) restated in numpy as the stage loop
on fp32 arrays, the Sylvester matrix, the inputs, and the three-launch composition every fused call has to equal."""
import numpy as np
import torch

from vsiquantization_amd.fakequant import (hadamard_transform, per_group_fake_quant, per_group_observe_fq,
                                           pg_ste_backward)

GROUPS = (32, 64, 128, 256)


# per G: one group (most of the wave is padding), a full chunk, a partial second chunk, several chunks
CASES = tuple((r, n, G) for G in GROUPS for r, n in ((3, G), (2, 256), (3, 256 + G), (2, 1024)))


def c_of(G):
    return np.float32(1.0 / np.sqrt(np.float64(G)))


def sylvester(G):
    i, pop = np.arange(G), np.array([bin(v).count("1") for v in range(G)])
    return np.where(pop[i[:, None] & i[None, :]] % 2 == 0, 1.0, -1.0)


def hadamard_np(x, G):
    """The definition: for h = 1, 2, ..., G/2 every pair (v[i], v[i + h]) with bit h of i clear becomes
    (a + b, a - b) in fp32, then one multiply by c_G; a NaN result is the canonical quiet NaN."""
    a = np.ascontiguousarray(x, np.float32).reshape(-1, G).copy()
    i, h = np.arange(G), 1
    while h < G:
        lo = i[(i & h) == 0]
        p, q = a[:, lo].copy(), a[:, lo + h].copy()
        a[:, lo], a[:, lo + h] = p + q, p - q
        h *= 2
    a = a * c_of(G)
    a[np.isnan(a)] = np.float32("nan")
    return a.reshape(np.shape(x))


def inputs(rows, rowlen, seed):
    """Gaussians times a random power of two in 2^-20 .. 2^20 per element: the order of additions shows."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, rowlen, generator=g) * torch.exp2(torch.randint(-20, 21, (rows, rowlen), generator=g).float())


def composed(x, G, symmetric, qmin, qmax, run_min, run_max):
    """hadamard -> per_group_observe_fq -> hadamard on x's device, the state updated in place."""
    r = per_group_observe_fq(hadamard_transform(x, G), group_size=G, symmetric=symmetric, qmin=qmin, qmax=qmax,
                             run_min=run_min, run_max=run_max, want_mask=True, want_codes=x.is_cuda)
    r["yr"], r["y"] = r["y"], hadamard_transform(r["y"], G)
    return r


def composed_backward(g, mask, scale, G):
    return hadamard_transform(pg_ste_backward(hadamard_transform(g, G), mask, scale, G), G)


def composed_fixed(x, G, scale, zp, qmin, qmax, zp_round):
    q, mask, codes = per_group_fake_quant(hadamard_transform(x, G), scale, zp, qmin, qmax, group_size=G,
                                          zp_round=zp_round, want_mask=True, want_codes=x.is_cuda)
    return dict(y=hadamard_transform(q, G), yr=q, mask=mask, codes=codes)
