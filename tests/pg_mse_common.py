"""Shared by the PerGroupMSEObserver tests: tests/pc_mse_common.py's oracle with a group as its
"row"; seeds by its decidability rule; a case's tensor and oracle are computed once.  No GPU."""
import functools

import torch

from tests.mse_common import make_input
from tests.pc_mse_common import (FAMILIES, ONGRID_RATIOS, OracleState, all_decidable,  # noqa: F401
                                 check_against_oracle, grid_of, mse_ratios, oracle_rows, same_bits)

GROUPS = (32, 64, 128, 256)
GRIDS = ((True, 4), (False, 2), (False, 4))   # (symmetric, bits): 2 to 4 bits exercise the search
MIXED = FAMILIES + FAMILIES[::-1]


def oracle_groups(x, G, ratios, symmetric, bits):
    """oracle_rows of every group of the CPU tensor x [rows, rowlen], in [rows, ngr] order."""
    rows, rowlen = x.shape
    F, nf = (rowlen // G) * G, rowlen // G
    full = oracle_rows(x[:, :F].reshape(-1, G), ratios, symmetric, bits) if F else []
    tail = oracle_rows(x[:, F:], ratios, symmetric, bits) if F < rowlen else []
    return [g for r in range(rows) for g in full[r * nf:(r + 1) * nf] + tail[r:r + 1]]


@functools.lru_cache(maxsize=None)
def case(families, rowlen, G, ratios, symmetric, bits, start=1):
    """(seed, x, oracle groups) at the first seed >= start at which every group is decidable
    (pick_seed's rule, on groups).  Row r of x [len(families), rowlen] is drawn from families[r];
    families == "mixed": MIXED as adjacent groups, 2 rows of 8 groups and a half-length ninth."""
    for seed in range(start, start + 40):
        if families == "mixed":
            body = torch.stack([make_input(f, G, seed + 7 * c) for c, f in enumerate(MIXED)]).reshape(2, 8 * G)
            tail = torch.stack([make_input("heavy", G // 2, seed + 3), make_input("gauss", G // 2, seed + 5)])
            x = torch.cat([body, tail], dim=1).contiguous()
        else:
            x = torch.stack([make_input(f, rowlen, seed + 7 * r) for r, f in enumerate(families)]).contiguous()
        groups = oracle_groups(x, G, ratios, symmetric, bits)
        if all_decidable(groups):
            return seed, x, groups
    raise AssertionError(f"no decidable seed for {families} x {rowlen} g{G}")


def run(x, G, symmetric, bits, ratios=mse_ratios(), want_errors=True, **kw):
    from vsiquantization_amd.fakequant import per_group_observe_mse
    qmin, qmax = grid_of(bits, symmetric)
    return per_group_observe_mse(x, group_size=G, symmetric=symmetric, qmin=qmin, qmax=qmax, num_bits=bits,
                                 ratios=ratios, want_errors=want_errors, **kw)


def flat(r):
    """A per_group_observe_mse dict with its [rows, ngr, ...] outputs as the oracle's [groups, ...]."""
    n = r["pick"].numel()
    return dict(err=r["err"].reshape(n, -1), pick=r["pick"].reshape(n), clip=r["clip"].reshape(n, 2),
                **{k: r[k].reshape(n) for k in ("run_min", "run_max", "scale", "zp")})


def same_but_errors(a, b, more=()):
    """Pick, clip, state and qparams of two result dicts (and the outputs named in ``more``) bit for bit."""
    return all(same_bits(a[k], b[k]) for k in ("pick", "clip", "scale", "zp", "run_min", "run_max") + tuple(more))
