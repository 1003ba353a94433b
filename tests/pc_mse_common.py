"""Shared by tests/test_pc_mse_cpu.py and tests/test_gpu_pc_mse.py: PerChannelMSEObserver's
oracle -- tests/mse_common.py's oracle_search and OracleObserver applied to every row on its
own, with the row's numpy fp32 min / max / NaN flag -- the kernel's form thresholds read from
the source, the row families and the comparison of one call's result with the oracle.
Nothing here touches a GPU; seeds are chosen with the oracle alone."""
import functools
import os
import re

import numpy as np
import torch

from tests.mse_common import (FAMILIES, ONGRID_RATIOS, OracleObserver, decidable, errors_close, grid_of, make_input,
                              margin, oracle_search, same_bits)
from vsiquantization_amd.fakequant import mse_ratios

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vsiquantization_amd", "csrc")


@functools.lru_cache(maxsize=None)
def forms():
    """The kernel's seams, read from csrc/k_pc_mse.hip and vsiq_common.cuh: rows per workgroup
    of the wave form, and the largest row of the short wave step, the wave form and the
    register-resident workgroup form (elements)."""
    common = open(os.path.join(CSRC, "vsiq_common.cuh")).read()
    src = open(os.path.join(CSRC, "k_pc_mse.hip")).read()

    def const(text, name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))

    block, wave = const(common, "kBlock"), const(common, "kWave")
    u, wc, bc = const(src, "kPcMseU"), const(src, "kPcMseWaveChunks"), const(src, "kPcMseBlockChunks")
    assert "constexpr int64_t kPcMseWaveShort = 4 * kWave;" in src
    assert "constexpr int64_t kPcMseWaveMax = 4 * kWave * kPcMseU * kPcMseWaveChunks;" in src
    assert "constexpr int64_t kPcMseBlockMax = 4 * kBlock * kPcMseU * kPcMseBlockChunks;" in src
    assert "if (a.rowlen <= kPcMseWaveMax) {" in src and "if (a.rowlen <= kPcMseBlockMax)" in src
    return dict(rows_per_wg=block // wave, wave_short=4 * wave, wave_max=4 * wave * u * wc,
                block_max=4 * block * u * bc)


def row_minmax(v):
    """(mn, mx, has_nan) of one fp32 row as K3 reduces it: NaN-ignoring min / max, a NaN flag."""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    nan = np.isnan(v)
    ok = v[~nan]
    if ok.size == 0:
        return np.float32(np.inf), np.float32(-np.inf), True
    return ok.min(), ok.max(), bool(nan.any())


def make_rows(families, rowlen, seed):
    """fp32 CPU [len(families), rowlen]: row c of family families[c], its own seed."""
    return torch.stack([make_input(f, rowlen, seed + 7 * c) for c, f in enumerate(families)]).contiguous()


def oracle_rows(x, ratios, symmetric, bits):
    """[(lo, hi, E, pick, has_nan)] of one call on the CPU tensor x [C, ...], row by row."""
    v = x.reshape(x.shape[0], -1).numpy()
    out = []
    for c in range(v.shape[0]):
        mn, mx, has_nan = row_minmax(v[c])
        lo, hi, E, k = oracle_search(v[c], mn, mx, has_nan, ratios, symmetric, bits)
        out.append((lo, hi, E, k, has_nan))
    return out


def all_decidable(rows):
    return all(decidable(E) for _, _, E, _, _ in rows)


def pick_seed(families, rowlen, ratios, symmetric, bits, start=1, tries=40):
    """The first seed >= start whose rows are all decidable (a clear margin or an exact tie
    between the two smallest errors): the precondition of bit-equal picks, from the oracle
    alone.  Returns (seed, x, oracle rows)."""
    for seed in range(start, start + tries):
        x = make_rows(families, rowlen, seed)
        rows = oracle_rows(x, ratios, symmetric, bits)
        if all_decidable(rows):
            return seed, x, rows
    raise AssertionError(f"no decidable seed for {families} x {rowlen}")


class OracleState:
    """One OracleObserver per row: the running state and f64 qparams the call must return."""

    def __init__(self, rows, symmetric, bits):
        self.obs = [OracleObserver(symmetric, bits) for _ in range(rows)]

    def update(self, rows):
        for o, (lo, hi, _, _, has_nan) in zip(self.obs, rows):
            o.update(lo, hi, has_nan)

    def run_min(self):
        return np.array([o.mn for o in self.obs], dtype=np.float32)

    def run_max(self):
        return np.array([o.mx for o in self.obs], dtype=np.float32)

    def scale(self):
        with np.errstate(all="ignore"):
            return np.array([o.qparams()[0] for o in self.obs], dtype=np.float64)

    def zp(self):
        with np.errstate(all="ignore"):
            return np.array([o.qparams()[1] for o in self.obs], dtype=np.float64)


def check_against_oracle(r, rows, state, tag):
    """One call's result dict ``r`` against the oracle rows and the oracle state after the
    update: every E within REL, pick / clip / running state / qparams bit for bit.  The
    precondition (every row decidable) is asserted first, for every row."""
    err, pick, clip = r["err"].cpu(), r["pick"].cpu(), r["clip"].cpu()
    for c, (lo, hi, E, k, _) in enumerate(rows):
        t = (tag, c, margin(E))
        assert decidable(E), t
        assert errors_close(err[c], E), t
        assert int(pick[c]) == k, t
        assert same_bits(clip[c], np.array([lo, hi], dtype=np.float64)), t
    assert same_bits(r["run_min"], state.run_min()), tag
    assert same_bits(r["run_max"], state.run_max()), tag
    assert same_bits(r["scale"], state.scale()), tag
    assert same_bits(r["zp"], state.zp()), tag


def same_result(a, b, keys=("err", "pick", "clip", "scale", "zp", "run_min", "run_max")):
    return all(same_bits(a[k], b[k]) for k in keys)


__all__ = ["FAMILIES", "ONGRID_RATIOS", "OracleState", "all_decidable", "check_against_oracle", "forms", "grid_of",
           "make_rows", "mse_ratios", "oracle_rows", "pick_seed", "row_minmax", "same_bits", "same_result"]
