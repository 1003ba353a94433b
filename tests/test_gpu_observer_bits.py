"""The observer family's records, bit for bit (MI355X only).

Every per-tensor observer form -- K2 (grid-stride and one-shot), K2p, K2m, K2o (both forms),
K8, K9, K10, K1r, the two finalize kernels and the deferred fold -- promises records that are
fixed per n.  The parity tests compare the sums to 1e-6, which a reordered fold would pass;
this file compares every form's folded stats record (all VSIQ_ST_LEN float64 bit
patterns), its qparams record, and the sha256 of its raw partial records and of its
fake-quantized output, with tests/golden/observer_records.json.  The fixture was recorded
on an MI355X before the observer kernels' repeated tails were folded into shared helpers
(csrc/k_observe.cuh), so equality here is the proof that those helpers kept every
accumulation order.  No size here reaches the K2o forms chosen by CU count, so the fixture
does not depend on the device.

Inputs: test_gpu_dispatch.py's base tensor (torch.Generator().manual_seed(20), x 2.0); the
"planted" variant holds three NaNs, one +inf and one -inf.  Each shape runs with act None
and with SiLU under goldens.GOLDEN_SILU_REF, and planted with act None.

`python -m tests.test_gpu_observer_bits --write` records the fixture again.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from vsiquantization_amd import _hip as H
from vsiquantization_amd import fakequant as FQ
from tests import goldens as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "observer_records.json")
QMIN, QMAX = 0, 255
RUN0 = (-0.5, 0.25)          # the running min / max before the call (K2, K8, K9, K10, K1r, finalize)
NBASE = 13_107_200 + 8       # test_gpu_dispatch.py's base tensor
NKEEP = 4_193_284            # the longest prefix used here
# kObsU 8 groups per lane x 256 lanes: one workgroup up to 8192 elements; kArriveFlat 128 workgroups
N_ONE, N_FLAT, N_TWO_LEVEL = 8191, 20_003, 128 * 256 * 8 * 4 + 4 + 3
N_PART_U8 = 4_193_284 - 3    # PART_SIZES[8][0] of test_gpu_dispatch.py, tail layout
N_K2O = 20_483
VARIANTS = (("clean", None), ("clean", "silu"), ("planted", None))
_x = {}


def _inputs():
    if not _x:
        base = torch.randn(NBASE, generator=torch.Generator().manual_seed(20))[:NKEEP + 1] * 2.0
        planted = base.clone()
        for i, v in ((5, float("nan")), (777, float("inf")), (4099, float("nan")), (8190, float("-inf")),
                     (20_001, float("nan"))):
            planted[i] = v
        _x["clean"], _x["planted"] = base.to(DEV), planted.to(DEV)
    return _x


@pytest.fixture(scope="module", autouse=True)
def _setup():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    H.lib()
    H.set_silu_reference(*G.GOLDEN_SILU_REF)
    yield
    H.set_silu_reference()
    _x.clear()


class tuned:
    """Set tuning keys (TUNE_<NAME>=value), restore the defaults after."""
    defaults = {"OBS_KERNEL": 0, "LSQ_GROUPS": 0, "K2O_FORM": 0, "K2O_GROUPS": 0, "K2O_BLOCK": 0}

    def __init__(self, **knobs):
        self.knobs = knobs

    def __enter__(self):
        for k, v in self.knobs.items():
            H.set_tuning(getattr(H, "TUNE_" + k), v)

    def __exit__(self, *exc):
        for k in self.knobs:
            H.set_tuning(getattr(H, "TUNE_" + k), self.defaults[k])


def view(var, n, offset=0):
    """n elements of input `var`; tail lengths and a one-element offset leave the 16-byte path."""
    return _inputs()[var][offset:offset + n]


def bits(t):
    return [int(v) for v in t.detach().cpu().contiguous().view(torch.int64).flatten().tolist()]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def cdiv(a, b):
    return -(-a // b)


def run_state():
    return torch.tensor(RUN0, dtype=torch.float32, device=DEV)


def rec(st=None, qp=None, parts=None, y=None):
    r = {}
    if st is not None:
        r["stats"] = bits(st)
    if qp is not None:
        r["qp"] = bits(qp)
    if parts is not None:
        r["parts_sha256"] = sha(parts)
    if y is not None:
        r["y_sha256"] = sha(y)
    return r


# --------------------------------------------------------------------------- the forms
def k2(n, knobs):
    def run(var, act):
        with tuned(**knobs):
            qp, st = FQ.observe_tensor(view(var, n), symmetric=False, run_minmax=run_state(), act=act)
        return rec(st, qp)
    return run


def k2p(n):
    def run(var, act):
        parts = FQ.observe_parts(view(var, n), act=act)
        return rec(FQ.fold_parts(parts.view(1, -1))[0], parts=parts)
    return run


def k2m(var, act):
    """One batch of three tensors, the second off the 16-byte path; every tensor's records and fold."""
    xs = [view(var, 8192), view(var, N_FLAT), view(var, 40_000)]
    out = {}
    for i, parts in enumerate(FQ.observe_parts_multi(xs, None, act=act)):
        out[str(i)] = rec(FQ.fold_parts(parts.view(1, -1))[0], parts=parts)
    return out


def k2o(knobs):
    def run(var, act):
        with tuned(**knobs):
            y, parts = FQ.observe_parts_out(view(var, N_K2O), act)
        return rec(FQ.fold_parts(parts.view(1, -1))[0], parts=parts, y=y)
    return run


def fold_fq_records(n):   # fold_fq_part_grid(n) workgroups x 4 waves
    return 4 * min(32, max(1, cdiv(cdiv(cdiv(n, 4), 256), 4)))


def observe_fq(n, form):
    def run(var, act):
        x = view(var, n)
        y, qp, st, m, c = FQ.observe_fake_quant(x, symmetric=False, qmin=QMIN, qmax=QMAX, run_minmax=run_state(),
                                                act=act, want_mask=True, want_codes=True, parts=form)
        parts = None
        if form:   # K9 / K10: the K2p records in the workspace (K10 writes fields 0..5 only)
            ws = H.workspace(x.device, n).ws
            parts = ws[:fold_fq_records(n) * H.PART_LEN].view(-1, H.PART_LEN)[:, :H.PART_LEN if form is True else 6]
        r = rec(st, qp, parts, y)
        r["mask_sha256"], r["codes_sha256"] = sha(m), sha(c)
        return r
    return run


def gathered_records():
    """Three ranks' stats records built on the host: unequal n, rank 1 holds NaNs."""
    g = np.zeros((3, H.ST_LEN))
    for r, (mn, mx, nan, n) in enumerate(((-3.25, 2.5, 0.0, 1000.0), (-1.5, 7.75, 2.0, 37.0), (-0.125, 0.5, 0.0, 4099.0))):
        rng = np.random.default_rng(100 + r)
        g[r, [H.ST_MIN, H.ST_MAX, H.ST_NAN, H.ST_N]] = mn, mx, nan, n
        g[r, [H.ST_SUMABS, H.ST_SUM, H.ST_SUMSQ]] = rng.uniform(1.0, 1e4, 3) * (1.0, -0.37, 3.1)
    return g


def ranks(with_nan):
    def run(var, act):
        g = gathered_records()
        if not with_nan:
            g[1, H.ST_NAN] = 0.0
        gd = torch.from_numpy(g).to(DEV)
        n = 1027
        x = view(var, n)
        out = {}
        for name in ("finalize_ranks", "k1r"):
            qp = torch.empty(H.QP_LEN, dtype=torch.float64, device=DEV)
            st = torch.empty(H.ST_LEN, dtype=torch.float64, device=DEV)
            run_mm, y = run_state(), None
            if name == "k1r":
                y = torch.empty_like(x)
                rc = H.lib().vsiq_act_fq_fwd_ranks_f32(H.ptr(x), H.ptr(y), None, None, H.c_i64(n), H.act_code(act),
                                                       H.ptr(gd), 3, H.ptr(st), H.ptr(run_mm), H.ptr(qp), 0,
                                                       FQ.qden(False, 8, 1e-8), 1e-8, QMIN, QMAX,
                                                       H.stream_of(torch.device(DEV)))
            else:
                rc = H.lib().vsiq_observe_finalize_ranks(H.ptr(gd), 3, H.ptr(st), H.ptr(run_mm), H.ptr(qp), 0,
                                                         FQ.qden(False, 8, 1e-8), 1e-8, H.stream_of(torch.device(DEV)))
            H.check(rc, name)
            out[name] = rec(st, qp, y=y)
        return out
    return run


def part_slot(nrec, seed, written=True):
    """A deferred-observer slot of nrec records (stride nrec + 2 records), synthetic values."""
    p = np.zeros((nrec + 2, H.PART_LEN))
    if written:
        rng = np.random.default_rng(seed)
        p[:nrec, 0] = -rng.uniform(0.0, 4.0, nrec).astype(np.float32)
        p[:nrec, 1] = rng.uniform(0.0, 4.0, nrec).astype(np.float32)
        p[:nrec, 2] = rng.integers(0, 2, nrec)
        p[:nrec, 3:6] = rng.uniform(-1e3, 1e3, (nrec, 3))
        p[:nrec, 6], p[:nrec, 7] = 123_457.0, nrec
    return p.reshape(-1)


def fold_parts(rows):
    def run(var, act):
        st = FQ.fold_parts(torch.from_numpy(np.stack(rows())).to(DEV))
        return {str(i): rec(st[i]) for i in range(st.shape[0])}
    return run


ONCE = (("synthetic", None),)   # forms whose inputs are built on the host
FORMS = {
    "k2_one_workgroup": (k2(N_ONE, {}), VARIANTS),
    "k2_flat_arrivals": (k2(N_FLAT, {}), VARIANTS),
    "k2_two_level_arrivals": (k2(N_TWO_LEVEL, {}), VARIANTS),
    # the one-shot K2 takes K4's groups per lane; 2 and 16 are reached through the LSQ_GROUPS knob only
    "k2_oneshot_g2": (k2(N_FLAT, {"OBS_KERNEL": 1, "LSQ_GROUPS": 2}), VARIANTS),
    "k2_oneshot_g16": (k2(N_FLAT, {"OBS_KERNEL": 1, "LSQ_GROUPS": 16}), VARIANTS),
    "k2p_u2": (k2p(N_FLAT), VARIANTS),
    "k2p_u8": (k2p(N_PART_U8), VARIANTS),
    "k2m": (k2m, VARIANTS),
    "k2o_grid_stride": (k2o({"K2O_FORM": 1}), VARIANTS),
    "k2o_g2_b256": (k2o({"K2O_GROUPS": 2, "K2O_BLOCK": 256}), VARIANTS),
    "k2o_g2_b512": (k2o({"K2O_GROUPS": 2, "K2O_BLOCK": 512}), VARIANTS),
    "k2o_g2_b1024": (k2o({"K2O_GROUPS": 2, "K2O_BLOCK": 1024}), VARIANTS),
    "k2o_g16_b256": (k2o({"K2O_GROUPS": 16, "K2O_BLOCK": 256}), VARIANTS),
    "k8_u2": (observe_fq(8191, False), VARIANTS),
    "k8_u16": (observe_fq(8197, False), VARIANTS),
    "k9": (observe_fq(N_FLAT, True), VARIANTS),
    "k10_1step": (observe_fq(131_071, "k10"), VARIANTS),
    "k10_2steps": (observe_fq(131_075, "k10"), VARIANTS),
    "ranks_world3": (ranks(True), (("clean", None), ("clean", "silu"))),
    "ranks_world3_no_nan": (ranks(False), (("clean", None),)),
    "fold_parts_3_records": (fold_parts(lambda: [part_slot(3, 1)]), ONCE),
    "fold_parts_2051_records": (fold_parts(lambda: [part_slot(8 * 256 + 3, 2)]), ONCE),
    "fold_parts_unwritten_slot": (fold_parts(lambda: [part_slot(5, 3), part_slot(5, 4, written=False),
                                                      part_slot(5, 5)]), ONCE),
}
CASES = [(form, var, act) for form, (_, variants) in FORMS.items() for var, act in variants]


def case_key(form, var, act):
    return f"{form}/{var}/{act or 'none'}"


def compute(form, var, act):
    got = FORMS[form][0](var, act)
    torch.cuda.synchronize()
    return got


def _golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("form,var,act", CASES, ids=[case_key(*c) for c in CASES])
def test_observer_bits(form, var, act):
    want = _golden()[case_key(form, var, act)]
    got = compute(form, var, act)
    print(case_key(form, var, act), json.dumps(got))
    assert got == want


def test_fixture_has_no_other_cases():
    assert sorted(_golden()) == sorted(case_key(*c) for c in CASES)


if __name__ == "__main__":
    assert "--write" in sys.argv, "usage: python -m tests.test_gpu_observer_bits --write [path]"
    H.lib()
    H.set_silu_reference(*G.GOLDEN_SILU_REF)
    path = sys.argv[sys.argv.index("--write") + 1] if len(sys.argv) > sys.argv.index("--write") + 1 else FIXTURE
    with open(path, "w") as f:   # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(case_key(*c))}: {json.dumps(compute(*c), sort_keys=True)}"
                                   for c in sorted(CASES, key=lambda c: case_key(*c))) + "\n}\n")
    print("wrote", path, os.path.getsize(path), "bytes")
