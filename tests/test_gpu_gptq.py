"""GPTQ on the GPU (csrc/k_gptq.hip) against the host loops, bit for bit, and the f64 reference."""
import pytest
import torch

from tests import gptq_common as C
import vsiquantization_amd as V
from oracle import fakequant_np as O
from tests.pg_common import same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_gpu_vs_host_bits(case):
    rows, rowlen, G = case[:3]
    host, dev = C.run(case), C.run(case, "cuda", want_codes=True)
    for k in ("y", "scale", "zp"):
        assert same_bits(dev[k].cpu(), host[k]), k
    y, s, z = (dev[k].cpu().double() for k in ("y", "scale", "zp"))
    codes = torch.round(y / s.repeat_interleave(G, 1) + z.repeat_interleave(G, 1))
    assert torch.equal(dev["codes"].cpu().double(), codes)


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_gpu_vs_reference(case):
    rows, rowlen, G, symmetric, bits, seed = case
    got = C.run(case, "cuda")
    C.check_against_reference(got, case)
    w, _, H = C.inputs(rows, rowlen, seed)
    qmin, qmax = O.qrange(bits, symmetric)
    rtn = V.per_group_observe_fq(torch.from_numpy(w).cuda(), group_size=G, symmetric=symmetric, qmin=qmin, qmax=qmax,
                                 obs_bits=bits)["y"]
    loss, loss_rtn = C.proxy_loss(w, got["y"].cpu().numpy(), H), C.proxy_loss(w, rtn.cpu().numpy(), H)
    print(f"proxy loss: gptq {loss:.6e}, nearest {loss_rtn:.6e}")
    assert loss < loss_rtn


@pytest.mark.parametrize("kind", ["linear", "conv", "model"])
def test_layer_gpu(kind):
    C.check_model("cuda") if kind == "model" else C.check_layer(kind, "cuda")
