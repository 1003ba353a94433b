"""GPTQ on CPU tensors: the host loops against the f64 reference, the layer level, the refusals."""
import pytest
import torch
import torch.nn as nn

from tests import gptq_common as C
import vsiquantization_amd as V


@pytest.mark.parametrize("case", C.CASES, ids=C.IDS)
def test_host_vs_reference(case):
    C.check_against_reference(C.run(case), case)


@pytest.mark.parametrize("kind", ["linear", "conv", "model"])
def test_layer_host(kind):
    C.check_model("cpu") if kind == "model" else C.check_layer(kind, "cpu")


def _nonleaf():
    layer, x = C.make_layer("linear")
    layer.get_weight_bias = lambda: (layer.linear_fuse.weight * 1.0, None)
    return layer, x


REFUSED = {
    "rotated": (lambda: C.make_layer("linear", wq="RotatedPerGroupQuantizer"), "RotatedPerGroupQuantizer"),
    "lsq": (lambda: C.make_layer("linear", wq="PerGroupLSQQuantizer"), "PerGroupLSQQuantizer"),
    "mse": (lambda: C.make_layer("linear", wobs="PerGroupMSEObserver"), "PerGroupMSEObserver"),
    "g256": (lambda: C.make_layer("linear", group=256), "Linear.*group_size 256"),
    "rowlen": (lambda: C.make_layer("linear", in_features=48), "Linear.*48 elements"),
    "grouped": (lambda: C.make_layer("conv", conv=nn.Conv2d(8, 6, 2, padding=1, groups=2)), "Conv.*groups=2"),
    "dilated": (lambda: C.make_layer("conv", conv=nn.Conv2d(8, 6, 2, padding=1, dilation=2)), "Conv.*dilation"),
    "bn": (lambda: C.make_layer("convbn", fuse_bn=False), "ConvBn.*unfolded BatchNorm"),
    "nonleaf": (_nonleaf, "Linear.*not a leaf"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_layer_refusals(name):
    make, match = REFUSED[name]
    layer, x = make()
    with pytest.raises(NotImplementedError, match=match):
        V.gptq_layer(layer, x)


def test_function_refusals():
    w, U = torch.zeros(2, 64), torch.eye(64)
    kw = dict(symmetric=True, qmin=-8, qmax=7)
    with pytest.raises(TypeError, match="float16"):
        V.per_group_gptq(w.half(), U, group_size=32, **kw)
    with pytest.raises(TypeError, match="float64"):
        V.per_group_gptq(w, U.double(), group_size=32, **kw)
    with pytest.raises(ValueError, match="rowlen = 64.*G = 128"):
        V.per_group_gptq(w, U, group_size=128, **kw)
    with pytest.raises(ValueError, match="group_size"):
        V.per_group_gptq(w, torch.eye(256), group_size=256, **kw)
    with pytest.raises(ValueError, match=r"U must be a \[64, 64\]"):
        V.per_group_gptq(w, torch.eye(32), group_size=32, **kw)
