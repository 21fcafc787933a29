"""The restatement behind the BatchNorm2d tests (tests/bn2d_ref.py, the NCHW view of tests/bngrad_ref.py) held to the fixtures the
reference's own double_conv wrote under torch.autograd (tests/golden/make_golden_bn2d.py) at 1e-9 + 1e-9 |ref| in float64, to
torch.autograd of F.batch_norm with and without F.relu, and to central differences; the restated head against its fixture; and the
Python signatures of the new entry points.  No GPU."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn2d_ref as R2
from tests import bngrad_ref as R
from tests import util
from tests.golden.make_golden_bn2d import CASES, TENSORS, channel_sums, head_positions, sample_positions


def tight(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1e-9 + 1e-9 * np.abs(ref))))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_against_the_fixtures(name):
    g = util.golden(f"bn2d_{name}.npz")
    _, shape, training, relu = CASES[name]
    seed = int(g["seed"])
    assert tuple(int(v) for v in g["shape"]) == shape and bool(g["relu"]) == relu and bool(g["training"]) == training
    assert 0 <= int(g["refused"]) <= 3
    x, gamma, beta, dy = R2.case(seed, *shape)
    C = shape[1]
    rm, rv = R.running(seed, C) if not training else (np.zeros(C, np.float32), np.ones(C, np.float32))
    ref = R2.batch_reference(x, gamma, beta, dy, relu, training, rm, rv)
    if relu:
        assert not R2.kink(ref["z"]).any(), "the selected seed has no element at the kink"
    worst = {}
    for t in TENSORS:
        pos = sample_positions(name, t, ref[t].size)
        worst[t] = max(tight(ref[t].reshape(-1)[pos], g[f"{t}_g"]), tight(channel_sums(t, ref[t]), g[f"{t}_sum"]))
    worst["running"] = max(tight(ref["running_mean"], g["running_mean"]), tight(ref["running_var"], g["running_var"]))
    print(f"{name}: of 1e-9 + 1e-9 |ref| -- " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0
    assert int(g["nbt"]) == (1 if training else 0)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_restatement_against_autograd(relu, training):
    B, C, H, W = 2, 7, 5, 6
    x, gamma, beta, dy = R2.case(3, B, C, H, W)
    rm, rv = R.running(3, C)
    ref = R2.batch_reference(x, gamma, beta, dy, relu, training, rm, rv)
    leaves = [torch.from_numpy(a).double().requires_grad_(True) for a in (x, gamma, beta)]
    z = F.batch_norm(leaves[0], None if training else torch.from_numpy(rm).double(), None if training else torch.from_numpy(rv).double(),
                     leaves[1], leaves[2], training, 0.0, R.EPS)
    y = F.relu(z) if relu else z
    grads = torch.autograd.grad(y, leaves, torch.from_numpy(dy).double())
    got = {"y": y.detach().numpy(), **{k: v.numpy() for k, v in zip(("dx", "dgamma", "dbeta"), grads)}}
    assert max(tight(ref[k], got[k]) for k in got) <= 1.0


@pytest.mark.parametrize("relu", [True, False])
def test_central_differences(relu):
    """(2, 3, 2, 3) in float64: d sum(y dy) / d (x, gamma, beta) by central differences of the restated forward, step 1e-6"""
    B, C, H, W = 2, 3, 2, 3
    x, gamma, beta, dy = (a.astype(np.float64) for a in R2.case(5, B, C, H, W))
    ref = R2.batch_reference(x, gamma, beta, dy, relu)
    assert not relu or np.abs(ref["z"]).min() > 1e-3, "no element near the kink"
    loss = lambda xx, gg, bb: float((R2.batch_reference(xx, gg, bb, dy, relu)["y"] * dy).sum())
    h = 1e-6
    for i, (name, a) in enumerate((("dx", x), ("dgamma", gamma), ("dbeta", beta))):
        num = np.zeros_like(a)
        for idx in np.ndindex(*a.shape):
            args = [x.copy(), gamma.copy(), beta.copy()]
            args[i][idx] += h
            up = loss(*args)
            args[i][idx] -= 2 * h
            num[idx] = (up - loss(*args)) / (2 * h)
        assert np.max(np.abs(num - ref[name])) <= 1e-6 * (1 + np.abs(ref[name]).max()), name


def test_head_against_its_fixture():
    """the restated head reproduces its own fixture (the generator ran the same class): output, dx, 8 parameter gradients, buffers, eval"""
    g = util.golden("bn2d_head.npz")
    seed = int(g["seed"])
    assert len(g["refused"]) <= 3
    x, dy = (torch.from_numpy(a).double() for a in R2.head_case(seed))
    m = R2.load_head(seed, torch.float64).train()
    res = R2.head_grads(m, m, x, dy)
    names = [str(n) for n in g["names"]]
    assert len(names) == 10 and set(names) == set(res)
    for i, name in enumerate(names):
        a = res[name].numpy()
        assert tight(a.reshape(-1)[head_positions(i, a.size)], g[f"{name}_g"]) <= 1.0 and tight(a.sum(keepdims=True).reshape(1), g[f"{name}_sum"]) <= 1.0
    for i, (n, b) in enumerate(R2.head_buffers(m).items()):
        assert str(g["buffer_names"][i]) == n and tight(b, g[f"buffer_{i}"]) <= 1.0


def test_python_signatures():
    from image_matching_amd import sptrain_net
    from image_matching_amd.engine import Engine
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(Engine.bn2d_forward_train) == ["self", "x", "gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "relu",
                                                "training", "momentum", "eps"]
    assert names(Engine.bn2d_backward) == ["self", "x", "gamma", "beta", "mean", "rstd", "dy", "relu", "training", "want"]
    d = {k: v.default for k, v in inspect.signature(Engine.bn2d_forward_train).parameters.items()}
    assert (d["relu"], d["training"], d["momentum"], d["eps"]) == (True, True, 0.1, 1e-5)
    assert inspect.signature(Engine.bn2d_backward).parameters["want"].default == (True, True, True)
    assert names(sptrain_net.batchnorm2d) == ["engine", "bn", "x", "relu"] and inspect.signature(sptrain_net.batchnorm2d).parameters["relu"].default is False
    for f, first in ((sptrain_net.conv_bn_relu_form, ["engine", "conv", "bn", "x"]), (sptrain_net.double_conv_form, ["engine", "block", "x"]),
                     (sptrain_net.down_form, ["engine", "block", "x"])):
        assert names(f) == first + ["form"] and inspect.signature(f).parameters["form"].default == "auto", f.__name__
    # the three functions without a form keep the signatures they had: they are the *_form functions at "auto"
    assert names(sptrain_net.conv_bn_relu) == ["engine", "conv", "bn", "x"] and names(sptrain_net.double_conv) == names(sptrain_net.down) == ["engine", "block", "x"]
    assert names(sptrain_net.head) == ["engine", "conv_a", "bn_a", "conv_b", "bn_b", "x"]
    assert issubclass(sptrain_net.bn2d, torch.autograd.Function)
    # the rule of "auto": the shape alone, and never "pixels" below B H W = 4096 (every block the earlier tests run keeps its path)
    assert not any(sptrain_net.pixels_form(B, C, HW) for B, C, HW in ((2, 16, 120), (2, 32, 120), (2, 16, 480), (1, 1024, 4095), (4095, 1, 1)))
    assert sptrain_net.pixels_form(16, 64, 240 * 320)
