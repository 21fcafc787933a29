"""BatchNorm1d + ReLU of SuperGlue's MLPs, forward and backward, host side: the project's restatement (tests/bngrad_ref.py: the closed
forms of DESIGN.md section 16 written out, no autograd) against the samples and per-channel sums the reference's own MLP and
KeypointEncoder wrote under torch.autograd (tests/golden/make_golden_bngrad.py), against autograd of the same written forward, against
finite differences, the ragged rules, the module's running statistics, and the Python surface of the entry points.  No GPU."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from tests import bngrad_ref as R
from tests import lingrad_ref as LR
from tests import util
from tests.golden.make_golden_bngrad import (CASES, KENC, MAX_REFUSED, RAGGED_COUNTS, RAGGED_FRAME, TENSORS, channel_sums, kenc_positions,
                                             kenc_sums, sample_positions)
from tests.golden.make_golden_lingrad import LAYER

FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(util.GOLDEN, "bngrad_*.npz")))


def frac64(got, ref):
    """the worst fraction of 1e-5 + 1e-5 |ref| used"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))))


def restated(name, dtype):
    """the restatement of one fixture's case; `ragged` as the NaN-padded batch of three, its results concatenated again"""
    g = util.golden(f"bngrad_{name}.npz")
    seed, (B, C, N), training = int(g["seed"]), (int(v) for v in g["shape"]), CASES[name][2]
    x, gamma, beta, dy = R.case(seed, B, C, N)
    rm, rv = R.running(seed, C) if not training else (np.zeros(C, np.float32), np.ones(C, np.float32))
    n = None
    if name == "ragged":
        x, dy, n = R.ragged_pad(x, RAGGED_COUNTS, RAGGED_FRAME), R.ragged_pad(dy, RAGGED_COUNTS, RAGGED_FRAME), RAGGED_COUNTS
    res = R.batch_reference(x, gamma, beta, dy, n, training, rm, rv, dtype=dtype)
    if name == "ragged":
        assert all(np.isfinite(a).all() for a in res.values()), "NaN padding leaked"
        res.update({t: R.ragged_cat(res[t], RAGGED_COUNTS) for t in ("y", "dx")})
    return g, res


def test_fixture_set():
    assert FIXTURES == sorted([f"bngrad_{n}.npz" for n in CASES] + ["bngrad_kenc.npz"])
    assert [CASES[n][1:] for n in ("c256", "c32", "b2", "eval")] == [((1, 256, 100), True), ((1, 32, 50), True), ((2, 64, 45), True), ((1, 128, 70), False)]
    assert CASES["ragged"][1:] == ((1, 64, 94), True) and RAGGED_COUNTS == (60, 33, 1) and RAGGED_FRAME == 64
    for name, (seed0, shape, training) in CASES.items():
        g = util.golden(f"bngrad_{name}.npz")
        assert os.path.getsize(os.path.join(util.GOLDEN, f"bngrad_{name}.npz")) < 75000
        assert tuple(int(v) for v in g["shape"]) == shape and int(g["seed"]) == seed0 + int(g["refused"])
        assert 0 <= int(g["refused"]) <= MAX_REFUSED, "at most three seeds refused by the kink rule"
        assert int(g["nbt"]) == (1 if training else 0)
        for t, n_sum in zip(TENSORS, (shape[1], shape[1], 1, 1)):
            assert np.isfinite(g[f"{t}_g"]).all() and np.isfinite(g[f"{t}_d32"]).all() and g[f"{t}_sum"].shape == (n_sum,) and len(g[f"{t}_g"]) <= 1000
    g = util.golden("bngrad_kenc.npz")
    assert os.path.getsize(os.path.join(util.GOLDEN, "bngrad_kenc.npz")) < 75000
    assert int(g["seed"]) == KENC[0] + int(g["refused"]) and 0 <= int(g["refused"]) <= MAX_REFUSED and KENC[1:] == (128, (32, 64, 128), 70)
    names = [str(n) for n in g["names"]]
    assert names[:3] == ["out", "dkpts", "dscores"] and names[3:] == [n for n, _ in R.KeypointEncoder(128, [32, 64, 128]).named_parameters()]
    assert len(names) == 17 and list(g["nbt"]) == [1, 1, 1]
    assert g["out_sum"].shape == (128,) and g["encoder.3.weight_sum"].shape == (64,) and g["dkpts_sum"].shape == (2,), "a sum per channel"
    assert all(np.isfinite(g[f"{n}_g"]).all() and np.isfinite(g[f"{n}_d32"]).all() and len(g[f"{n}_g"]) <= 400 for n in names)
    x = R.case(1, 1, 256, 100)[0]
    assert 1.0 < x.std() < 1.3 and np.abs(x).max() > 6, "heavy-tailed inputs of standard deviation about 1.13"


@pytest.mark.parametrize("name", list(CASES))
def test_no_kink_in_the_committed_seeds(name):
    """no element of the committed cases has |z64| < 1e-5: the ReLU mask is the same in fp32 and float64"""
    _, res = restated(name, torch.float64)
    assert not R.kink(res["z"], RAGGED_COUNTS if name == "ragged" else None).any()


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_float64(name):
    """samples and per-channel sums of y, dx, dgamma, dbeta, and the running statistics after the step, within 1e-5 + 1e-5 |ref| of the
    reference's float64 autograd"""
    g, res = restated(name, torch.float64)
    f = 0.0
    for t in TENSORS:
        pos = sample_positions(name, t, res[t].size)
        f = max(f, frac64(res[t].reshape(-1)[pos], g[f"{t}_g"]), frac64(channel_sums(t, res[t]), g[f"{t}_sum"]))
    f = max(f, frac64(res["running_mean"], g["running_mean"]), frac64(res["running_var"], g["running_var"]))
    print(f"{name}: the float64 restatement uses {f:.3g} of 1e-5 + 1e-5 |ref|")
    assert f <= 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_fp32(name):
    """the closed forms in fp32 at the default bar on the samples"""
    g, res = restated(name, torch.float32)
    fr = {}
    for t in TENSORS:
        pos = sample_positions(name, t, res[t].size)
        fr[t] = float(np.max(np.abs(res[t].reshape(-1)[pos] - g[f"{t}_g"]) / R.bar(g[f"{t}_g"], g[f"{t}_d32"])))
    print(f"{name}: the fp32 restatement uses " + ", ".join(f"{v:.3g} ({t})" for t, v in fr.items()) + " of the default bar")
    assert max(fr.values()) <= 1.0


def test_restated_keypoint_encoder_against_the_fixture():
    """the restated KeypointEncoder (tests/bngrad_ref.py) in float64 with the seeded parameters, train mode: output, dkpts, dscores and
    every parameter gradient within 1e-5 + 1e-5 |ref| of what the reference's module wrote (samples and sums), no kink element in any
    of its three BatchNorm outputs, and the buffers after the step"""
    g = util.golden("bngrad_kenc.npz")
    seed, (_, d, layers, N) = int(g["seed"]), KENC
    m = R.KeypointEncoder(d, list(layers)).train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.kenc_parameters(seed, m).items()}, strict=False)
    m = m.double()
    kpts, scores, dy = (torch.from_numpy(a).double() for a in R.kenc_case(seed, N, d))
    res = {}
    zs = R.bn_outputs(m, lambda: res.update(R.kenc_grads(m, m, kpts, scores, dy)))
    assert len(zs) == 3 and not any(R.kink(z.numpy()).any() for z in zs)
    f = 0.0
    for i, name in enumerate(str(n) for n in g["names"]):
        a = res[name].numpy()
        f = max(f, frac64(a.reshape(-1)[kenc_positions(i, a.size)], g[f"{name}_g"]), frac64(kenc_sums(name, a), g[f"{name}_sum"]))
    for i, bn in enumerate(mod for mod in m.encoder if isinstance(mod, torch.nn.BatchNorm1d)):
        f = max(f, frac64(bn.running_mean.numpy(), g[f"running_mean_{i}"]), frac64(bn.running_var.numpy(), g[f"running_var_{i}"]))
    print(f"kenc: the restated module in float64 uses {f:.3g} of 1e-5 + 1e-5 |ref|")
    assert f <= 1.0


def test_layer_fixture_seed_has_no_kink():
    """the committed lingrad_layer.npz seed: no element of the layer's hidden activation (the BatchNorm output of the restated module, in
    float64) lies within 1e-5 of 0, so the layer test of the GPU suite can use that fixture as it is"""
    seed, d, heads, N, M = LAYER
    m = LR.AttentionalPropagation(d, heads).train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in LR.layer_parameters(seed, m).items()}, strict=False)
    m = m.double()
    x, source, _ = (torch.from_numpy(a).double() for a in LR.layer_case(seed, d, N, M))
    zs = R.bn_outputs(m, lambda: m(x, source))
    assert len(zs) == 1 and zs[0].shape == (1, 2 * d, N) and not R.kink(zs[0].numpy()).any()
    print(f"layer: the smallest |z64| of the hidden activation is {float(zs[0].abs().min()):.3g}")


@pytest.mark.parametrize("shape,training", [((2, 5, 9), True), ((1, 33, 40), True), ((3, 2, 1), True), ((2, 7, 11), False)])
def test_closed_form_against_autograd(shape, training):
    """float64: the closed forms and torch.autograd of the same written forward agree to rounding, with the ReLU's own mask and with a
    mask handed in"""
    x, gamma, beta, dy = R.case(31 + shape[2], *shape)
    rm, rv = R.running(5, shape[1])
    rng = np.random.default_rng(shape[2])
    for mask in (None, rng.random(shape) < 0.5):
        res = R.batch_reference(x, gamma, beta, dy, None, training, rm, rv, mask=mask)
        ref = R.autograd(x, gamma, beta, dy, training, rm, rv, mask=mask)
        for t in TENSORS:
            if t == "y" and mask is not None:
                continue                                  # (with a mask handed in, y = z mask is not the ReLU's)
            assert np.max(np.abs(res[t] - ref[t])) <= 1e-12 * max(1.0, np.abs(ref[t]).max()), (t, mask is None)


@pytest.mark.parametrize("training", [True, False])
def test_restatement_against_finite_differences(training):
    """(B, C, N) = (2, 3, 5), float64, central differences of sum(y * dy) in every element of x, gamma and beta, z kept off 0"""
    x, gamma, beta, dy = (a.astype(np.float64) for a in R.case(12, 2, 3, 5))
    rm, rv = (a.astype(np.float64) for a in R.running(12, 3))
    h = 1e-6
    fwd = lambda *a: R.forward(*a, None, training, rm, rv)
    assert np.abs(fwd(x, gamma, beta)["z"]).min() > 1e-3, "z is kept off the kink"
    res = R.batch_reference(x, gamma, beta, dy, None, training, rm, rv)
    value = lambda *a: float((fwd(*a)["y"] * dy).sum())
    args = [x, gamma, beta]
    for arg, t in enumerate(("dx", "dgamma", "dbeta")):
        fd = np.zeros_like(args[arg])
        for idx in np.ndindex(*args[arg].shape):
            d = np.zeros_like(args[arg])
            d[idx] = h
            hi, lo = list(args), list(args)
            hi[arg], lo[arg] = args[arg] + d, args[arg] - d
            fd[idx] = (value(*hi) - value(*lo)) / (2 * h)
        assert np.max(np.abs(fd - res[t])) < 1e-6, (t, np.max(np.abs(fd - res[t])))


def test_ragged_rules_of_the_restatement():
    """NaN on the padding of x and dy must not leak: the valid region equals the concatenated columns as one pair, everything else is 0,
    a pair of count 0 changes nothing, M = 0 gives zeros and leaves the running statistics, M = 1 leaves running_var"""
    counts, N, C = [9, 5, 1, 0], 9, 6
    x, gamma, beta, dy = R.case(50, 1, C, sum(counts))
    rm, rv = R.running(50, C)
    xp, dyp = R.ragged_pad(x, counts, N), R.ragged_pad(dy, counts, N)
    for dtype in (torch.float64, torch.float32):
        res = R.batch_reference(xp, gamma, beta, dyp, counts, True, rm, rv, dtype=dtype)
        one = R.batch_reference(x, gamma, beta, dy, None, True, rm, rv, dtype=dtype)
        assert all(np.isfinite(a).all() for a in res.values())
        for b, cnt in enumerate(counts):
            assert not res["y"][b, :, cnt:].any() and not res["dx"][b, :, cnt:].any()
        tol = 1e-12 if dtype == torch.float64 else 1e-5
        for t in ("y", "dx"):
            assert np.allclose(R.ragged_cat(res[t], counts), one[t], rtol=tol, atol=tol), t
        for t in ("dgamma", "dbeta", "mean", "rstd", "running_mean", "running_var"):
            assert np.allclose(res[t], one[t], rtol=tol, atol=tol), t
        without = R.batch_reference(xp[:3], gamma, beta, dyp[:3], counts[:3], True, rm, rv, dtype=dtype)
        assert all(np.array_equal(res[t], without[t]) for t in ("dgamma", "dbeta", "mean", "rstd", "running_mean", "running_var"))
        assert np.array_equal(res["y"][:3], without["y"]) and np.array_equal(res["dx"][:3], without["dx"]), "the empty pair adds nothing"
    empty = R.batch_reference(xp, gamma, beta, dyp, [0, 0, 0, 0], True, rm, rv)
    assert not any(empty[t].any() for t in ("y", "dx", "dgamma", "dbeta", "mean", "rstd"))
    assert np.array_equal(empty["running_mean"], rm.astype(np.float64)) and np.array_equal(empty["running_var"], rv.astype(np.float64))
    single = R.batch_reference(xp, gamma, beta, dyp, [0, 1, 0, 0], True, rm, rv)
    assert np.array_equal(single["running_var"], rv.astype(np.float64)) and not np.array_equal(single["running_mean"], rm.astype(np.float64))
    assert np.allclose(single["mean"], xp[1, :, 0]) and np.allclose(single["rstd"], R.EPS ** -0.5) and not single["dx"].any()


@pytest.mark.parametrize("training", [True, False])
def test_running_statistics_against_the_module(training):
    """three steps of nn.BatchNorm1d on the CPU in float64 against the restatement fed its own running statistics: running_mean,
    running_var and the outputs agree to rounding; num_batches_tracked counts the training steps"""
    C = 7
    bn = torch.nn.BatchNorm1d(C).double().train(training)
    rm, rv = (a.astype(np.float64) for a in R.running(3, C))
    bn.load_state_dict({"running_mean": torch.from_numpy(rm), "running_var": torch.from_numpy(rv)}, strict=False)
    steps = 0
    for step in range(3):
        x, gamma, beta, _ = R.case(70 + step, 2, C, 13)
        bn.load_state_dict({"weight": torch.from_numpy(gamma).double(), "bias": torch.from_numpy(beta).double()}, strict=False)
        with torch.no_grad():
            y = torch.relu(bn(torch.from_numpy(x).double())).numpy()
        res = R.forward(x, gamma, beta, None, training, rm, rv, bn.eps, bn.momentum)
        rm, rv = res["running_mean"], res["running_var"]
        steps += 1 if training else 0
        assert np.allclose(res["y"], y, rtol=1e-12, atol=1e-12)
        assert np.allclose(rm, bn.running_mean.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(rv, bn.running_var.numpy(), rtol=1e-12, atol=1e-12)
    assert int(bn.num_batches_tracked) == steps


def test_entry_points_are_declared_and_bound():
    """the Python surface has the documented signatures; a CPU tensor is an ImxError (the exported tables: tests/test_train_library_host.py)"""
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine, ImxError
    sig = lambda f: list(inspect.signature(f).parameters)
    default = lambda f, p: inspect.signature(f).parameters[p].default
    assert sig(Engine.bn_relu_forward_train) == ["self", "x", "gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "n",
                                                 "training", "momentum", "eps"]
    assert (default(Engine.bn_relu_forward_train, "training"), default(Engine.bn_relu_forward_train, "momentum"),
            default(Engine.bn_relu_forward_train, "eps")) == (True, 0.1, 1e-5)
    assert sig(Engine.bn_relu_backward) == ["self", "x", "gamma", "beta", "mean", "rstd", "dy", "n", "training", "want"]
    assert default(Engine.bn_relu_backward, "want") == (True, True, True)
    assert issubclass(sgtrain_grad.bn_relu, torch.autograd.Function)
    assert sig(sgtrain_grad.bn_relu.forward)[:4] == ["ctx", "engine", "x", "gamma"]
    assert sig(sgtrain_grad.batchnorm_relu) == ["engine", "bn", "x", "n"]
    assert sig(sgtrain_grad.mlp) == ["engine", "seq", "x", "x1", "n"]
    assert sig(sgtrain_grad.keypoint_encoder) == ["engine", "kenc", "kpts", "scores", "n"]
    assert sig(sgtrain_grad.gnn_layer) == ["engine", "layer", "x", "source", "n", "ns"]
    assert sig(sgtrain_grad.attentional_propagation) == ["engine", "layer", "x", "source"], "the existing layer keeps its signature"
    bn = torch.nn.BatchNorm1d(4)
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        sgtrain_grad.batchnorm_relu(None, bn, torch.zeros(1, 4, 3))
    for bad in (torch.nn.BatchNorm1d(4, momentum=None), torch.nn.BatchNorm1d(4, affine=False), torch.nn.BatchNorm1d(4, track_running_stats=False)):
        with pytest.raises(ImxError, match="not supported"):
            sgtrain_grad.batchnorm_relu(None, bad, torch.zeros(1, 4, 3))
    with pytest.raises(ImxError, match="mlp: expected"):
        sgtrain_grad.mlp(None, torch.nn.Sequential(torch.nn.Conv1d(4, 4, 1), torch.nn.ReLU(), torch.nn.Conv1d(4, 4, 1)), torch.zeros(1, 4, 3))
