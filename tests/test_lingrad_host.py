"""The 1x1 convolutions of SuperGlue's GNN, forward and backward, host side: the project's restatement (tests/lingrad_ref.py: the closed
forms of DESIGN.md section 15 written out, no autograd) against the samples and per-channel sums the reference's own MLP wrote under
torch.autograd (tests/golden/make_golden_lingrad.py), against autograd of the same written forward, against finite differences, the
ragged rules, and the Python surface of the entry points.  No GPU."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from tests import lingrad_ref as R
from tests import util
from tests.golden.make_golden_lingrad import CASES, LAYER, RAGGED_FRAME, TENSORS, channel_sums, layer_positions, sample_positions

FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(util.GOLDEN, "lingrad_*.npz")))
ITEMS = [(name, k) for name in CASES for k in range(len(CASES[name]))]


def frac64(got, ref):
    """the worst fraction of 1e-5 + 1e-5 |ref| used"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))))


def item(g, k):
    return {key[:-len(f"_{k}")]: v for key, v in g.items() if key.endswith(f"_{k}")}


def restated(name, k, dtype):
    it = item(util.golden(f"lingrad_{name}.npz"), k)
    seed, (Cout, C0, C1, N) = int(it["seed"]), (int(x) for x in it["shape"])
    return it, R.batch_reference(*R.case(seed, 1, Cout, C0, C1, N, wseed=CASES[name][0][0]), dtype=dtype)


def test_fixture_set():
    assert FIXTURES == sorted([f"lingrad_{n}.npz" for n in CASES] + ["lingrad_layer.npz"])
    assert [CASES[n][0][1:] for n in ("proj", "mlp0", "kenc0", "d64")] == [(128, 128, 0, 70), (256, 128, 128, 100), (32, 3, 0, 50), (64, 128, 0, 45)]
    assert [c[1:] for c in CASES["ragged"]] == [(128, 64, 64, N) for N in (60, 33, 1)] and RAGGED_FRAME == 64
    for name, items in CASES.items():
        path = os.path.join(util.GOLDEN, f"lingrad_{name}.npz")
        g = util.golden(f"lingrad_{name}.npz")
        assert os.path.getsize(path) < 75000 and int(g["n_items"]) == len(items)
        for k, (seed, Cout, C0, C1, N) in enumerate(items):
            it = item(g, k)
            assert int(it["seed"]) == seed and tuple(int(x) for x in it["shape"]) == (Cout, C0, C1, N)
            for t, n_sum in zip(TENSORS, (Cout, C0 + C1, Cout, 1)):
                assert np.isfinite(it[f"{t}_g"]).all() and np.isfinite(it[f"{t}_d32"]).all() and it[f"{t}_sum"].shape == (n_sum,)
    g = util.golden("lingrad_layer.npz")
    assert os.path.getsize(os.path.join(util.GOLDEN, "lingrad_layer.npz")) < 75000
    assert (int(g["seed"]),) + tuple(int(x) for x in g["shape"]) == LAYER == (8, 128, 4, 70, 100)
    names = [str(n) for n in g["names"]]
    assert names[:3] == ["out", "dx", "dsource"] and names[3:] == [n for n, _ in R.AttentionalPropagation(128, 4).named_parameters()]
    assert all(np.isfinite(g[f"{n}_g"]).all() and np.isfinite(g[f"{n}_d32"]).all() and len(g[f"{n}_g"]) <= 200 for n in names)
    x0 = R.case(1, 1, 128, 128, 0, 70)[0]
    assert 1.0 < x0.std() < 1.3 and np.abs(x0).max() > 6, "heavy-tailed inputs of standard deviation about 1.13"


@pytest.mark.parametrize("name,k", ITEMS)
def test_restatement_float64(name, k):
    """samples and per-channel sums of y, dx, dw, db within 1e-5 + 1e-5 |ref| of the reference's float64 autograd"""
    it, res = restated(name, k, torch.float64)
    f = 0.0
    for t in TENSORS:
        pos = sample_positions(CASES[name][0][0], t, res[t].size, len(CASES[name]))
        f = max(f, frac64(res[t].reshape(-1)[pos], it[f"{t}_g"]), frac64(channel_sums(t, res[t]), it[f"{t}_sum"]))
    print(f"{name}[{k}]: the float64 restatement uses {f:.3g} of 1e-5 + 1e-5 |ref|")
    assert f <= 1.0


@pytest.mark.parametrize("name,k", ITEMS)
def test_restatement_fp32(name, k):
    """the closed forms in fp32 at the default bar on the samples"""
    it, res = restated(name, k, torch.float32)
    fr = {}
    for t in TENSORS:
        pos = sample_positions(CASES[name][0][0], t, res[t].size, len(CASES[name]))
        fr[t] = float(np.max(np.abs(res[t].reshape(-1)[pos] - it[f"{t}_g"]) / R.bar(it[f"{t}_g"], it[f"{t}_d32"])))
    print(f"{name}[{k}]: the fp32 restatement uses " + ", ".join(f"{v:.3g} ({t})" for t, v in fr.items()) + " of the default bar")
    assert max(fr.values()) <= 1.0


def test_restated_layer_against_the_fixture():
    """the restated AttentionalPropagation (tests/lingrad_ref.py) in float64 with the seeded parameters, train mode: output, dx, dsource
    and every parameter gradient within 1e-5 + 1e-5 |ref| of what the reference's module wrote (samples and sums)"""
    g = util.golden("lingrad_layer.npz")
    seed, d, heads, N, M = LAYER
    m = R.AttentionalPropagation(d, heads).train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.layer_parameters(seed, m).items()}, strict=False)
    m = m.double()
    res = R.layer_grads(m, m, *(torch.from_numpy(a).double() for a in R.layer_case(seed, d, N, M)))
    f = 0.0
    for i, name in enumerate(str(n) for n in g["names"]):
        a = res[name].numpy()
        f = max(f, frac64(a.reshape(-1)[layer_positions(seed, i, a.size)], g[f"{name}_g"]), frac64(a.sum(), g[f"{name}_sum"]))
    print(f"layer: the restated module in float64 uses {f:.3g} of 1e-5 + 1e-5 |ref|")
    assert f <= 1.0


@pytest.mark.parametrize("shape", [(2, 5, 4, 3, 9), (1, 33, 7, 0, 40), (2, 3, 1, 6, 1)])
def test_closed_form_against_autograd(shape):
    """float64: the closed forms and torch.autograd of the same written forward agree to rounding"""
    inputs = R.case(31 + shape[4], *shape)
    res, ref = R.batch_reference(*inputs), R.autograd(*inputs)
    for t in TENSORS:
        assert np.max(np.abs(res[t] - ref[t])) <= 1e-12 * max(1.0, np.abs(ref[t]).max()), t


def test_restatement_against_finite_differences():
    """(B, Cout, C0, C1, N) = (1, 3, 2, 1, 4), float64, central differences of sum(y * dy) in every element of x0, x1, w and bias"""
    x0, x1, w, bias, dy = (a.astype(np.float64) for a in R.case(11, 1, 3, 2, 1, 4))
    dx, dw, db = R.backward(x0, x1, w, dy)
    value = lambda *a: float((R.forward(*a) * dy).sum())
    h = 1e-6
    args = [x0, x1, w, bias]
    for arg, g in ((0, dx[:, :2]), (1, dx[:, 2:]), (2, dw), (3, db)):
        fd = np.zeros_like(args[arg])
        for idx in np.ndindex(*args[arg].shape):
            d = np.zeros_like(args[arg])
            d[idx] = h
            hi, lo = list(args), list(args)
            hi[arg], lo[arg] = args[arg] + d, args[arg] - d
            fd[idx] = (value(*hi) - value(*lo)) / (2 * h)
        assert np.max(np.abs(fd - g)) < 1e-7, (arg, np.max(np.abs(fd - g)))


def test_ragged_rules_of_the_restatement():
    """NaN on the padding of every input must not leak: the valid region equals the pair alone, everything else is 0, and a pair of
    count 0 adds nothing to dw and db"""
    counts, N, Cout, C0, C1 = [9, 5, 1, 0], 9, 6, 4, 3
    x0, x1, dy = (np.full(s, np.nan, np.float32) for s in ((4, C0, N), (4, C1, N), (4, Cout, N)))
    _, _, w, bias, _ = R.case(50, 1, Cout, C0, C1, N)
    alone = []
    for b, n in enumerate(counts):
        a0, a1, _, _, ga = R.case(50 + b, 1, Cout, C0, C1, max(n, 1))
        x0[b, :, :n], x1[b, :, :n], dy[b, :, :n] = a0[0, :, :n], a1[0, :, :n], ga[0, :, :n]
        alone.append(R.batch_reference(a0, a1, w, bias, ga) if n else None)
    for dtype in (torch.float64, torch.float32):
        res = R.batch_reference(x0, x1, w, bias, dy, counts, dtype)
        assert all(np.isfinite(a).all() for a in res.values())
        for b, n in enumerate(counts):
            for t in ("y", "dx"):
                assert not res[t][b, :, n:].any()
                if alone[b] is not None and dtype == torch.float64:
                    assert np.array_equal(res[t][b, :, :n], alone[b][t][0])
        without = R.batch_reference(x0[:3], x1[:3], w, bias, dy[:3], counts[:3], dtype)
        assert np.array_equal(res["dw"], without["dw"]) and np.array_equal(res["db"], without["db"]), "the empty pair adds nothing"
        if dtype == torch.float64:
            assert np.allclose(res["dw"], sum(a["dw"] for a in alone if a), rtol=1e-12, atol=1e-12)
            assert np.allclose(res["db"], sum(a["db"] for a in alone if a), rtol=1e-12, atol=1e-12)


def test_entry_points_are_declared_and_bound():
    """the Python surface has the documented signatures; a CPU tensor is an ImxError (the exported tables: tests/test_train_library_host.py)"""
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine, ImxError
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Engine.conv1x1_forward_train) == ["self", "x0", "w", "bias", "x1", "n"]
    assert sig(Engine.conv1x1_backward) == ["self", "x0", "w", "dy", "x1", "n", "want"]
    assert inspect.signature(Engine.conv1x1_backward).parameters["want"].default == (True, True, True, True)
    assert issubclass(sgtrain_grad.conv1x1, torch.autograd.Function)
    assert sig(sgtrain_grad.conv1x1.forward) == ["ctx", "engine", "x", "weight", "bias", "x1", "n"]
    assert sig(sgtrain_grad.conv1d) == ["engine", "x", "weight", "bias", "x1", "n"]
    assert sig(sgtrain_grad.attentional_propagation) == ["engine", "layer", "x", "source"]
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        sgtrain_grad.conv1d(None, torch.zeros(1, 4, 3), torch.zeros(2, 4, 1), torch.zeros(2))
