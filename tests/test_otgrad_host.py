"""The gradient of the SuperGlue match loss through the unrolled Sinkhorn, host side: the project's restatement (tests/otgrad_ref.py:
the recursion of DESIGN.md section 13 written out, no autograd) against the samples, row and column sums the reference's own autograd
wrote (tests/golden/make_golden_otgrad.py), against finite differences, and the Python surface of the entry points.  No GPU."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from tests import otgrad_ref as O
from tests import util
from tests.golden.make_golden_otgrad import CASES, RAGGED_FRAME, sample_positions

FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(util.GOLDEN, "otgrad_*.npz")))
ITEMS = [(name, k) for name in CASES for k in range(len(CASES[name]))]


def frac64(got, ref):
    """the worst fraction of 1e-5 + 1e-5 |ref| used"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))))


def item(g, k):
    return {key[:-len(f"_{k}")]: v for key, v in g.items() if key.endswith(f"_{k}")}


def test_fixture_set():
    assert FIXTURES == sorted(f"otgrad_{n}.npz" for n in CASES)
    for name, items in CASES.items():
        path = os.path.join(util.GOLDEN, f"otgrad_{name}.npz")
        g = util.golden(f"otgrad_{name}.npz")
        assert os.path.getsize(path) < 1000000 and int(g["n_items"]) == len(items)
        for k, (seed, m, n, iters) in enumerate(items):
            it = item(g, k)
            scores, matches = O.case_scores(seed, m, n)
            assert np.array_equal(it["scores"].view(np.int32), scores.view(np.int32)) and np.array_equal(it["matches"], matches), "the recipe regenerates the inputs bit for bit"
            assert int(it["iters"]) == iters and np.isfinite([it["loss32"], it["loss64"]]).all() and np.isfinite(it["g"]).all()
            assert 4.0 < scores.std() < 6.5 and np.abs(scores).max() > 25, "heavy-tailed scores of standard deviation about 5"
    assert [int(item(util.golden("otgrad_iters.npz"), k)["iters"]) for k in range(4)] == [0, 1, 2, 3]
    assert all(m <= RAGGED_FRAME[0] and n <= RAGGED_FRAME[1] for _, m, n, _ in CASES["ragged"])


@pytest.mark.parametrize("name,k", ITEMS)
def test_restatement_float64(name, k):
    """samples, row sums, column sums, d bin_score and the value within 1e-5 + 1e-5 |ref| of the reference's float64 autograd"""
    it = item(util.golden(f"otgrad_{name}.npz"), k)
    loss, g, gbin, flag = O.loss_grad(it["scores"], float(it["bin"]), it["matches"], int(it["iters"]))
    pos = sample_positions(int(it["seed"]), g.size)
    f = max(frac64(g.reshape(-1)[pos], it["g"]), frac64(g.sum(1), it["rows"]), frac64(g.sum(0), it["cols"]), frac64(gbin, it["gbin64"]),
            frac64(loss, it["loss64"]))
    print(f"{name}[{k}]: the float64 restatement uses {f:.3g} of 1e-5 + 1e-5 |ref|")
    assert flag == 0 and f <= 1.0


@pytest.mark.parametrize("name,k", ITEMS)
def test_restatement_fp32(name, k):
    """the recursion in fp32 at the default bar, at gout = n_all: the direct term is -1 per listing and the gradient O(1)"""
    it = item(util.golden(f"otgrad_{name}.npz"), k)
    K = it["matches"].shape[1]
    loss, g, gbin, _ = O.loss_grad(it["scores"], float(it["bin"]), it["matches"], int(it["iters"]), gout=float(K), dtype=torch.float32)
    pos = sample_positions(int(it["seed"]), g.size)
    ref, d32 = K * it["g"], K * it["d32"].astype(np.float64)
    f = float(np.max(np.abs(g.reshape(-1)[pos] - ref) / O.bar(ref, d32)))
    fb = float(abs(gbin - K * it["gbin64"]) / O.bar(K * it["gbin64"], K * (it["gbin32"] - it["gbin64"])))
    fl = float(abs(loss - it["loss64"]) / (1e-4 + 1e-4 * abs(it["loss64"])))
    print(f"{name}[{k}]: the fp32 restatement uses {f:.3g} of the default bar on d scores, {fb:.3g} on d bin_score, {fl:.3g} on the value")
    assert max(f, fb, fl) <= 1.0


def test_restatement_against_finite_differences():
    """a 5 x 4 pair, float64, central differences of the written loss in every score and in bin_score"""
    scores, matches = O.case_scores(11, 5, 4)
    scores = scores.astype(np.float64) / 3
    matches = np.concatenate([matches, matches[:, :1]], 1)               # one listing twice
    for iters in (0, 1, 4):
        loss, g, gbin, _ = O.loss_grad(scores, 0.7, matches, iters)
        assert abs(loss - O.loss_autograd(scores, 0.7, matches, iters)[0]) < 1e-12
        h = 1e-5
        fd = np.zeros_like(scores)
        for i in range(5):
            for j in range(4):
                d = np.zeros_like(scores)
                d[i, j] = h
                fd[i, j] = (O.loss_grad(scores + d, 0.7, matches, iters)[0] - O.loss_grad(scores - d, 0.7, matches, iters)[0]) / (2 * h)
        fdb = (O.loss_grad(scores, 0.7 + h, matches, iters)[0] - O.loss_grad(scores, 0.7 - h, matches, iters)[0]) / (2 * h)
        assert np.max(np.abs(fd - g)) < 1e-8 and abs(fdb - gbin) < 1e-8, (iters, np.max(np.abs(fd - g)), fdb - gbin)


def test_list_rules_of_the_restatement():
    scores, matches = O.case_scores(12, 6, 5)
    l1, g1, b1, f1 = O.loss_grad(scores, 1.0, matches, 3)
    bad = np.concatenate([matches, np.array([[7], [0]])], 1)             # x = 7 > m = 6: flagged, inert, but K counts it
    l2, g2, b2, f2 = O.loss_grad(scores, 1.0, bad, 3)
    K = matches.shape[1]
    assert f1 == 0 and f2 == O.FLAG_INDEX and np.allclose(g2 * (K + 1), g1 * K, rtol=1e-10, atol=1e-14) and abs(l2 * (K + 1) - l1 * K) < 1e-12
    assert O.loss_grad(scores, 1.0, matches[:, :0], 3)[:3:2] == (0.0, 0.0)
    lo = scores.copy()
    lo[0, 0] = -400.0                                                    # a listed entry whose exp underflows: +inf, finite gradient
    one = np.array([[0], [0]])
    l3, g3, b3, _ = O.loss_grad(lo, 1.0, one, 3, dtype=torch.float32)
    assert l3 == np.inf and np.isfinite(g3).all() and np.isfinite(b3)
    assert np.isnan(O.loss_autograd(lo, 1.0, one, 3, dtype=torch.float32)[1]).any(), "torch's own gradient is NaN there"
    g3_64 = O.loss_grad(lo, 1.0, one, 3)[1]
    assert np.max(np.abs(g3 - g3_64) / O.bar(g3_64)) <= 1.0


def test_entry_points_are_declared_and_bound():
    """the Python surface has the documented signatures; a CPU tensor is an error (the exported tables: tests/test_train_library_host.py)"""
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Engine.ot_match_loss_grad)[:9] == ["self", "scores", "bin_score", "all_matches", "n_all", "iters", "n0", "n1", "gout"]
    assert issubclass(sgtrain_grad.ot_match_loss, torch.autograd.Function)
    assert sig(sgtrain_grad.ot_match_loss.forward)[:7] == ["ctx", "engine", "scores", "bin_score", "all_matches", "n_all", "iters"]
    assert sig(sgtrain_grad.match_loss)[:6] == ["engine", "scores", "bin_score", "all_matches", "n_all", "iters"]
    with pytest.raises(Exception, match="contiguous fp32 cuda"):
        sgtrain_grad.match_loss(None, torch.zeros(1, 3, 3), torch.zeros(()), torch.zeros(1, 2, 6, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 3)
