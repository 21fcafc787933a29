"""The attention of SuperGlue's GNN, forward and backward, host side: the project's restatement (tests/mhagrad_ref.py: the closed forms
of DESIGN.md section 14 written out, no autograd) against the samples and per-head sums the reference's own attention wrote under
torch.autograd (tests/golden/make_golden_mhagrad.py), against autograd of the same written forward, against finite differences, the
ragged rules, and the Python surface of the entry points.  No GPU."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from tests import mhagrad_ref as R
from tests import util
from tests.golden.make_golden_mhagrad import CASES, RAGGED_FRAME, TENSORS, sample_positions

FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(util.GOLDEN, "mhagrad_*.npz")))
ITEMS = [(name, k) for name in CASES for k in range(len(CASES[name]))]


def frac64(got, ref):
    """the worst fraction of 1e-5 + 1e-5 |ref| used"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))))


def item(g, k):
    return {key[:-len(f"_{k}")]: v for key, v in g.items() if key.endswith(f"_{k}")}


def restated(name, k, dtype):
    it = item(util.golden(f"mhagrad_{name}.npz"), k)
    seed, (D, H, N, M) = int(it["seed"]), (int(x) for x in it["shape"])
    q, kk, v, dout = R.case(seed, 1, D, H, N, M)
    res = R.batch_reference(q, kk, v, dout, dtype=dtype)
    return it, seed, len(CASES[name]), res


def test_fixture_set():
    assert FIXTURES == sorted(f"mhagrad_{n}.npz" for n in CASES)
    assert [c[0][1:] for c in (CASES["d32"], CASES["d64"], CASES["d16"])] == [(32, 4, 70, 100), (64, 4, 100, 130), (16, 4, 50, 45)]
    for name, items in CASES.items():
        path = os.path.join(util.GOLDEN, f"mhagrad_{name}.npz")
        g = util.golden(f"mhagrad_{name}.npz")
        assert os.path.getsize(path) < 75000 and int(g["n_items"]) == len(items)
        for k, (seed, D, H, N, M) in enumerate(items):
            it = item(g, k)
            assert int(it["seed"]) == seed and tuple(int(x) for x in it["shape"]) == (D, H, N, M)
            for t in TENSORS:
                assert np.isfinite(it[f"{t}_g"]).all() and np.isfinite(it[f"{t}_d32"]).all() and it[f"{t}_sum"].shape == (H,)
    assert all(N <= RAGGED_FRAME[0] and M <= RAGGED_FRAME[1] for _, _, _, N, M in CASES["ragged"])
    q = R.case(1, 1, 32, 4, 70, 100)[0]
    assert 1.0 < q.std() < 1.3 and np.abs(q).max() > 6, "heavy-tailed inputs of standard deviation about 1.13"


@pytest.mark.parametrize("name,k", ITEMS)
def test_restatement_float64(name, k):
    """samples and per-head sums of out, dq, dk, dv within 1e-5 + 1e-5 |ref| of the reference's float64 autograd"""
    it, seed, n, res = restated(name, k, torch.float64)
    f = 0.0
    for t in TENSORS:
        pos = sample_positions(seed, t, res[t].size, n)
        f = max(f, frac64(res[t].reshape(-1)[pos], it[f"{t}_g"]), frac64(res[t][0].sum(axis=(0, 2)), it[f"{t}_sum"]))
    print(f"{name}[{k}]: the float64 restatement uses {f:.3g} of 1e-5 + 1e-5 |ref|")
    assert f <= 1.0


@pytest.mark.parametrize("name,k", ITEMS)
def test_restatement_fp32(name, k):
    """the closed forms in fp32 at the default bar on the samples"""
    it, seed, n, res = restated(name, k, torch.float32)
    fr = {}
    for t in TENSORS:
        pos = sample_positions(seed, t, res[t].size, n)
        fr[t] = float(np.max(np.abs(res[t].reshape(-1)[pos] - it[f"{t}_g"]) / R.bar(it[f"{t}_g"], it[f"{t}_d32"])))
    print(f"{name}[{k}]: the fp32 restatement uses " + ", ".join(f"{v:.3g} ({t})" for t, v in fr.items()) + " of the default bar")
    assert max(fr.values()) <= 1.0


@pytest.mark.parametrize("shape", [(2, 16, 2, 9, 13), (1, 32, 3, 40, 33), (2, 64, 1, 1, 7)])
def test_closed_form_against_autograd(shape):
    """float64: the closed forms and torch.autograd of the same written forward agree to rounding"""
    q, k, v, dout = R.case(31 + shape[3], *shape)
    res = R.batch_reference(q, k, v, dout)
    out, dq, dk, dv = R.autograd(q, k, v, dout)
    for got, ref in ((res["out"], out), (res["dq"], dq), (res["dk"], dk), (res["dv"], dv)):
        assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.abs(ref).max())
    S = np.einsum("bdhn,bdhm->bhnm", q.astype(np.float64), k.astype(np.float64)) / shape[1] ** .5
    assert np.max(np.abs(res["lse"] - np.log(np.exp(S).sum(-1)))) < 1e-12


def test_restatement_against_finite_differences():
    """(D, H, N, M) = (16, 1, 3, 4), float64, central differences of sum(out * dout) in every element of q, k and v"""
    q, k, v, dout = (a.astype(np.float64) for a in R.case(11, 1, 16, 1, 3, 4))
    dq, dk, dv = R.backward(q, k, v, dout)
    value = lambda q_, k_, v_: float((R.forward(q_, k_, v_)[0] * dout).sum())
    h = 1e-6
    for x, g, arg in ((q, dq, 0), (k, dk, 1), (v, dv, 2)):
        fd = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            d = np.zeros_like(x)
            d[idx] = h
            hi, lo = [q, k, v], [q, k, v]
            hi[arg], lo[arg] = x + d, x - d
            fd[idx] = (value(*hi) - value(*lo)) / (2 * h)
        assert np.max(np.abs(fd - g)) < 1e-7, (arg, np.max(np.abs(fd - g)))


def test_ragged_rules_of_the_restatement():
    """NaN on the padding of every input must not leak: the valid region equals the pair alone, everything else is 0"""
    counts = [(9, 13), (5, 1), (1, 13), (0, 6), (4, 0)]
    N, M, D, H = 9, 13, 16, 2
    q, k, v, dout = (np.full(s, np.nan, np.float32) for s in ((5, D, H, N), (5, D, H, M), (5, D, H, M), (5, D, H, N)))
    alone = []
    for b, (n, m) in enumerate(counts):
        qa, ka, va, ga = R.case(50 + b, 1, D, H, max(n, 1), max(m, 1))
        q[b, :, :, :n], k[b, :, :, :m], v[b, :, :, :m], dout[b, :, :, :n] = qa[0, :, :, :n], ka[0, :, :, :m], va[0, :, :, :m], ga[0, :, :, :n]
        alone.append(R.batch_reference(qa, ka, va, ga) if n and m else None)
    nq, nk = [c[0] for c in counts], [c[1] for c in counts]
    for dtype in (torch.float64, torch.float32):
        res = R.batch_reference(q, k, v, dout, nq, nk, dtype)
        assert all(np.isfinite(a).all() for a in res.values())
        for b, (n, m) in enumerate(counts):
            for t, cnt in (("out", n), ("dq", n), ("dk", m), ("dv", m)):
                assert not res[t][b, :, :, cnt:].any()
                if alone[b] is None:
                    assert not res[t][b].any()
                elif dtype == torch.float64:
                    assert np.array_equal(res[t][b, :, :, :cnt], alone[b][t][0])
            assert not res["lse"][b, :, n:].any()


def test_entry_points_are_declared_and_bound():
    """the Python surface has the documented signatures; a CPU tensor is an ImxError (the exported tables: tests/test_train_library_host.py)"""
    from image_matching_amd import sgtrain_grad
    from image_matching_amd.engine import Engine, ImxError
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Engine.mha_forward_train) == ["self", "q", "k", "v", "nq", "nk", "want_lse"]
    assert sig(Engine.mha_backward) == ["self", "q", "k", "v", "out", "lse", "dout", "nq", "nk", "want"]
    assert inspect.signature(Engine.mha_backward).parameters["want"].default == (True, True, True)
    assert issubclass(sgtrain_grad.mha, torch.autograd.Function)
    assert sig(sgtrain_grad.mha.forward) == ["ctx", "engine", "query", "key", "value", "nq", "nk"]
    assert sig(sgtrain_grad.attention) == ["engine", "query", "key", "value", "nq", "nk"]
    with pytest.raises(ImxError, match="contiguous fp32 cuda"):
        sgtrain_grad.attention(None, torch.zeros(1, 16, 2, 3), torch.zeros(1, 16, 2, 4), torch.zeros(1, 16, 2, 4))
