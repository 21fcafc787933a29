"""Gradients of the two SuperPoint training losses, host side: the project's restatement (tests/spgrad_ref.py) against the samples and
per-cell norms the reference's own autograd wrote (tests/golden/make_golden_spgrad.py), crafted hinge and clamp cases through the
restatement, and the Python surface of the entry points.  No GPU."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from tests import spgrad_ref as G
from tests import sptrain_ref as R
from tests import util
from tests.golden.make_golden_spgrad import DET_CASES, METHODS, desc_key, det_key, sample_positions
from tests.golden.make_golden_sptrain import DIMS, LAMDA_D, MARGIN, SETTINGS, desc_maps

FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(util.GOLDEN, "spgrad_*.npz")))


def frac64(got, ref):
    """the worst fraction of 1e-5 + 1e-5 |ref| used"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (1e-5 + 1e-5 * np.abs(ref))))


def check_against_fixture(g, seed, key, name, norm_name, g64, g32):
    """a float64 and an fp32 gradient of one tensor against its samples and per-cell norms: (fraction of the float64 bar, of the default bar)"""
    pos = sample_positions(seed, key, g64.size)
    ref = g[name].astype(np.float64)
    f64 = max(frac64(g64.reshape(-1)[pos], ref), frac64(G.cell_l1(g64), g[norm_name]))
    f32 = float(np.max(np.abs(g32.reshape(-1)[pos] - ref) / G.bar(ref, g[name + "_d32"])))
    return f64, f32


def test_fixture_set():
    assert len(FIXTURES) == 4 and {n.split("_")[1] for n in FIXTURES} == {"120x160", "136x200"}
    for n in FIXTURES:
        assert os.path.exists(os.path.join(util.GOLDEN, n.replace("spgrad_", "sptrain_"))) and os.path.getsize(os.path.join(util.GOLDEN, n)) < 1000000


@pytest.mark.parametrize("name", FIXTURES)
def test_detector_grad_restatement(name):
    g, src = util.golden(name), util.golden(name.replace("spgrad_", "sptrain_"))
    seed = int(g["seed"])
    labels = np.stack([src["labels"], src["warped_labels"]]).astype(np.float32)
    mask = np.stack([np.ones_like(src["warped_valid_mask"]), src["warped_valid_mask"]]).astype(np.float32)
    worst = [0.0, 0.0]
    for case, sl in zip(DET_CASES, (slice(0, 1), slice(1, 2), slice(0, 2))):
        args = (src["semi"][sl], labels[sl], mask[sl])
        cond = G.detector_grad(*args, conditioned=True)[1]
        written = G.detector_grad(*args, conditioned=False)[1]
        w32 = G.detector_grad(*args, dtype=torch.float32, conditioned=False)[1]
        assert frac64(cond, written) <= 1.0, "the conditioned and the written form agree on the fixtures"
        assert np.max(np.abs(G.detector_grad_closed(*args) - cond)) <= 1e-12, "the rule written out equals autograd of the conditioned form"
        for g64 in (cond, written):
            f64, f32 = check_against_fixture(g, seed, det_key(case), f"gdet_{case}", f"ndet_{case}", g64, w32)
            worst = [max(worst[0], f64), max(worst[1], f32)]
    print(f"{name}: detector gradient at most {worst[0]:.3g} of the float64 bar, {worst[1]:.3g} of the default bar (fp32)")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


@pytest.mark.parametrize("name", FIXTURES)
def test_desc_grad_restatement(name):
    g, src = util.golden(name), util.golden(name.replace("spgrad_", "sptrain_"))
    seed = int(g["seed"])
    H, W = (int(v) for v in src["size"])
    Hc, Wc = H // 8, W // 8
    worst = [0.0, 0.0]
    for si in range(len(SETTINGS)):
        choice, non = src[f"choice_{si}"], src[f"nonmatch_{si}"].astype(np.int64)
        for d in DIMS:
            da, db = desc_maps(seed, d, Hc, Wc)
            for method in METHODS:
                a = (da, db, src["pair_a"], src["pair_b"], choice, non, LAMDA_D, MARGIN, method)
                l64, l32 = G.desc_grad(*a), G.desc_grad(*a, dtype=torch.float32)
                assert abs(l64[0] - src[f"loss_{si}_{d}_{method}_f64"][0]) <= 1e-5 * abs(l64[0])
                for side, s in enumerate("ab"):
                    f64, f32 = check_against_fixture(g, seed, desc_key(si, d, method, side), f"g{s}_{si}_{d}_{method}", f"n{s}_{si}_{d}_{method}",
                                                     l64[1 + side], l32[1 + side])
                    assert f64 <= 1.0 and f32 <= 1.0, (si, d, method, s, f64, f32)
                    worst = [max(worst[0], f64), max(worst[1], f32)]
    print(f"{name}: descriptor gradient at most {worst[0]:.3g} of the float64 bar, {worst[1]:.3g} of the default bar (fp32), 24 combinations")


def collisions(src, si=2):
    """(the most match entries one a cell receives, the most non-match rows one b cell receives) in setting si"""
    ia = src["pair_a"][src[f"choice_{si}"]]
    return int(np.bincount(ia).max()), int(np.bincount(src[f"nonmatch_{si}"].astype(np.int64).reshape(-1)).max())


@pytest.mark.parametrize("name", FIXTURES)
def test_the_512_8_setting_collides(name):
    m, n = collisions(util.golden(name.replace("spgrad_", "sptrain_")))
    assert SETTINGS[2] == (512, 8) and m >= 2 and n >= 8, (m, n)


def tiny(Hc=2, Wc=2, d=4):
    a = np.zeros((d, Hc, Wc))
    a[0] = 1.0                                                           # every cell of a: e_0, unit norm
    pa = np.arange(Hc * Wc)
    return a, pa


def test_match_hinge_rules():
    """inactive where <a, b> > 1 (b = 1.5 a); at exactly 0 (b = a, unit norm) the gradient passes: torch.clamp(min=0) is inclusive"""
    a, pa = tiny()
    choice, non = np.array([1]), np.array([[2]])
    ortho = np.zeros_like(a)
    ortho[1] = 1.0                                                       # the non-match row is orthogonal to a: below the margin, inactive
    for method in METHODS:
        b = 1.5 * a
        b[:, 1, 0] = ortho[:, 1, 0]                                      # cell 2 of b
        loss, ga, gb = G.desc_grad(a, b, pa, pa, choice, non, 250., 0.2, method)
        assert loss == 0.0 and not ga.any() and not gb.any()
    b = a.copy()
    b[:, 1, 0] = ortho[:, 1, 0]
    loss, ga, gb = G.desc_grad(a, b, pa, pa, choice, non, 250., 0.2, "1d")
    assert loss == 0.0                                                   # 1 - <a, b> is exactly 0 ...
    assert np.array_equal(ga.reshape(4, -1)[:, 1], -250. * b.reshape(4, -1)[:, 1]) and np.array_equal(gb.reshape(4, -1)[:, 1], -250. * a.reshape(4, -1)[:, 1])
    assert np.count_nonzero(ga) == 1 and np.count_nonzero(gb) == 1       # ... and the gradient passes, at the matched cell only
    with torch.enable_grad():
        assert torch.autograd.grad(torch.clamp(x := torch.tensor([-1., 0., 1.], requires_grad=True), min=0).sum(), x)[0].tolist() == [0., 1., 1.]


def test_non_match_hinge_is_strict_and_counts_are_constants():
    a, pa = tiny()
    b = np.zeros_like(a)
    b[0] = np.array([[0.2, 0.7], [0.1, 0.9]])                            # products with a: 0.2 (at the margin: inactive), 0.7, 0.1, 0.9
    b[1, 0, 0] = 1.0
    choice, non = np.array([0]), np.array([[0, 1, 2, 3]])
    loss, ga, gb = G.desc_grad(a, b, pa, pa, choice, non, 0.0, 0.2, "1d")
    flat = gb.reshape(4, -1)
    assert not flat[:, 0].any() and not flat[:, 2].any()                 # strict: nothing at the margin, nothing below it
    assert np.allclose(flat[:, 1], a.reshape(4, -1)[:, 0] / 3) and np.allclose(flat[:, 3], a.reshape(4, -1)[:, 0] / 3)    # 2 hard negatives + 1
    assert np.allclose(ga.reshape(4, -1)[:, 0], (b.reshape(4, -1)[:, 1] + b.reshape(4, -1)[:, 3]) / 3)


def test_detector_grad_at_logit_gaps_0_40_120_200():
    """the conditioned derivative stays finite and a clamped term gives zero; the rule written out (the kernel's) equals autograd"""
    semi = np.full((1, 65, 1, 3), -200.0)
    semi[0, 0], semi[0, 1], semi[0, 2] = 0.0, -40.0, -120.0
    semi[0, :, 0, 0] = 0.0                                               # cell 0: gap 0 everywhere
    labels = np.zeros((1, 8, 24))
    labels[0, 0, 0] = 1                                                  # cell 0: on channel 0
    labels[0, 0, 8 + 1] = 1                                              # cell 1: on the channel 40 below
    labels[0, 0, 16 + 2] = 1                                             # cell 2: on the channel 120 below: -log p clamps at 100
    ones = np.ones((1, 8, 24))
    loss, g = G.detector_grad(semi, labels, ones)
    closed = G.detector_grad_closed(semi, labels, ones)
    assert np.isfinite(g).all() and np.isfinite(closed).all() and np.max(np.abs(g - closed)) <= 1e-12
    g = g[0, :, 0, :] * (3 + 1e-10)                                      # per cell, without 1 / D
    assert abs(g[0, 0] + 1) < 1e-12 and np.allclose(g[1:, 0], 1 / 64, atol=1e-12)    # gap 0: q = (-1, 1/64, ...), sum q = 0
    assert abs(g[1, 1] + 2) < 1e-12 and abs(g[0, 1] - 2) < 1e-12         # cell 1: -t_1 - p_1 q_0 with q_0 = p_0 / (1 - p_0) = e^40: -1 - 1
    assert abs(g[2, 2]) < 1e-30                                          # cell 2, the labelled channel: its -log p term is clamped, a constant
    assert (np.abs(g[3:, 1:]) < 1e-30).all()                             # gap 200: -log p clamped and t = 0, ratio e^-200
    # the written form in float64 rounds p_max to 1 there: its derivative is no longer that of the value the library returns
    written = G.detector_grad(semi, labels, ones, conditioned=False)[1]
    assert not np.allclose(written[0, :, 0, 1], g[:, 1] / (3 + 1e-10), atol=1e-3)


def test_entry_points_are_declared_and_bound():
    """the Python surface has the documented signatures; a CPU tensor is an error (the exported tables: tests/test_train_library_host.py)"""
    from image_matching_amd import sptrain_grad
    from image_matching_amd.engine import Engine
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(Engine.detector_loss_grad)[:5] == ["self", "semi", "labels", "mask", "gout"]
    assert sig(Engine.desc_loss_sparse_grad)[:10] == ["self", "desc_a", "desc_b", "homographies", "choice", "nonmatch_b", "lamda_d", "margin", "method", "gout"]
    assert sig(Engine.sp_train_loss_grads) == sig(Engine.sp_train_losses) and "lambda_loss" in sig(Engine.sp_train_loss_grads)
    for f in (sptrain_grad.detector_loss, sptrain_grad.sparse_descriptor_loss):
        assert issubclass(f, torch.autograd.Function)
    assert sig(sptrain_grad.detector_loss.forward) == ["ctx", "engine", "semi", "labels", "mask"]
    assert sig(sptrain_grad.sparse_descriptor_loss.forward)[:7] == ["ctx", "engine", "desc_a", "desc_b", "homographies", "choice", "nonmatch_b"]
    assert sig(sptrain_grad.total_loss)[:7] == ["engine", "semi", "semi_warp", "desc", "desc_warp", "sample", "lambda_loss"]
    with pytest.raises(Exception, match="contiguous fp32 cuda"):
        sptrain_grad.detector_loss.apply(None, torch.zeros(1, 65, 1, 1), torch.zeros(1, 8, 8), torch.zeros(1, 8, 8))
