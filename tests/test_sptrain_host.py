"""SuperPoint descriptor training, host side: the project's restatement (tests/sptrain_ref.py) against the fixtures the reference
wrote (tests/golden/make_golden_sptrain.py), the erosion element written out, the Engine's methods and the drop-ins.  No GPU."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from tests import sptrain_ref as R
from tests import util
from tests.golden.make_golden_sptrain import DIMS, LAMDA_D, MARGIN, SETTINGS, desc_maps

FIXTURES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(util.GOLDEN, "sptrain_*.npz")))


def rel_close(a, b, tol=1e-5):
    return abs(a - b) <= tol * abs(b)


def test_fixture_set():
    assert len(FIXTURES) == 4 and {n.split("_")[1] for n in FIXTURES} == {"120x160", "136x200"}


@pytest.mark.parametrize("name", FIXTURES)
def test_labels_restatement(name):
    g = util.golden(name)
    H, W = (int(v) for v in g["size"])
    labels, flag = R.points_to_2d(g["pts"], H, W)
    assert flag == 0 and np.array_equal(labels, g["labels"])
    wl, res, kept = R.warp_labels(g["pts"], R.scale_pixels(g["homography"], H, W)[0], H, W)
    assert np.array_equal(wl, g["warped_labels"]) and 0 < wl.sum() < len(g["pts"])
    assert np.array_equal((np.abs(res).sum(0) != 0), g["warped_res_support"].astype(bool))
    assert np.array_equal(kept, g["warped_pnts"])                       # the same fp32 operations: bit for bit
    assert np.array_equal(res[:, wl == 1], g["warped_res"])


def test_labels_restatement_edges():
    eye = np.eye(3, dtype=np.float32)
    # an out-of-range point without matrices: flagged, written nowhere
    labels, flag = R.points_to_2d([[3.9, 2.1], [16.0, 1.0]], 8, 16)
    assert flag == 1 and labels.sum() == 1 and labels[2, 3] == 1
    # exact k + 0.5 ties round half to even; the residual keeps the sign
    shift = eye.copy()
    shift[0, 2], shift[1, 2] = 0.5, 1.5
    wl, res, _ = R.warp_labels([[2, 2], [3, 4]], shift, 8, 16)
    assert wl[4, 2] == 1 and wl[6, 4] == 1 and wl.sum() == 2           # 2.5 -> 2, 3.5 -> 4; 3.5 -> 4, 5.5 -> 6
    assert res[0, 4, 2] == 0.5 and res[1, 4, 2] == -0.5 and res[0, 6, 4] == -0.5
    # two points on one pixel: the higher index writes the residual
    sc = eye.copy()
    sc[0, 0] = 0.25
    wl, res, _ = R.warp_labels([[4, 1], [5, 1]], sc, 8, 16)           # 1.0 and 1.25 -> pixel 1
    assert wl.sum() == 1 and res[0, 1, 1] == 0.25


def test_erosion_element_written_out():
    assert R.ellipse(1).tolist() == [[0, 1], [1, 1]]
    assert R.ellipse(2).tolist() == [[0, 0, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]]
    assert R.ellipse(3).tolist() == [[0, 0, 0, 1, 0, 0], [0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1],
                                     [0, 1, 1, 1, 1, 1]]
    m = np.ones((8, 8), np.float32)
    m[4, 4] = 0
    e = R.erode(m, 1)
    assert sorted(map(tuple, np.argwhere(e == 0))) == [(4, 4), (4, 5), (5, 4)]      # out(y,x) reads in(y+i-1, x+j-1) over the set (i,j)
    assert np.array_equal(R.erode(m, 0), m) and R.erode(np.ones((8, 8), np.float32), 3).min() == 1     # outside pixels take no part


@pytest.mark.parametrize("name", FIXTURES)
def test_detector_loss_restatement(name):
    g = util.golden(name)
    labels = np.stack([g["labels"], g["warped_labels"]]).astype(np.float32)
    mask = np.stack([np.ones_like(g["warped_valid_mask"]), g["warped_valid_mask"]]).astype(np.float32)
    for i in (0, 1):
        for cond in (False, True):
            loss, msum = R.detector_loss(g["semi"][i:i + 1], labels[i:i + 1], mask[i:i + 1], conditioned=cond)
            assert rel_close(loss, g["det_loss_f64"][i]) and msum == g["det_mask_sum"][i], (i, cond, loss)
    both, _ = R.detector_loss(g["semi"], labels, mask)
    assert rel_close(both, g["det_loss_f64"][2])
    assert abs(g["det_loss_f32"][2] - g["det_loss_f64"][2]) <= 0.01 * (1e-4 + 1e-4 * abs(g["det_loss_f64"][2]))


def test_detector_loss_conditioned_form_beyond_the_written_one():
    """gaps 0, 40, 120, 200 with the label OFF the maximum: the exact cell value is 40 + 40 (-log p of the labelled channel, and
    -log(1 - p) of the maximum, whose complement is e^-40); the written form rounds p_max to 1 -- in float64 too -- and clamps at 100"""
    semi = np.full((1, 65, 1, 1), -200.0)
    semi[0, 0], semi[0, 1], semi[0, 2] = 0.0, -40.0, -120.0
    labels = np.zeros((1, 8, 8))
    labels[0, 0, 1] = 1
    ones = np.ones((1, 8, 8))
    good, _ = R.detector_loss(semi, labels, ones, conditioned=True)
    written, _ = R.detector_loss(semi, labels, ones, conditioned=False)
    scale = 1 + 1e-10                                                  # loss = cell / (1 + 1e-10)
    assert abs(good * scale - 80.0) < 1e-9 and abs(written * scale - 140.0) < 1e-9


@pytest.mark.parametrize("name", FIXTURES)
def test_desc_loss_restatement(name):
    g = util.golden(name)
    H, W = (int(v) for v in g["size"])
    Hc, Wc = H // 8, W // 8
    pa, pb = R.desc_pairs(R.scale_cells(g["homography"], Hc, Wc)[0], Hc, Wc)
    assert len(pa) == int(g["n_valid"]) and np.array_equal(pa, g["pair_a"]) and np.array_equal(pb, g["pair_b"])
    assert 121 <= len(pa) <= 425
    for si, (M, Rn) in enumerate(SETTINGS):
        choice, non = g[f"choice_{si}"], g[f"nonmatch_{si}"].astype(np.int64)
        assert choice.shape == (M,) and non.shape == (M, Rn) and choice.max() < len(pa)
        for d in DIMS:
            da, db = desc_maps(int(g["seed"]), d, Hc, Wc)
            for method in ("1d", "2d"):
                for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                    got = R.desc_loss(da, db, pa, pb, choice, non, LAMDA_D, MARGIN, method, dt)
                    ref = g[f"loss_{si}_{d}_{method}_{tag}"]
                    assert all(rel_close(got[k], ref[k]) for k in range(3)), (si, d, method, tag, got[:3], ref)
                    assert got[3] == int(g[f"hard_{si}_{d}"])


def test_entry_points_are_declared_and_bound():
    """the Engine has the methods of the stage (the exported tables: tests/test_train_library_host.py)"""
    from image_matching_amd.engine import Engine
    for m in ("warp_labels", "erode_mask", "detector_loss", "desc_loss_sparse", "desc_pairs", "sp_train_losses"):
        assert callable(getattr(Engine, m, None)), m


def test_dropins_import_and_raise_where_stated():
    from image_matching_amd.datasets.ALLSS import ALLSS
    from image_matching_amd.superpoint.loss_functions.sparse_loss import batch_descriptor_loss_sparse, descriptor_loss_sparse
    from image_matching_amd.superpoint.Train_model_heatmap import Train_model_heatmap
    assert list(inspect.signature(batch_descriptor_loss_sparse).parameters) == ["descriptors", "descriptors_warped", "homographies", "options"]
    assert list(inspect.signature(descriptor_loss_sparse).parameters)[:12] == [
        "descriptors", "descriptors_warped", "homographies", "mask_valid", "cell_size", "device", "descriptor_dist", "lamda_d",
        "num_matching_attempts", "num_masked_non_matches_per_match", "dist", "method"]
    assert list(inspect.signature(Train_model_heatmap.detector_loss).parameters) == ["self", "input", "target", "mask", "loss_type"]
    assert list(inspect.signature(ALLSS.__init__).parameters)[:3] == ["self", "export", "transform"]
    tm = Train_model_heatmap.__new__(Train_model_heatmap)
    with pytest.raises(NotImplementedError, match="backward"):
        tm.train()
    with pytest.raises(NotImplementedError, match="l2"):
        tm.detector_loss(None, None, None, loss_type="l2")
    for key in ("photometric", "gaussian_label"):
        cfg = {"augmentation": {"photometric": {"enable": key == "photometric"}}, "gaussian_label": {"enable": key == "gaussian_label"}}
        with pytest.raises(NotImplementedError, match="imgaug"):
            ALLSS(task="val", images=np.zeros((1, 16, 16), np.float32), points=[np.zeros((0, 2), np.float32)], **cfg)
