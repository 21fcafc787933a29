"""SuperGlue training pairs without a GPU: the project's restatement (tests/trainpairs_ref.py) against the fixtures the REFERENCE
wrote (tests/golden/make_golden_trainpairs.py), the declarations of the three entry points, and the drop-in classes."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import superglue_ref
from tests import trainpairs_ref as R
from tests import util

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PIPE = ("trainpairs_small.npz", "trainpairs_ragged.npz")


def samples(name):
    g = util.golden(name)
    return g, range(len(g["seeds"]))


@pytest.mark.parametrize("name", PIPE)
def test_restatement_equals_the_reference_on_the_pipeline_fixtures(name):
    g, idx = samples(name)
    assert len(idx) == 3
    assert len({g[f"M_{i}"].tobytes() for i in idx}) == 3, "the three samples must carry three different matrices"
    for i in idx:
        proj = R.project(g[f"kpts0_{i}"], g[f"M_{i}"])
        assert proj.dtype == np.float32 and np.array_equal(proj.view(np.uint32), g[f"proj_{i}"].view(np.uint32)), f"{name} sample {i}: projection"
        out = R.gt_matches(proj, g[f"kpts1_{i}"])
        assert np.array_equal(out["matches"], g[f"matches_{i}"]), f"{name} sample {i}: matches"
        assert np.array_equal(out["all_matches"], g[f"all_matches_{i}"]), f"{name} sample {i}: all_matches"
        # the fixture's recorded margins are the restatement's, and far above the refusal limit
        m = R.margins(out["dists"])
        mine = np.array([m["row_gap"].min(), m["col_gap"].min(), m["radius_gap"].min()])
        assert np.array_equal(mine, g[f"margins_{i}"]) and mine.min() >= 1e-6
    if name == "trainpairs_ragged.npz":
        for i in idx:
            n0, n1 = len(g[f"kpts0_{i}"]), len(g[f"kpts1_{i}"])
            assert n0 != n1 and max(n0, n1) < int(g["cap"])


@pytest.mark.parametrize("name", PIPE)
def test_restated_warp_equals_the_fixture(name):
    g, idx = samples(name)
    for i in idx:
        img, minv = g[f"image_{i}"], R.invert3(g[f"M_{i}"])
        w = R.warp_perspective_u8(img, minv)
        assert np.array_equal(w, g[f"warped_{i}"])
        # the integer weights are the exact bilinear weights times 2^15: the rounded value is the rounded float64 bilinear
        assert np.abs(w.astype(np.float64) - R.warp_bilinear_f64(img, minv)).max() <= 0.5 + 1e-9
        b = R.warp_boundary_pixels(minv, *img.shape)
        assert np.array_equal(b, g[f"boundary_{i}"].reshape(-1, 2)) and len(b) <= 1e-4 * img.size
        assert 0.2 < (w > 0).mean(), "the warp left almost nothing of the image"


def test_restatement_equals_the_reference_on_the_edge_fixture():
    g = util.golden("trainpairs_edge.npz")
    names = [str(n) for n in g["names"]]
    assert {"none", "all", "two_to_one", "radius", "one_0", "one_1", "ties"} <= set(names)
    for n in names:
        proj = R.project(g[f"kpts0_{n}"], g[f"M_{n}"])
        assert np.array_equal(proj.view(np.uint32), g[f"proj_{n}"].view(np.uint32)), n
        out = R.gt_matches(proj, g[f"kpts1_{n}"])
        assert np.array_equal(out["matches"], g[f"matches_{n}"]), n
        assert np.array_equal(out["all_matches"], g[f"all_matches_{n}"]), n
    # what the cases are there for
    assert g["matches_none"].shape[1] == 0 and g["all_matches_none"].shape[1] == 12 + 9
    assert g["matches_all"].shape[1] == 40 and g["all_matches_all"].shape[1] == 40
    assert g["matches_two_to_one"].tolist() == [[0, 2], [0, 1]]           # the nearer of the two takes the point
    assert g["matches_radius"].tolist() == [[0, 2], [0, 2]]               # 2.999 matches, 3.001 does not
    assert g["matches_ties"].tolist() == [[0, 2, 4, 6], [0, 3, 5, 6]]     # the lowest index wins on either side (rows 1, 3, 5 lose their ties)
    assert g["margins_ties"].min() == 0.0


@pytest.mark.parametrize("name", PIPE)
def test_restated_loss_equals_the_reference(name):
    g, idx = samples(name)
    gd = util.golden(name.replace(".npz", "_desc.npz"))
    sd, cfg = util.sg_sd(128, variant="t"), util.sg_config(128)
    H, W = g["image_0"].shape
    for i in idx:
        data = {"keypoints0": torch.from_numpy(g[f"kpts0_{i}"])[None], "keypoints1": torch.from_numpy(g[f"kpts1_{i}"])[None],
                "scores0": torch.from_numpy(g[f"scores0_{i}"])[None], "scores1": torch.from_numpy(g[f"scores1_{i}"])[None],
                "descriptors0": torch.from_numpy(gd[f"desc0_{i}"])[None], "descriptors1": torch.from_numpy(gd[f"desc1_{i}"])[None],
                "image_shape0": (1, 1, H, W), "image_shape1": (1, 1, H, W)}
        Z = superglue_ref.superglue_forward(data, sd, cfg, return_dense=True)["dense"]["Z"][0].numpy()
        loss = R.match_loss(Z, g[f"all_matches_{i}"])
        ref = g[f"loss_t_{i}"]
        print(f"{name} sample {i}: loss {float(loss):.6f}, reference {float(ref[0]):.6f}, float64 {float(g[f'loss_t_f64_{i}'][0]):.6f}")
        util.assert_close(np.array([loss]), ref, f"{name} sample {i}: loss")
        util.assert_close(np.array([R.match_loss(Z.astype(np.float64), g[f"all_matches_{i}"], np.float64)]), g[f"loss_t_f64_{i}"], f"{name} sample {i}: float64 loss")


def test_loss_restatement_underflow_and_empty():
    Z = np.array([[-1.0, -250.0], [-2.0, -3.0]], np.float32)
    assert R.match_loss(Z, np.array([[0, 1], [0, 0]])) == np.float32(1.5)
    assert np.isposinf(R.match_loss(Z, np.array([[0, 0], [0, 1]])))
    assert R.match_loss(Z, np.zeros((2, 0), np.int64)) == 0


def test_entry_points_are_declared():
    header = open(os.path.join(ROOT, "include", "imx.h")).read()
    from image_matching_amd import _lib
    for n in ("imx_warp_perspective_u8", "imx_gt_matches", "imx_match_loss"):
        assert re.search(r"^IMX_API int " + n + r"\(", header, re.M), n
        assert n in _lib.EXPORTS
    assert len(_lib.EXPORTS) == 34 == len(set(re.findall(r"^IMX_API [^\n]*?\b(imx_\w+)\(", header, re.M)))


def test_dropin_classes_import_and_refuse_training():
    from image_matching_amd.datasets.GlueSparse import GlueSparse
    from image_matching_amd.superglue.models.superglue_train import SuperGlue
    import inspect
    assert list(inspect.signature(GlueSparse.__init__).parameters) == ["self", "train_path", "sp_config", "resize", "device"]
    sg = SuperGlue(util.sg_config(128))
    assert sg.config["weights"] is None and sg.config["descriptor_dim"] == 128
    assert SuperGlue.default_config["weights"] == "" and SuperGlue.default_config["sinkhorn_iterations"] == 100
    with pytest.raises(NotImplementedError, match="backward"):
        sg.train()
    assert sg.eval() is sg
    # no keypoints on a side: the reference's early return (superglue_train.py:238-246), no GPU involved
    out = sg({"keypoints0": torch.zeros(1, 1, 0, 2), "keypoints1": torch.zeros(1, 1, 5, 2),
              "descriptors0": torch.zeros(128, 1, 0), "descriptors1": torch.zeros(128, 1, 5)})
    assert out["skip_train"] is True and out["matches1"].dtype == torch.int32 and out["matches1"].tolist() == [-1] * 5 and out["matches0"].shape == (0,)


def test_dataset_skip_dict_and_key_set_match_the_fixture():
    from image_matching_amd import trainpairs
    g = util.golden("trainpairs_edge.npz")
    img = np.zeros((12, 16), np.uint8)
    skip = trainpairs.skip_sample(img, img, "a.png")
    assert sorted(skip) == [str(k) for k in g["skip_keys"]]
    for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1"):
        assert skip[k].dtype == torch.double and list(skip[k].shape) == g["skip_shape_" + k].tolist()
    # a full sample, from host arrays shaped like Engine.train_pairs' output: the reference's keys, containers and dtypes
    small = util.golden("trainpairs_small.npz")
    K, d, n0, n1 = 8, 4, 5, 3
    host = {"counts0": np.array([n0]), "counts1": np.array([n1]), "n_matches": np.array([2]), "n_all": np.array([6]),
            "all_matches": np.array([[[0, 4, 1, 2, 3, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1], [1, 2, 3, 3, 3, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1]]], np.int64),
            "keypoints0": np.zeros((1, K, 2), np.float32), "keypoints1": np.zeros((1, K, 2), np.float32),
            "scores0": np.zeros((1, K), np.float32), "scores1": np.zeros((1, K), np.float32),
            "descriptors0": np.zeros((1, K, d), np.float32), "descriptors1": np.zeros((1, K, d), np.float32)}
    s = trainpairs.reference_sample(host, 0, img, img, "a.png", "cpu")
    assert sorted(s) == [str(k) for k in small["keys"]]

    def kind(v):
        if isinstance(v, list):
            return "list/" + type(v[0]).__name__ + "/" + str(getattr(v[0], "dtype", ""))
        return type(v).__name__ + "//" + str(getattr(v, "dtype", "")).replace("torch.", "")
    assert [kind(s[k]) for k in sorted(s)] == [str(t) for t in small["types"]]
    assert s["keypoints0"][0].shape == (n0, 2) and len(s["descriptors0"]) == d and s["descriptors1"][0].shape == (n1,)
    assert len(s["scores0"]) == n0 and s["matches"].shape == (2, 2) and s["all_matches"][0].shape == (6,) and s["image0"].shape == (1, 12, 16)


def test_corner_sampler_is_seeded_and_solves_its_four_points():
    from image_matching_amd import trainpairs
    a = trainpairs.sample_matrix(np.random.default_rng([3, 7]), (120, 160))
    assert np.array_equal(a, trainpairs.sample_matrix(np.random.default_rng([3, 7]), (120, 160))) and a.dtype == np.float64
    src = np.array([[0, 0], [0, 160], [120, 0], [120, 160]], np.float64)
    dst = src + [[5, -7], [-30, 12], [44, 9], [-3, -60]]
    M = trainpairs.four_point_matrix(src, dst)
    assert np.array_equal(M, R.four_point_matrix(src, dst))
    p = np.concatenate([src, np.ones((4, 1))], 1) @ M.T
    assert np.abs(p[:, :2] / p[:, 2:] - dst).max() < 1e-9
