"""superpoint_glue_register.py --transform homography on the GPU: the registration CLI with the RANSAC homography fit
(imx_estimate_homography) and the perspective warp (imx_warp_perspective_u8) in place of the 4-DoF similarity.  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def grad_enabled():
    """(importing the script switches autograd off for the whole process: put it back for the modules that run after this one)"""
    yield
    torch.set_grad_enabled(True)


def test_cli_homography_on_synthetic_dataset(tmp_path):
    """--synthetic 2 --transform homography writes both transforms, and the fitted matrix reproduces the planted shift of the synthetic
    sources -- source i is the template rolled by (8, 16) (i + 1) px (rows, columns) at the network's resolution -- within the fit's
    threshold at the four corners, measured at the network's resolution"""
    import superpoint_glue_register as cli
    scale = 0.5
    img_dir, res_dir = str(tmp_path / "data") + "/", str(tmp_path / "out") + "/"
    res = cli.main(["--img_dir", img_dir, "--Result_dir", res_dir, "--synthetic", "2", "--resize_scale", str(scale), "--max_keypoints", "512",
                    "--exper_name", "h", "--transform", "homography"])
    assert sorted(os.listdir(os.path.join(res_dir, "h", "Transform"))) == ["trans_src_000.png", "trans_src_001.png"]
    assert sorted(os.listdir(os.path.join(res_dir, "h", "Match"))) == ["src_000.png", "src_001.png"]
    W, H = int(round(640 / scale)), int(round(480 / scale))                 # the original images
    corners = np.array([[0, 0, 1], [W - 1, 0, 1], [W - 1, H - 1, 1], [0, H - 1, 1]], np.float64).T
    for i, r in enumerate(res):
        M = r[5]
        assert M is not None and M.shape == (3, 3) and r[4] >= 4, r[:5]
        dy, dx = int(8 / scale) * (i + 1), int(16 / scale) * (i + 1)        # source = roll(template): source (x, y) is template (x - dx, y - dy)
        p = M @ corners
        err = np.sqrt((p[0] / p[2] - (corners[0] - dx)) ** 2 + (p[1] / p[2] - (corners[1] - dy)) ** 2) * scale
        print(f"pair {i}: {r[3]} matches, {r[4]} inliers, corner errors at the network's resolution {err.round(3).tolist()} px")
        assert err.max() <= cli.HOMOGRAPHY_THRESH, err


def test_cli_similarity_is_the_registration_script_itself(tmp_path):
    """--transform similarity (the default) hands over to superpoint_glue_test.run_registration: the same matrices as that script's own
    main on the same synthetic dataset; and the official models run through the homography path too"""
    import superpoint_glue_test as base
    import superpoint_glue_register as cli
    img_dir = str(tmp_path / "data") + "/"
    common = ["--img_dir", img_dir, "--synthetic", "2", "--resize_scale", "0.5", "--max_keypoints", "512"]
    mine = cli.main(common + ["--Result_dir", str(tmp_path / "a") + "/", "--exper_name", "s"])
    theirs = base.main(common + ["--Result_dir", str(tmp_path / "b") + "/", "--exper_name", "s"])
    assert [r[:5] for r in mine] == [r[:5] for r in theirs] and all(np.array_equal(a[5], b[5]) for a, b in zip(mine, theirs))
    assert sorted(os.listdir(tmp_path / "a" / "s" / "Transform")) == sorted(os.listdir(tmp_path / "b" / "s" / "Transform"))
    res = cli.main(common + ["--Result_dir", str(tmp_path / "c") + "/", "--exper_name", "o", "--models", "official", "--transform", "homography"])
    assert [r[0] for r in res] == ["src_000.png", "src_001.png"] and all(r[1] == 512 and r[2] == 512 for r in res)
    assert sorted(os.listdir(tmp_path / "c" / "o" / "Match")) == ["src_000.png", "src_001.png"]


def test_homography_helper_falls_back_like_the_similarity_helper():
    import superpoint_glue_register as cli
    from image_matching_amd.engine import Engine
    from tests import util
    eng = Engine(util.sp_config(128, 64), util.sg_config(128), "cuda")
    pred = {"matches0": torch.full((1, 64), -1, dtype=torch.int64, device="cuda"), "keypoints0": [torch.zeros(64, 2, device="cuda")],
            "keypoints1": [torch.zeros(64, 2, device="cuda")]}
    assert cli.gpu_homography(eng, pred, 3.0) == (None, None)                 # at most 3 matches: the caller's host fit
    # a planted shift: the helper returns it with every match an inlier
    k0 = torch.rand(64, 2, device="cuda") * 300
    pred = {"matches0": torch.arange(64, device="cuda")[None], "keypoints0": [k0], "keypoints1": [k0 + torch.tensor([5.0, -3.0], device="cuda")]}
    Hm, mask = cli.gpu_homography(eng, pred, 3.0)
    assert mask.shape == (64, 1) and mask.all()
    np.testing.assert_allclose(Hm, [[1, 0, 5], [0, 1, -3], [0, 0, 1]], atol=1e-3)
