"""Homographic adaptation, host side (no GPU): the CPU restatement the GPU tests lean on (tests/homoadapt_ref.py) reproduces
the fixtures the reference itself wrote (tests/golden/make_golden_homoadapt.py); the sampler; the ABI surface; the CLI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import homoadapt_ref as R
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("imx_warp_homography", "imx_combine_heatmap", "imx_superpoint_heatmap", "imx_homography_adapt", "imx_heatmap_points")


def fixture(name):
    g = util.golden(name + ".npz")
    g["warped"] = util.golden(name + "_warped.npz")["warped"]
    g["heat"] = util.golden(name + "_heat.npz")["heat"]
    return g


def image(g):
    H, W = (int(v) for v in g["size"])
    return util.pair(int(g["seed"]), H, W)[0][0, 0]


@pytest.mark.parametrize("name", ["homoadapt_small", "homoadapt_ragged"])
def test_restatement_reproduces_the_reference(name):
    g = fixture(name)
    H, W = (int(v) for v in g["size"])
    hom, inv = g["homographies"], g["inv_homographies"]
    warped = R.warp(image(g), inv).numpy()
    assert np.array_equal(warped, g["warped"]), "warped images"
    assert np.array_equal(R.valid_mask(inv, H, W).numpy(), g["mask"].astype(np.float32)), "valid masks"
    comb, cnt = R.combine(g["heat"], g["mask"].astype(np.float32), hom)
    util.assert_close(cnt, g["count"], "count map")
    ok = ~np.isnan(g["combined"])
    assert np.array_equal(np.isnan(comb.numpy()), ~ok), "NaN pattern of the combined map"
    util.assert_close(comb.numpy()[ok], g["combined"][ok], "combined map")
    for key in (k for k in g if k.startswith("pts_")):
        _, thr, nms = key.split("_")
        mine = R.points(g["combined"], float(thr), int(nms))
        assert R.rows_equal_up_to_ties(mine.T, g[key].T), key


def test_restatement_heatmap_is_the_fixture_heatmap():
    """flattenDetection through the oracle's network on the fixture's warped images (fp32 CPU)."""
    from oracle import superpoint_ref
    g = fixture("homoadapt_small")
    sd = util.sp_sd(128)
    with torch.no_grad():
        semi, _ = superpoint_ref.heads_bn(superpoint_ref.encoder_bn(torch.from_numpy(g["warped"])[:, None], sd), sd)
    util.assert_close(R.flatten_detection(semi).numpy(), g["heat"], "heatmaps")
    assert torch.equal(R.flatten_detection(semi), superpoint_ref.score_map(semi))


@pytest.mark.parametrize("name", ["homoadapt_small", "homoadapt_ragged"])
def test_float64_stacks(name):
    """The fixtures' float64 evaluations of the two stacks (float32 differences): the restatement's float64 warp reproduces the
    warped one, and the reference's own fp32 results sit within the project tolerance of both."""
    g = fixture(name)
    w64 = g["warped"].astype(np.float64) + util.golden(name + "_warped_d64.npz")["warped_d64"]
    h64 = g["heat"].astype(np.float64) + util.golden(name + "_heat_d64.npz")["heat_d64"]
    mine = R.warp(image(g).double(), g["inv_homographies"], "bilinear", torch.float64).numpy()
    assert np.abs(mine - w64).max() <= 1e-7          # (stored as a float32 difference: ~1e-12 here)
    util.assert_close(g["warped"], w64, "reference fp32 warp vs float64")
    util.assert_close(g["heat"], h64, "reference fp32 heatmaps vs float64")


def test_missing_checkpoint_is_an_error(tmp_path):
    from image_matching_amd.superpoint.models.model_wrap import SuperPointFrontend_torch
    cfg = {"model": {"name": "superpoint_train", "params": {"descriptor_length": 128}, "subpixel": {"enable": False}}}
    with pytest.raises(FileNotFoundError):
        SuperPointFrontend_torch(config=cfg, weights_path=str(tmp_path / "absent.pth.tar"), nms_dist=4, conf_thresh=0.015, nn_thresh=0.7)
    (tmp_path / "pointer.pth.tar").write_text("version https://git-lfs.github.com/spec/v1\n")
    with pytest.raises(FileNotFoundError):
        SuperPointFrontend_torch(config=cfg, weights_path=str(tmp_path / "pointer.pth.tar"), nms_dist=4, conf_thresh=0.015, nn_thresh=0.7)
    fe = SuperPointFrontend_torch(config=cfg, weights_path=None, nms_dist=4, conf_thresh=0.015, nn_thresh=0.7)     # asked for: fine
    assert fe.net is not None


def test_restatement_points_on_the_stress_maps():
    st = util.golden("homoadapt_stress.npz")
    for key in (k for k in st if k.startswith("map_")):
        for nms in (4, 1):
            ref = st[f"pts_{key[4:]}_{nms}"]
            mine = R.points(st[key], 0.015, nms)
            assert mine.shape == ref.shape and R.rows_equal_up_to_ties(mine.T, ref.T), (key, nms)
    assert st["pts_chain_4"].shape[1] >= 30 and st["pts_empty_4"].shape[1] == 0 and st["pts_one_4"].shape[1] == 1


def test_subpixel_restatement_is_the_patch_centroid():
    h = np.zeros((20, 24))
    h[10, 12], h[10, 13], h[9, 12] = 2.0, 1.0, 1.0
    out = R.subpixel(h, np.array([[12.], [10.], [2.]]))
    assert np.allclose(out[:, 0], [12.25, 9.75, 2.0])


def test_sample_homographies():
    from image_matching_amd import homoadapt as HA
    a, ai = HA.sample_homographies(12, 5, **HA.EXPORT_PARAMS)
    b, bi = HA.sample_homographies(12, 5, **HA.EXPORT_PARAMS)
    c, _ = HA.sample_homographies(12, 6, **HA.EXPORT_PARAMS)
    assert a.dtype == ai.dtype == np.float32 and a.shape == ai.shape == (12, 3, 3)
    assert np.array_equal(a, b) and np.array_equal(ai, bi) and not np.array_equal(a, c)
    assert np.array_equal(a[0], np.eye(3, dtype=np.float32))
    for m, mi in zip(a, ai):
        assert abs(np.linalg.det(m.astype(np.float64))) > 1e-3
        assert np.abs(m.astype(np.float64) @ mi.astype(np.float64) - np.eye(3)).max() < 1e-5
    # without artifacts every sampled patch stays inside the unit square (the bound utils/homographies.py:77,102 enforces)
    rng = np.random.default_rng(0)
    for _ in range(50):
        q = HA.sample_patch_corners(rng, scaling_amplitude=0.2, perspective_amplitude_x=0.2, perspective_amplitude_y=0.2, patch_ratio=0.85)
        assert (q >= -1e-12).all() and (q <= 1 + 1e-12).all()
    # the matrix maps the corners of [-1,1]^2 onto the patch it was built from
    m = HA.four_point_transform([[-1, -1], [-1, 1], [1, 1], [1, -1]], [[-.5, -.6], [-.4, .7], [.9, .8], [.6, -.7]])
    p = m @ np.array([1., 1., 1.])
    assert np.allclose(p[:2] / p[2], [.9, .8])


def test_abi_declares_the_entry_points():
    """Fails before the feature: the header, the bindings and the library all lack them."""
    from image_matching_amd import _lib
    header = open(os.path.join(ROOT, "include", "imx.h")).read()
    for name in ENTRIES:
        assert re.search(r"^IMX_API int " + name + r"\(", header, re.M), name + " not declared"
        assert name in _lib.EXPORTS, name + " not in _lib.EXPORTS"
    from image_matching_amd.engine import Engine
    for m in ("warp_homography", "combine_heatmap", "superpoint_heatmap", "homography_adapt", "heatmap_points"):
        assert callable(getattr(Engine, m, None)), m


def test_python_surface_signatures():
    import inspect
    from image_matching_amd.utils import utils as U
    from image_matching_amd.superpoint.models.model_wrap import SuperPointFrontend_torch as FE
    want = {"inv_warp_image_batch": ["img", "mat_homo_inv", "device", "mode"], "inv_warp_image": ["img", "mat_homo_inv", "device", "mode"],
            "compute_valid_mask": ["image_shape", "inv_homography", "device", "erosion_radius"],
            "combine_heatmap": ["heatmap", "inv_homographies", "mask_2D", "device"], "getPtsFromHeatmap": ["heatmap", "conf_thresh", "nms_dist"]}
    for fn, args in want.items():
        assert list(inspect.signature(getattr(U, fn)).parameters) == args, fn
    assert list(inspect.signature(FE.__init__).parameters)[1:] == ["config", "weights_path", "nms_dist", "conf_thresh", "nn_thresh", "cuda", "trained", "device", "grad", "load"]
    assert list(inspect.signature(FE.run).parameters)[1:] == ["inp", "onlyHeatmap", "train"]
    with pytest.raises(NotImplementedError):
        U.compute_valid_mask((8, 8), torch.eye(3), erosion_radius=2)


def test_cli_flags_equal_the_reference():
    """superpoint_export_pseudo.py:21-28 (typed in here, like test_host.py does for the matching CLIs)."""
    sys.path.insert(0, ROOT)
    import superpoint_export_pseudo as cli
    ref = {"command": "export_detector_homoAdapt", "config": "superpoint/configs/magicpoint_allss_export.yaml",
           "exper_name": "magicpoint_synth_homoAdapt_allss_50_[640,480]", "export_task": "train", "save_output": "Results/ALLSS",
           "eval": False, "outputImg": True, "debug": False}
    a = vars(cli.build_parser().parse_args([]))
    for k, v in ref.items():
        assert a[k] == v, k
    assert set(a) - set(ref) == {"synthetic"} and a["synthetic"] == 0
