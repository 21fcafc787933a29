"""Writes the SuperPoint-descriptor-training fixtures from the REFERENCE itself (imported unchanged; never runs where the
reference is absent):

    python tests/golden/make_golden_sptrain.py --reference /path/to/reference

  sptrain_<H>x<W>_s<seed>.npz   120 x 160 (15 x 20 cells) and 136 x 200 (17 x 25 cells, odd width), two seeds each

Each holds one warped pair: the matrices (image_matching_amd.homoadapt.sample_homographies with the shipped yaml's
warped_pair.params), points, the reference's label / residual maps (datasets/data_tools.py warpLabels, ALLSS.points_to_2D) and valid
mask, the reference network's `semi` for both images, its detector losses (Train_model_heatmap.detector_loss on labels2Dto3D /
getMasks) in fp32 and float64, and descriptor_loss_sparse for d in {64, 128, 256} x method in {1d, 2d} x four (M, R) settings, in
fp32 and float64, next to what the seeded reference DREW: crop_or_pad_choice and create_non_correspondences are wrapped so that they
record their results, which are the kernel's inputs.  The descriptor maps are unit-norm normal draws of numpy's Generator seeded by
(seed, d, side): the tests regenerate them (desc_maps below).

Stubs: cv2 and torchvision as empty modules (imported at module level, called by nothing used here), nn.Module.cuda as the identity.
descriptor_loss_sparse indexes with a list of 0-d tensors (:130-131), which this torch refuses: the name `list` in that module's
globals is shadowed with torch.as_tensor and the reference's own body runs.  In float64 with method '2d' grid_sample is handed a
float32 grid and a float64 map: the grid is cast to the map's type on the way in.

Seeds are taken in order, never searched.  A seed is REFUSED (printed, recorded in the fixture that follows it) when a decision is
closer to flipping than an FMA-contracted and an uncontracted fp32 evaluation can differ:
  - a warped coordinate (labels: pixels, descriptor loss: cells) within 16 fp32 spacings at the coordinate's magnitude bound of a
    rounding boundary or a filter_points edge;
  - a non-match product within 1e-5 of the margin 0.2 (any d, any setting).
At most a quarter of consecutive seeds may be refused."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SIZES = ((120, 160), (136, 200))
DIMS = (64, 128, 256)
SETTINGS = ((64, 100), (100, 10), (512, 8), (100, 1))        # (M, R): a whole wave / a partial wave / padding with repeats
N_SEEDS, K_PTS, LAMDA_D, MARGIN = 2, 150, 250., 0.2


def desc_maps(seed, d, Hc, Wc):
    """the two (d,Hc,Wc) unit-norm descriptor maps of a fixture (the tests call this too)"""
    out = []
    for side in (0, 1):
        x = np.random.default_rng([seed, d, side]).standard_normal((d, Hc, Wc))
        out.append((x / np.sqrt((x * x).sum(0, keepdims=True))).astype(np.float32))
    return out


def load_reference(path):
    sys.path.insert(0, path)
    for name in ("cv2", "torchvision"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision.transforms", sys.modules["torchvision"].transforms)
    torch.nn.Module.cuda = lambda self, *a, **k: self
    import utils.utils as U                                                        # noqa: E402  (the reference's)
    import datasets.data_tools as DT                                               # noqa: E402
    import superpoint.loss_functions.sparse_loss as SL                             # noqa: E402
    from superpoint.models.superpoint_train import SuperPoint                     # noqa: E402
    from superpoint.Train_model_heatmap import Train_model_heatmap as TM          # noqa: E402
    SL.__dict__["list"] = torch.as_tensor
    return U, DT, SL, SuperPoint, TM


def spacing_margin(bound):
    return 16 * float(np.spacing(np.float32(bound / 2)))      # 16 spacings at the magnitude bound (|x| < bound)


def near_decision(c, size, margin):
    """any coordinate within `margin` of a rounding boundary (k + 0.5) or of a filter edge (0, size - 1, and -0.5 / size - 0.5 after round)"""
    c = np.asarray(c, np.float64)
    c = c[np.isfinite(c) & (c > -2) & (c < size + 1)]
    frac = np.abs(c - np.floor(c) - 0.5)
    return bool((frac < margin).any() or (np.abs(c) < margin).any() or (np.abs(c - (size - 1)) < margin).any())


def build(ref, H, W, seed):
    """the fixture dict of one (size, seed), or a string: why the seed is refused"""
    U, DT, SL, SuperPoint, TM = ref
    from image_matching_amd.homoadapt import sample_homographies
    from tests import sptrain_ref as R
    from tests import util
    Hc, Wc = H // 8, W // 8
    hom, inv = (m[1] for m in sample_homographies(2, seed, **R.WARPED_PAIR_PARAMS))
    hom_t, inv_t = torch.from_numpy(hom), torch.from_numpy(inv)
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.random(K_PTS) * (W - 1), rng.random(K_PTS) * (H - 1)], 1).astype(np.float32)
    pts[1] = np.trunc(pts[0]) + np.float32(0.25)                                           # two points on one pixel
    fx = {"seed": np.int64(seed), "size": np.array([H, W], np.int64), "homography": hom, "inv_homography": inv, "pts": pts}
    # ---- labels: the reference's warpLabels, and the refusal test on its own warped points
    ws = DT.warpLabels(pts, H, W, hom_t)
    raw = U.warp_points(torch.from_numpy(pts).long(), DT.homography_scaling(hom_t, H, W)).numpy()
    if near_decision(raw[:, 0], W, spacing_margin(256)) or near_decision(raw[:, 1], H, spacing_margin(256)):
        return "a warped label point near a rounding boundary or an image edge"
    labels = np.zeros((H, W))
    labels[pts.astype(int)[:, 1], pts.astype(int)[:, 0]] = 1                       # (ALLSS.points_to_2D needs OpenCV's module to import)
    fx["labels"] = labels.astype(np.uint8)
    fx["warped_labels"] = ws["labels"].numpy().reshape(H, W).astype(np.uint8)
    fx["warped_pnts"] = ws["warped_pnts"].numpy()
    res = ws["res"].transpose(1, 2).transpose(0, 1).numpy()                        # ALLSS.py:226
    fx["warped_res_support"] = (np.abs(res).sum(0) != 0).astype(np.uint8)
    fx["warped_res"] = res[:, fx["warped_labels"] == 1]                            # (2, n) in row-major pixel order
    mask = U.compute_valid_mask(torch.tensor([H, W]), inv_homography=inv_t, erosion_radius=0)[0]
    fx["warped_valid_mask"] = mask.numpy().astype(np.uint8)
    # ---- detector loss on the reference network's semi (synthetic weights, d = 128)
    img = util.pair(seed, H, W)[0][0, 0]
    net = SuperPoint(128).eval()
    net.load_state_dict(util.sp_sd(128))
    with torch.no_grad():
        warped = U.inv_warp_image(img, inv_t, mode="bilinear")
        x = torch.stack([img, warped])[:, None]
        semi = net(x)["semi"]
        gaps = (semi.max(1, keepdim=True).values - semi).numpy()
        assert not ((gaps > 80) & (gaps < 110)).any(), "a logit gap where the reference's fp32 leaves its float64 value"
        lab2 = torch.stack([torch.from_numpy(labels).float(), ws["labels"].reshape(H, W)])[:, None]
        msk2 = torch.stack([torch.ones(H, W), mask])[:, None]
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            t3 = U.labels2Dto3D(lab2.to(dt), 8, add_dustbin=True)
            m3 = torch.prod(U.labels2Dto3D(msk2.to(dt), 8, add_dustbin=False), 1)  # getMasks (Train_model_frontend.py:362-377)
            fx["det_loss_" + tag] = np.array([float(TM.detector_loss(None, semi[i:i + 1].to(dt), t3[i:i + 1], m3[i:i + 1], "softmax")) for i in (0, 1)]
                                             + [float(TM.detector_loss(None, semi.to(dt), t3, m3, "softmax"))], np.float64)
        fx["det_mask_sum"] = np.array([float(m3[0].sum()), float(m3[1].sum())])
    fx["semi"] = semi.numpy()
    # ---- sparse descriptor loss
    hc = SL.scale_homography_torch(hom_t, (Hc, Wc), shift=(-1, -1))
    cells = SL.get_coor_cells(Hc, Wc, 8, uv=True)
    wc = U.warp_points(cells, hc).numpy()
    if near_decision(wc[:, 0], Wc, spacing_margin(32)) or near_decision(wc[:, 1], Hc, spacing_margin(32)):
        return "a warped cell near a rounding boundary or a filter_points edge"
    uvb, keep = U.filter_points(torch.from_numpy(wc).round(), torch.tensor([Wc, Hc]), return_mask=True)     # sparse_loss.py:121-124
    pa = torch.nonzero(keep)[:, 0].numpy().astype(np.int32)
    pb = (uvb[:, 0] + uvb[:, 1] * Wc).long().numpy().astype(np.int32)
    fx["pair_a"], fx["pair_b"], fx["n_valid"] = pa, pb, np.int64(len(pa))
    drawn = {}
    crop, nonc, gs = SL.crop_or_pad_choice, SL.correspondence_finder.create_non_correspondences, torch.nn.functional.grid_sample

    def rec_crop(*a, **k):
        drawn["choice"] = np.asarray(crop(*a, **k))
        return drawn["choice"]

    def rec_nonc(*a, **k):
        drawn["non"] = nonc(*a, **k)
        return drawn["non"]
    SL.crop_or_pad_choice, SL.correspondence_finder.create_non_correspondences = rec_crop, rec_nonc
    torch.nn.functional.grid_sample = lambda inp, grid, **k: gs(inp, grid.to(inp.dtype), **k)
    try:
        for si, (M, R_) in enumerate(SETTINGS):
            for d in DIMS:
                da, db = (torch.from_numpy(m) for m in desc_maps(seed, d, Hc, Wc))
                for method in ("1d", "2d"):
                    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
                        np.random.seed(seed * 100 + si)
                        torch.manual_seed(seed * 100 + si)
                        out = SL.descriptor_loss_sparse(da.to(dt), db.to(dt), hom_t, device="cpu", lamda_d=LAMDA_D, num_matching_attempts=M,
                                                        num_masked_non_matches_per_match=R_, dist="cos", method=method)
                        choice = drawn["choice"].astype(np.int32)
                        non = (drawn["non"][0] + drawn["non"][1] * Wc).long().numpy().astype(np.int32)      # tuple_to_1d, then .long()
                        assert non.shape == (M, R_) and non.min() >= 0 and non.max() < Hc * Wc
                        if f"choice_{si}" in fx:
                            assert np.array_equal(fx[f"choice_{si}"], choice) and np.array_equal(fx[f"nonmatch_{si}"], non), "the draws moved"
                        fx[f"choice_{si}"], fx[f"nonmatch_{si}"] = choice, non.astype(np.int16)
                        fx[f"loss_{si}_{d}_{method}_{tag}"] = np.array([float(v) for v in out], np.float64)
                    # the reference's count of hard negatives, and the margin refusal, on the restatement's products
                    l64 = R.desc_loss(da, db, pa, pb, choice, non, LAMDA_D, MARGIN, method, torch.float64)
                    if (np.abs(l64[4] - MARGIN) < 1e-5).any():
                        return f"a non-match product within 1e-5 of the margin (d = {d}, M = {M}, R = {R_})"
                    fx[f"hard_{si}_{d}"] = np.int64(l64[3])
    finally:
        SL.crop_or_pad_choice, SL.correspondence_finder.create_non_correspondences, torch.nn.functional.grid_sample = crop, nonc, gs
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    ref = load_reference(a.reference)
    tried = refused_total = 0
    for H, W in SIZES:
        seed, kept, refused = 1, 0, []
        while kept < N_SEEDS:
            fx = build(ref, H, W, seed)
            tried += 1
            if isinstance(fx, str):
                print(f"{H}x{W} seed {seed} REFUSED: {fx}")
                refused.append(seed)
                refused_total += 1
            else:
                fx["refused_seeds"] = np.array(refused, np.int64)
                name = f"sptrain_{H}x{W}_s{seed}.npz"
                np.savez_compressed(os.path.join(HERE, name), **fx)
                size = os.path.getsize(os.path.join(HERE, name))
                assert size < (1 << 19), f"{name}: {size} bytes"
                print(f"{name}: {size} bytes, n_valid {int(fx['n_valid'])}, {int(fx['warped_labels'].sum())} warped labels, det loss {fx['det_loss_f32']}, "
                      f"|f32 - f64| / (1e-4 + 1e-4 |f64|) {np.abs(fx['det_loss_f32'] - fx['det_loss_f64']) / (1e-4 + 1e-4 * np.abs(fx['det_loss_f64']))}")
                kept, refused = kept + 1, []
            seed += 1
    assert 4 * refused_total <= tried, f"{refused_total} of {tried} consecutive seeds refused: more than a quarter"


if __name__ == "__main__":
    main()
