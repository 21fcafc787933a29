"""Writes the soft-label fixtures of libimx_sploop.so from the REFERENCE itself (imported unchanged; never runs where the reference is
absent):

    python tests/golden/make_golden_sploop.py --reference /path/to/reference

  sploop_labels_<H>x<W>.npz     120 x 160 and 136 x 200 (odd number of cells across)

Each holds one batch of KCAP + 1 images, image b with b points (so every count from 0 to KCAP occurs): the matrices
(image_matching_amd.homoadapt.sample_homographies with the shipped yaml's warped_pair.params, on [-1,1]^2, and `mats_px`, what the
reference's homography_scaling_torch made of them where the fixture was written: that 3x3 product chain goes through the host's
matrix product, whose bits differ between processors, so the tests hand the kernel the recorded pixel-space matrices), the points (rows past an
image's count are zero), and the reference's own datasets/data_tools.py warpLabels(pnts, H, W, homography, bilinear=True): its
'labels_bi' (`warped_labels_bi`), its 'labels' (`warped_labels`), and 'labels_bi' pushed through the two quantisation lines of
ImgAugTransform.__call__ (utils/photometric.py:74, :76), `(img * 255).astype(np.uint8)` and `.astype(np.float32) / 255`
(`warped_labels_gaussian` where the blur between them is the identity).

imgaug cannot be imported on the machines of this project, so ImgAugTransform itself cannot run: the two quantisation lines are
RESTATED here in numpy (quantise below), and the GaussianBlur between them is left out -- datasets/ALLSS_train.py serves only a sigma at
which it is provably the identity on 8-bit images.

torch's CPU matrix product, through which the reference's warp_points (utils/utils.py:561-584) forms H @ (x, y, 1), takes a different
code path below 12 columns on this torch build: each row is then ((m0 x + m2) + m1 y) with every product rounded, where from 12
columns on it is fma(m2, 1, fma(m1, y, m0 x)) -- the order imx_warp_labels documents, the one that sptrain_*.npz pin and the one real
label files (hundreds of points an image) get.  A fixture whose images hold 0 .. KCAP points would pin both orders at once, by the
count alone.  So the name `warp_points` in datasets/data_tools.py's globals is wrapped (padded_warp_points below): a list shorter than
PAD_TO points is padded with copies of its first point, the reference's own warp_points runs on the padded list, and the padding rows
are cut off its result.  A column of the product depends on its own point alone, so this changes which path torch takes and nothing
else; the generator asserts that padding to PAD_TO and to 4 PAD_TO give the same bits.  Everything after the warp is the reference's
own code on the image's own points.

Stubs: cv2, torchvision and matplotlib as empty modules where they are absent (imported at module level by utils/utils.py, called by
nothing used here).

A seed decides a whole set: image b draws its points from numpy's Generator seeded by (seed, b) and its matrix from
sample_homographies(2, (seed, b)).  Seeds are taken in order from 1 and the first is kept for which THE REFERENCE'S OWN RESULT meets
every condition below, asserted again on the kept set:
  - no two kept entries (a corner of a point inside the image) of an image share a pixel, so torch's indexed assignment is defined;
  - no warped coordinate lies in (-1, 0), where the reference's cast to uint8 of a weight outside [0,1] is undefined;
  - some point's +1 corners leave the right border (trunc(x) = W - 1) and some point's the bottom border (trunc(y) = H - 1);
  - some point is warped outside the image altogether (none of its corners is kept).
Seeds tried when the committed fixtures were written: 28 for 120x160 (seed 28 kept), 41 for 136x200 (seed 41 kept); each fixture
records its own count as `seeds_tried`.  Most seeds passed over had a warped coordinate in (-1, 0) or no point on the right or bottom border."""
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
KCAP = 16
PAD_TO = 16                     # torch's product takes the documented (fused) order from 12 columns on


def quantise(img):
    """utils/photometric.py:74 and :76, restated (imgaug is not importable here): the 8-bit round trip of ImgAugTransform.__call__"""
    img = np.array(img)
    img = (img * 255).astype(np.uint8)
    return img.astype(np.float32) / 255


def load_reference(path):
    sys.path.insert(0, path)
    for name in ("cv2", "torchvision", "matplotlib"):
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["matplotlib"], "pyplot"):
        for sub in ("pyplot", "cm"):
            sys.modules["matplotlib." + sub] = types.ModuleType("matplotlib." + sub)
            setattr(sys.modules["matplotlib"], sub, sys.modules["matplotlib." + sub])
    import datasets.data_tools as DT                                               # noqa: E402  (the reference's)
    import utils.utils as U                                                        # noqa: E402
    own = U.warp_points

    def padded_warp_points(points, homographies, device='cpu', pad_to=PAD_TO):
        """the reference's warp_points on a list of at least pad_to points (see the module docstring); 2-D homographies only"""
        n = points.shape[0]
        if n == 0 or n >= pad_to:
            return own(points, homographies, device)
        return own(torch.cat((points, points[:1].expand(pad_to - n, 2))), homographies, device)[:n]
    DT.warp_points = padded_warp_points
    return DT, U


def build(ref, H, W, seed):
    """the fixture dict of one (size, seed), or a string: the condition the reference's result does not meet"""
    DT, U = ref
    from image_matching_amd.homoadapt import sample_homographies
    from tests import sptrain_ref as R
    B = KCAP + 1
    pts = np.zeros((B, KCAP, 2), np.float32)
    homs = np.zeros((B, 3, 3), np.float32)
    mats_px = np.zeros((B, 3, 3), np.float32)
    bi, lab = np.zeros((B, H, W), np.float32), np.zeros((B, H, W), np.uint8)
    right = bottom = outside = 0
    for b in range(B):
        rng = np.random.default_rng([seed, b])
        pts[b, :b] = np.stack([rng.random(b) * (W - 1), rng.random(b) * (H - 1)], 1).astype(np.float32)
        homs[b] = sample_homographies(2, [seed, b], **R.WARPED_PAIR_PARAMS)[0][1]
        mats_px[b] = DT.homography_scaling(torch.from_numpy(homs[b]), H, W).numpy()
        if b == 0:
            continue                                                   # (the reference cannot index with an empty point list; the map is zero)
        hom_t = torch.from_numpy(homs[b])
        out = DT.warpLabels(pts[b, :b], H, W, hom_t, bilinear=True)
        bi[b] = out["labels_bi"].numpy().reshape(H, W)
        lab[b] = out["labels"].numpy().reshape(H, W).astype(np.uint8)
        # ---- the conditions, on the reference's own warped points and corners
        wp = DT.warp_points(torch.from_numpy(pts[b, :b]).long(), DT.homography_scaling(hom_t, H, W)).reshape(-1, 2)
        wide = DT.warp_points(torch.from_numpy(pts[b, :b]).long(), DT.homography_scaling(hom_t, H, W), pad_to=4 * PAD_TO).reshape(-1, 2)
        assert torch.equal(wp, wide) or not bool(torch.isfinite(wp).all()), "the padded product depends on how far it is padded"
        if not bool(torch.isfinite(wp).all()):
            return "a non-finite warped point"
        if bool(((wp > -1) & (wp < 0)).any()):
            return "a warped coordinate in (-1, 0)"
        ext, _ = DT.extrapolate_points(wp)
        kept, mask = U.filter_points(ext, torch.tensor([W, H]), return_mask=True)
        flat = (kept[:, 1] * W + kept[:, 0]).long().numpy()
        if len(np.unique(flat)) != len(flat):
            return "two kept entries on one pixel"
        q = wp.long()
        right += int((q[:, 0] == W - 1).sum())
        bottom += int((q[:, 1] == H - 1).sum())
        outside += int((~mask.reshape(4, -1).any(0)).sum())
    if not (right and bottom and outside):
        return f"coverage: {right} points on the right border, {bottom} on the bottom border, {outside} outside"
    return {"seed": np.int64(seed), "size": np.array([H, W], np.int64), "pts": pts, "counts": np.arange(B, dtype=np.int32), "homographies": homs, "mats_px": mats_px,
            "labels_bi": bi, "labels_gaussian": quantise(bi), "labels": lab,
            "coverage": np.array([right, bottom, outside], np.int64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    ref = load_reference(a.reference)
    for H, W in SIZES:
        seed = 1
        while True:
            fx = build(ref, H, W, seed)
            if not isinstance(fx, str):
                break
            print(f"{H}x{W} seed {seed} passed over: {fx}")
            seed += 1
            assert seed < 1000, "no seed in 1..999 meets the conditions"
        assert sorted(fx["counts"].tolist()) == list(range(KCAP + 1))
        fx["seeds_tried"] = np.int64(seed)
        name = f"sploop_labels_{H}x{W}.npz"
        np.savez_compressed(os.path.join(HERE, name), **fx)
        size = os.path.getsize(os.path.join(HERE, name))
        assert size < (1 << 19), f"{name}: {size} bytes"
        print(f"{name}: {size} bytes, seed {seed} ({seed} tried), coverage (right, bottom, outside) {fx['coverage'].tolist()}, "
              f"{int((fx['labels_bi'] != 0).sum())} non-zero soft labels, {int(fx['labels'].sum())} hard labels")


if __name__ == "__main__":
    main()
