"""Writes the SuperGlue training-pair fixtures from the REFERENCE itself (imported unchanged; never runs where the reference is
absent):

    python tests/golden/make_golden_trainpairs.py --reference /path/to/reference

  trainpairs_small.npz    120 x 160, max_keypoints 256, three seeds of the whole pipeline (datasets/GlueSparse.py:24-104), the loss
                          of superglue/models/superglue_train.py:289-299 with the "t" weight set in fp32 and in float64
  trainpairs_ragged.npz   136 x 200, a keypoint threshold that leaves the two sides with different counts below the cap
  trainpairs_edge.npz     crafted keypoints through the reference's own lines 64-82 (its SuperPoint replaced by a callable)
with the descriptors of the first two in files of their own (<name>_desc.npz) so that every file stays below 1 MiB.

OpenCV is on no machine of this project: a stand-in `cv2` module goes into sys.modules whose five functions are the restatements
of tests/trainpairs_ref.py (the arithmetic of include/imx.h; parity with OpenCV itself is unpinned).  Everything
else -- the keypoints, cdist, the argmins, the set operations, the SuperGlue forward and its loss -- is the reference's own code.

A seed is refused when a decision of lines 67-74 is closer than 1e-6 to flipping (the gap between the smallest and second smallest
distance of any row or column, |row minimum - 3|): the tests may then demand exact index equality.  A seed is also refused when it
has too few matches to be worth keeping, or when the reference's own fp32 loss is not finite (an exp(Z) underflowed).  The tie cases of the edge file
are exempt: they sit on an integer lattice under the identity, where float64 is exact and numpy's argmin rule decides."""
import argparse
import copy
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import trainpairs_ref as R          # noqa: E402
from tests import util                         # noqa: E402
from image_matching_amd import hostops         # noqa: E402

D = 128
MARGIN = 1e-6


class Cv2StandIn(types.ModuleType):
    """the five OpenCV calls of datasets/GlueSparse.py; records what went through them"""

    def __init__(self):
        super().__init__("cv2")
        self.forced_M = None
        self.seen = {}

    def imread(self, path, flags=0):
        return np.load(path)

    def resize(self, img, size_wh):
        return hostops.resize_linear_u8(img, size_wh)

    def getPerspectiveTransform(self, src, dst):
        M = R.four_point_matrix(src, dst) if self.forced_M is None else np.asarray(self.forced_M, np.float64)
        self.seen["M"] = M
        return M

    def warpPerspective(self, src, M, dsize):
        assert tuple(dsize) == (src.shape[1], src.shape[0])
        out = R.warp_perspective_u8(src, R.invert3(M))
        self.seen["warped"] = out
        return out

    def perspectiveTransform(self, pts, M):
        out = R.project(pts.reshape(-1, 2), M).reshape(pts.shape)
        self.seen["proj"] = out.reshape(-1, 2)
        return out


def load_reference(path):
    sys.path.insert(0, path)
    cv2 = Cv2StandIn()
    sys.modules["cv2"] = cv2
    from datasets.GlueSparse import GlueSparse                         # noqa: E402  (the reference's)
    from superglue.models.superglue_train import SuperGlue             # noqa: E402
    return cv2, GlueSparse, SuperGlue


def image_u8(seed, H, W):
    return np.clip(np.rint(util.pair(seed, H, W)[0][0, 0].numpy().astype(np.float64) * 255.0), 0, 255).astype(np.uint8)


def dataset(GlueSparse, tmp, img, name, K, thr):
    d = os.path.join(tmp, name)
    os.makedirs(d)
    np.save(os.path.join(d, "image.npy"), img)
    ds = GlueSparse(d, util.sp_config(D, K, keypoint_threshold=thr), (img.shape[1], img.shape[0]), "cpu")
    ds.superpoint.load_state_dict(util.sp_sd(D))
    return ds


def describe(sample):
    """key -> 'container/element/dtype' of a __getitem__ dict, as strings"""
    def one(v):
        if isinstance(v, list):
            e = v[0] if v else None
            return "list/" + type(e).__name__ + "/" + str(getattr(e, "dtype", ""))
        return type(v).__name__ + "//" + str(getattr(v, "dtype", "")).replace("torch.", "")
    keys = sorted(sample)
    return np.array(keys), np.array([one(sample[k]) for k in keys])


def to_model_input(sample, dtype):
    """what the training loop hands the model (superpoint_glue_train.py:106-112) from a batch-1 DataLoader, on the host"""
    pred = torch.utils.data.default_collate([sample])
    for k in pred:
        if k not in ("file_name", "image0", "image1"):
            pred[k] = pred[k].to(dtype) if isinstance(pred[k], torch.Tensor) else torch.stack(pred[k])
    for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1", "scores0", "scores1"):
        pred[k] = pred[k].to(dtype)
    return pred


def check_margins(name, Dm, exempt=False):
    m = R.margins(Dm)
    low = {k: float(v.min()) for k, v in m.items()}
    if not exempt and min(low.values()) < MARGIN:
        return None
    return np.array([low["row_gap"], low["col_gap"], low["radius_gap"]])


def pipeline(cv2, GlueSparse, SuperGlue, name, H, W, K, thr, first_seed, min_matches, want=3):
    fx, desc, seeds = {}, {}, []
    sg = SuperGlue(util.sg_config(D)).eval()
    sg.load_state_dict(util.sg_sd(D, variant="t"))
    sg64 = copy.deepcopy(sg).double()
    sgd = SuperGlue(util.sg_config(D)).eval()
    sgd.load_state_dict(util.sg_sd(D))
    with tempfile.TemporaryDirectory() as tmp:
        seed = first_seed
        while len(seeds) < want:
            seed += 1
            img = image_u8(seed, H, W)
            ds = dataset(GlueSparse, tmp, img, f"{name}_{seed}", K, thr)
            cv2.forced_M, cv2.seen = None, {}
            np.random.seed(seed)
            with torch.no_grad():
                s = ds[0]
            if "matches" not in s:
                print(f"{name}: seed {seed} refused: a side has no keypoints")
                continue
            k0, k1 = s["keypoints0"][0], s["keypoints1"][0]
            n = s["matches"].shape[1]
            mg = check_margins(name, R.distances(cv2.seen["proj"], k1))
            if mg is None or n < min_matches or (thr > 0.005 and (len(k0) == len(k1) or max(len(k0), len(k1)) >= K)):
                print(f"{name}: seed {seed} refused: margins {mg}, {n} matches, counts {len(k0)} / {len(k1)}")
                continue
            with torch.no_grad():
                loss_t = sg(to_model_input(s, torch.float32))["loss"].numpy()
                loss_d = sgd(to_model_input(s, torch.float32))["loss"].numpy()
                loss_64 = sg64(to_model_input(s, torch.float64))["loss"].numpy()
            if not (np.isfinite(loss_t).all() and np.isfinite(loss_d).all()):
                # (an exp(Z) of the reference's own fp32 forward underflowed: its loss is +inf, which no tolerance can compare)
                print(f"{name}: seed {seed} refused: the reference's fp32 loss is {float(loss_t[0])} / {float(loss_d[0])}")
                continue
            i = len(seeds)
            seeds.append(seed)
            fx.update({f"image_{i}": img, f"M_{i}": cv2.seen["M"], f"warped_{i}": cv2.seen["warped"], f"kpts0_{i}": k0, f"kpts1_{i}": k1,
                       f"scores0_{i}": np.asarray(s["scores0"], np.float32), f"scores1_{i}": np.asarray(s["scores1"], np.float32),
                       f"proj_{i}": cv2.seen["proj"], f"matches_{i}": s["matches"].astype(np.int64),
                       f"all_matches_{i}": np.stack(s["all_matches"]).astype(np.int64), f"loss_t_{i}": loss_t.astype(np.float32),
                       f"loss_default_{i}": loss_d.astype(np.float32), f"loss_t_f64_{i}": loss_64.astype(np.float64), f"margins_{i}": mg,
                       f"boundary_{i}": R.warp_boundary_pixels(R.invert3(cv2.seen["M"]), H, W)})
            assert len(fx[f"boundary_{i}"]) <= 1e-4 * H * W, f"{name}: seed {seed}: {len(fx[f'boundary_{i}'])} pixels on a rounding boundary"
            desc.update({f"desc0_{i}": np.stack(s["descriptors0"]).astype(np.float32), f"desc1_{i}": np.stack(s["descriptors1"]).astype(np.float32)})
            fx["keys"], fx["types"] = describe(s)
            print(f"{name}: seed {seed}: counts {len(k0)} / {len(k1)}, {n} matches among {fx[f'all_matches_{i}'].shape[1]} columns, loss t {float(loss_t[0]):.4f} "
                  f"(f64 {float(loss_64[0]):.6f}) default {float(loss_d[0]):.4f}; margins {mg}; {len(fx[f'boundary_{i}'])} boundary pixels")
    fx["seeds"], fx["cap"], fx["keypoint_threshold"] = np.array(seeds, np.int64), np.int64(K), np.float64(thr)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **fx)
    np.savez_compressed(os.path.join(HERE, name + "_desc.npz"), **desc)


def edge_cases():
    """name -> (keypoints of side 0, keypoints of side 1, forward matrix, exempt from the margin rule)"""
    rng = np.random.default_rng(5)
    eye = np.eye(3)
    grid = np.stack(np.meshgrid(np.arange(8) * 17.0 + 9, np.arange(5) * 19.0 + 11), -1).reshape(-1, 2).astype(np.float32)     # 40 points
    out = {"none": (grid[:12], grid[:9] + np.float32(7.25), eye, False),
           "all": (grid, grid[rng.permutation(len(grid))], eye, False)}
    # two points of side 0 next to one point of side 1 (the nearer one takes it); another such pair the other way round
    out["two_to_one"] = (np.array([[30, 30], [31.5, 30], [80, 60], [120, 90]], np.float32),
                         np.array([[30.5, 30.25], [80.25, 60.5], [81, 59.25], [140, 20]], np.float32), eye, False)
    # distances of 2.999 and 3.001 (and the same through a translation)
    out["radius"] = (np.array([[20, 20], [60, 20], [20, 70], [60, 70]], np.float32),
                     np.array([[22.999, 20], [63.001, 20], [20, 72.999], [60, 73.001]], np.float32), eye, False)
    shift = np.array([[1, 0, 4.5], [0, 1, -2.25], [0, 0, 1.0]])
    out["radius_shift"] = (out["radius"][0], out["radius"][1] + np.array([4.5, -2.25], np.float32), shift, False)
    out["one_0"] = (grid[17:18] + np.float32(1.25), grid[10:30], eye, False)
    out["one_1"] = (grid[10:30], grid[17:18] + np.float32(1.25), eye, False)
    out["one_one_far"] = (grid[:1], grid[5:6], eye, False)
    # a projective matrix on scattered points: the projection's division
    persp = R.four_point_matrix([[0, 0], [0, 160], [120, 0], [120, 160]], [[9, -7], [-12, 150], [131, 11], [110, 171]])
    p0 = (rng.random((67, 2)) * [150, 110] + 5).astype(np.float32)
    moved = R.project(p0, persp)[rng.permutation(67)][:40] + (rng.random((40, 2)).astype(np.float32) * 4 - 2)
    out["perspective"] = (p0, moved.astype(np.float32), persp, False)
    # exact ties on an integer lattice under the identity: the lowest index wins
    out["ties"] = (np.array([[10, 10], [12, 10], [40, 40], [41, 41], [70, 20], [70, 22], [100, 50]], np.float32),
                   np.array([[11, 10], [9, 10], [10, 11], [40, 41], [41, 40], [70, 21], [102, 50], [98, 50], [100, 52]], np.float32), eye, True)
    return out


def edge(cv2, GlueSparse):
    fx = {}
    img = image_u8(3, 120, 160)
    with tempfile.TemporaryDirectory() as tmp:
        ds = dataset(GlueSparse, tmp, img, "edge", 256, 0.005)
        for name, (k0, k1, M, exempt) in edge_cases().items():
            feed = iter([k0, k1])

            def fake_superpoint(x, feed=feed):
                k = torch.from_numpy(np.ascontiguousarray(next(feed), np.float32))
                return {"keypoints": [k], "scores": [torch.zeros(len(k))], "descriptors": [torch.zeros(2, len(k))]}
            ds.superpoint = fake_superpoint
            cv2.forced_M, cv2.seen = M, {}
            s = ds[0]
            mg = check_margins(name, R.distances(cv2.seen["proj"], k1), exempt)
            assert mg is not None, f"edge case {name}: a decision is within {MARGIN} of flipping"
            fx.update({f"kpts0_{name}": k0, f"kpts1_{name}": k1, f"M_{name}": np.asarray(M, np.float64), f"proj_{name}": cv2.seen["proj"],
                       f"matches_{name}": s["matches"].astype(np.int64), f"all_matches_{name}": np.stack(s["all_matches"]).astype(np.int64),
                       f"margins_{name}": mg})
            print(f"edge {name}: counts {len(k0)} / {len(k1)}, {s['matches'].shape[1]} matches, margins {mg}")
        # the skip sample (:52-61): one side without keypoints
        feed = iter([np.zeros((0, 2), np.float32), edge_cases()["all"][1]])
        ds.superpoint = lambda x: {"keypoints": [torch.from_numpy(next(feed))], "scores": [torch.zeros(0)], "descriptors": [torch.zeros(2, 0)]}
        cv2.forced_M = None
        s = ds[0]
        fx["skip_keys"], fx["skip_types"] = describe(s)
        for k in ("keypoints0", "keypoints1", "descriptors0", "descriptors1"):
            fx["skip_shape_" + k] = np.array(s[k].shape, np.int64)
    fx["names"] = np.array(list(edge_cases()))
    np.savez_compressed(os.path.join(HERE, "trainpairs_edge.npz"), **fx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    cv2, GlueSparse, SuperGlue = load_reference(a.reference)
    pipeline(cv2, GlueSparse, SuperGlue, "trainpairs_small", 120, 160, 256, 0.005, 0, 20)
    pipeline(cv2, GlueSparse, SuperGlue, "trainpairs_ragged", 136, 200, 256, 0.13, 100, 10)
    edge(cv2, GlueSparse)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("trainpairs_"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < (1 << 20), f"{f}: {size} bytes"
            print(f, size)


if __name__ == "__main__":
    main()
