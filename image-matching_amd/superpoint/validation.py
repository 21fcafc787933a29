"""What a SuperPoint checkpoint does once it is DEPLOYED, measured on the GPU under known warps: the SuperPoint paper's detector
repeatability and localisation error, matching score, and homography-estimation correctness.

`SuperPointValidator` owns an inference Engine of its own.  evaluate(state_dict) loads the state dict the way the inference classes do
(Engine.load_state_dict: BatchNorm folded from the RUNNING statistics), then runs NMS, threshold and top-k on `image` and `warped_img`
of the first `pairs` samples of the dataset, matches the descriptors by mutual nearest neighbour (libimx_speval.so), counts what
repeats and which matches are correct under the known warp, fits a homography to the matches by RANSAC and takes its corner error.
Everything is accumulated on the device; ONE row is read back per evaluate().

Differences from the paper's protocol: the keypoints are the top-k of the whole image, not re-selected inside the shared view, and no
nearest-neighbour mAP is computed."""
import torch

from .. import _lib as L
from ..engine import Engine

SCALARS = ("val_repeatability", "val_localization_error", "val_keypoints", "val_matching_score", "val_match_precision",
           "val_corner_error_median", "val_homography_correct_1", "val_homography_correct_3", "val_homography_correct_5")
MAX_KEYPOINTS = 4096          # imx_keypoint_pair_metrics stages both sides in LDS


def reduce_rows(counts, sums, err, nkpts):
    """The nine scalars from the per-pair parts, on whatever device they live: counts (P,8) [v0, v1, r0, r1, m, c, bad, 0], sums (P,2)
    float64, err (P) float64 corner errors (+inf: no fit), nkpts (P) keypoints of both images.  Returns a (9) float64 tensor in
    SCALARS' order.  The median of an even count is the mean of the two middle ones; +inf stays in the order statistics."""
    c = counts.double()
    v, r = c[:, 0] + c[:, 1], c[:, 2] + c[:, 3]
    zero = torch.zeros((), dtype=torch.float64, device=c.device)
    rep = torch.where(v > 0, r / v.clamp(min=1.0), zero).mean()
    loc = torch.where(r.sum() > 0, sums.sum() / r.sum().clamp(min=1.0), zero)
    score = (c[:, 5] / c[:, 0].clamp(min=1.0)).mean()
    prec = c[:, 5].sum() / c[:, 4].sum().clamp(min=1.0)
    e = torch.sort(err)[0]
    n = e.numel()
    lo, hi = e[(n - 1) // 2], e[n // 2]
    median = torch.where(lo == hi, lo, 0.5 * (lo + hi))              # (inf + inf stays inf; no inf - inf anywhere)
    return torch.stack([rep, loc, nkpts.double().sum() / (2.0 * n), score, prec, median] + [(err < k).double().mean() for k in (1.0, 3.0, 5.0)])


class SuperPointValidator:
    def __init__(self, config, dataset, device, max_keypoints=1000, eps=3.0, ransac_thresh=3.0, hypotheses=512, pairs=16, batch_size=None,
                 seed=0):
        model = config["model"]
        d = int(model.get("descriptor_length", 256))
        if not 1 <= int(max_keypoints) <= MAX_KEYPOINTS:
            raise ValueError(f"SuperPointValidator: max_keypoints = {max_keypoints} outside [1, {MAX_KEYPOINTS}]")
        if int(pairs) < 1:
            raise ValueError(f"SuperPointValidator: pairs = {pairs}")
        self.sp_config = {"descriptor_dim": d, "nms_radius": int(model["nms"]), "keypoint_threshold": float(model["detection_threshold"]),
                          "max_keypoints": int(max_keypoints), "remove_borders": 4}
        self.engine = Engine(self.sp_config, {"descriptor_dim": d}, device)      # its own: not the training loop's plain engine
        self.dataset = dataset
        self.eps, self.ransac_thresh, self.hypotheses = float(eps), float(ransac_thresh), int(hypotheses)
        self.pairs, self.seed = int(pairs), int(seed)
        self.batch_size = int(batch_size or model.get("eval_batch_size", 1))
        self.parts = None                 # evaluate(keep_parts=True): the per-batch device tensors of the last pass

    def _batches(self):
        n = min(self.pairs, len(self.dataset))
        return [list(range(i, min(i + self.batch_size, n))) for i in range(0, n, self.batch_size)]

    def _batch(self, b):
        """one batch of pairs: every Engine call of the protocol, nothing read back"""
        eng = self.engine
        img, warped = b["image"], b["warped_img"]
        B, H, W = int(img.shape[0]), int(img.shape[-2]), int(img.shape[-1])
        k0, _, d0, n0 = eng.superpoint_batch(img)
        k1, _, d1, n1 = eng.superpoint_batch(warped)
        # [-1,1]^2 to pixels by the expression Engine.warp_labels uses for the labels of the warped image
        H_gt = eng._scaled(b["homographies"], B, float(W), float(H), -1.).double()
        m0, m1, _, _ = eng.mutual_nn_match(d0.transpose(1, 2), d1.transpose(1, 2), n0, n1)
        counts, sums = eng.keypoint_pair_metrics(k0, n0, k1, n1, H_gt, (H, W), self.eps, matches0=m0)
        H_est, _, _, _ = eng.estimate_homography(k0, k1, m0, counts0=n0, ransac_thresh=self.ransac_thresh, hypotheses=self.hypotheses)
        err = eng.homography_corner_error(H_est, H_gt, (H, W))
        return {"kpts0": k0, "n0": n0, "desc0": d0, "kpts1": k1, "n1": n1, "desc1": d1, "H_gt": H_gt, "matches0": m0, "matches1": m1,
                "counts": counts, "sums": sums, "H_est": H_est, "err": err, "size": (H, W)}

    def evaluate(self, state_dict, keep_parts=False):
        """-> {scalar: float} of SCALARS plus "pairs".  Every call sees the same warps: the dataset's draws are keyed by its seed, which is
        set to the validator's for the pass and put back afterwards."""
        if len(self.dataset) == 0:
            raise RuntimeError("SuperPointValidator.evaluate: the dataset is empty")
        self.engine.load_state_dict(L.NET_SUPERPOINT, state_dict)
        ds = self.dataset
        in_instance, old_seed = "seed" in vars(ds), getattr(ds, "seed", None)
        parts = []
        try:
            if old_seed is not None:
                ds.seed = self.seed
            with torch.no_grad():
                for indices in self._batches():
                    b = ds.batch(indices)
                    if "warped_img" not in b:
                        raise NotImplementedError("SuperPointValidator needs data.warped_pair.enable: the known warp is the ground truth")
                    parts.append(self._batch(b))
                row = reduce_rows(torch.cat([p["counts"] for p in parts]), torch.cat([p["sums"] for p in parts]),
                                  torch.cat([p["err"] for p in parts]), torch.cat([p["n0"] + p["n1"] for p in parts])).cpu().tolist()   # the ONE read-back
        finally:
            if old_seed is not None:
                if in_instance:
                    ds.seed = old_seed
                else:
                    del ds.seed                  # (it was the class's: the instance gets no attribute it did not have)
        self.parts = parts if keep_parts else None
        out = dict(zip(SCALARS, row))
        out["pairs"] = sum(int(p["err"].numel()) for p in parts)
        return out
