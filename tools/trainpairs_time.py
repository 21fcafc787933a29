#!/usr/bin/env python
"""Times SuperGlue training-pair generation (datasets/GlueSparse.py:24-104) and the loss (superglue_train.py:289-299) on the GPU:
a batch of 64 samples at 480 x 640 with max_keypoints 1024, HIP events on the stream, a warm-up, then the median of `--batches`
(at least 20) batches for

  warp          imx_warp_perspective_u8 of the 64 images
  superpoint    `/255` of both stacks and SuperPoint on the 128 images (the existing path: the yardstick of the new stages)
  gt_matches    imx_gt_matches on the 64 pairs
  match_loss    imx_match_loss on the 64 pairs after a SuperGlue forward (the forward itself is reported, not part of the stage)
  sample        Engine.train_pairs, everything of a sample in one go

and beside them the same glue the way the reference does it, per SAMPLE at batch 1 (the median of `--baseline_samples` samples,
times 64 for the batch figure): the warp on the host (numpy restatement of the OpenCV call: OpenCV itself is not available), two
SuperPoint forwards as PyTorch-ROCm ops (the oracle's statement of the reference module, on the GPU), the keypoints copied to the
host, scipy's cdist and the numpy argmin / set operations, and the loss gathered entry by entry from the device tensor in a Python
loop.  Wall clock around a device synchronisation for the baseline (it has host work in it).  Needs a GPU.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from image_matching_amd import _lib as L                      # noqa: E402
from image_matching_amd import synth, trainpairs              # noqa: E402
from image_matching_amd.engine import Engine                  # noqa: E402
from oracle import superpoint_ref                             # noqa: E402
from tests import trainpairs_ref as R                         # noqa: E402
from tests import util                                        # noqa: E402

B, H, W, K, D = 64, 480, 640, 1024, 128


def events_ms(fn, batches, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(batches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"median_ms": round(float(np.median(times)), 4), "min_ms": round(min(times), 4), "batches": len(times)}


def wall_ms(fn, n, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 4)


def host_assignment(proj, k1):
    """GlueSparse.py:65-82 as numpy / scipy do it: cdist, two argmins, the mutual test, the three runs of columns"""
    from scipy.spatial.distance import cdist
    d = cdist(proj, k1)
    near_i, near_j = d.argmin(0), d.argmin(1)
    js = np.nonzero((near_j[near_i] == np.arange(len(k1))) & (d[near_i, np.arange(len(k1))] < 3))[0]
    un0, un1 = np.setdiff1d(np.arange(len(proj)), near_i[js]), np.setdiff1d(np.arange(len(k1)), js)
    return np.concatenate([np.stack([near_i[js], js]), np.stack([un0, np.full(len(un0), len(k1))]), np.stack([np.full(len(un1), len(proj)), un1])], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--baseline_samples", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("trainpairs_time needs a GPU (no CPU fallback)")
    batches = max(a.batches, 20)
    eng = Engine(util.sp_config(D, K), util.sg_config(D), "cuda")
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(D))
    eng.load_state_dict(L.NET_SUPERGLUE, util.sg_sd(D, variant="t"))
    imgs_np = np.stack([np.clip(np.rint(synth.synth_pair(i, H, W)[0].astype(np.float64) * 255), 0, 255).astype(np.uint8) for i in range(B)])
    Ms = np.stack([trainpairs.sample_matrix(np.random.default_rng([0, i]), (H, W)) for i in range(B)])
    imgs = torch.from_numpy(imgs_np).cuda()
    minv = torch.from_numpy(np.stack([np.linalg.inv(m) for m in Ms])).cuda()
    Md = torch.from_numpy(Ms).cuda()

    out = eng.train_pairs(imgs, Ms)
    x = torch.empty(2 * B, 1, H, W, dtype=torch.float32, device="cuda")

    def superpoint():
        eng.ingest(imgs, out=x[:B])
        eng.ingest(out["warped"], out=x[B:])
        return eng.superpoint_batch(x)

    def forward():
        return eng.superglue(out["keypoints0"], out["scores0"], out["descriptors0"].transpose(1, 2), (H, W),
                             out["keypoints1"], out["scores1"], out["descriptors1"].transpose(1, 2), (H, W), n0=out["counts0"], n1=out["counts1"])
    res = {"warp": events_ms(lambda: eng.warp_perspective_u8(imgs, minv, inverse=True), batches),
           "superpoint": events_ms(superpoint, batches),
           "gt_matches": events_ms(lambda: eng.gt_matches(out["keypoints0"], out["keypoints1"], Md, out["counts0"], out["counts1"]), batches),
           "superglue_forward": events_ms(forward, batches)}
    m0 = forward()[0]
    res["match_loss"] = events_ms(lambda: eng.match_loss(out["all_matches"], out["n_all"], m0, out["gt0"]), batches)
    res["sample"] = events_ms(lambda: eng.train_pairs(imgs, Ms), batches)
    counts = {k: out[k].cpu().numpy() for k in ("counts0", "counts1", "n_matches", "n_all")}

    # ---- the reference's way, per sample at batch 1
    sd = {k: v.cuda() for k, v in util.sp_sd(D).items()}
    cfg = util.sp_config(D, K)
    state = {}

    def base_warp():
        state["warped"] = R.warp_perspective_u8(imgs_np[0], np.linalg.inv(Ms[0]))

    def base_superpoint():
        for key, im in (("p0", imgs_np[0]), ("p1", state["warped"])):
            t = torch.from_numpy(im / 255.).float()[None, None].cuda()
            state[key] = superpoint_ref.superpoint_forward(t, sd, cfg)

    def base_assignment():
        k0, k1 = state["p0"]["keypoints"][0].cpu().numpy(), state["p1"]["keypoints"][0].cpu().numpy()
        state["all_matches"] = host_assignment(R.project(k0, Ms[0]), k1)

    Z = torch.randn(K + 1, K + 1, device="cuda")[None]

    def base_loss():
        am = torch.from_numpy(state["all_matches"].T.copy()).cuda()
        loss = []
        for i in range(len(am)):
            loss.append(-torch.log(Z[0][am[i][0]][am[i][1]].exp()))
        return float(torch.mean(torch.stack(loss)))
    base_warp()
    base_superpoint()
    base_assignment()
    n = max(a.baseline_samples, 20)
    base = {"warp_host": wall_ms(base_warp, n), "superpoint_torch": wall_ms(base_superpoint, n), "assignment_host": wall_ms(base_assignment, n),
            "loss_python_loop": wall_ms(base_loss, max(n // 4, 5))}
    base["sample"] = round(base["warp_host"] + base["superpoint_torch"] + base["assignment_host"], 4)
    new_stages = res["warp"]["median_ms"] + res["gt_matches"]["median_ms"]
    note = None
    if new_stages > 0.1 * res["superpoint"]["median_ms"]:
        worst = "warp_perspective" if res["warp"]["median_ms"] > res["gt_matches"]["median_ms"] else "gt_matches (gt_nearest)"
        note = f"the two new stages take {new_stages:.3f} ms, more than a tenth of SuperPoint's {res['superpoint']['median_ms']:.3f} ms on the same batch; the larger one is {worst}"
    print(json.dumps({"tool": "trainpairs_time", "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0),
                      "batch": B, "H": H, "W": W, "max_keypoints": K, "descriptor_dim": D,
                      "keypoints_mean": [float(counts["counts0"].mean()), float(counts["counts1"].mean())], "gt_matches_mean": float(counts["n_matches"].mean()),
                      "timing": "HIP events on the stream, median of the batches after a warm-up; baseline: wall clock around a device synchronisation, median per sample at batch 1",
                      "ms_per_batch_of_64": res, "new_stages_over_superpoint": round(new_stages / res["superpoint"]["median_ms"], 4), "note": note,
                      "baseline_ms_per_sample": base, "baseline_ms_per_batch_of_64": {k: round(v * B, 2) for k, v in base.items()}}))


if __name__ == "__main__":
    main()
