#!/usr/bin/env python
"""Times the descriptor-training stages (superpoint/Train_model_heatmap.py:83-314) on the GPU: a batch of 8 warped pairs at
480 x 640, d = 128 and 256, M = 1000 matches x R = 100 non-matches, HIP events on the stream, a warm-up, then the median of
`--batches` (at least 20) batches for

  warp_labels       imx_warp_labels: both label maps (with and without matrices) of the 8 images
  erode_mask        imx_erode_mask, radius 3 (the shipped yaml's valid_border_margin)
  detector_loss     imx_detector_loss, both losses
  desc_loss_sparse  imx_desc_loss_sparse (per d), and its draws restated on the device (Engine.desc_pairs + sptrain.draw_*)
  dense             the two dense SuperPoint forwards of the batch (the existing path: the yardstick of the new stages)
  sp_train_losses   Engine.sp_train_losses, the whole batch in one go (per d)

and beside them the same steps the way the reference does them, per IMAGE at batch 1 (median of `--baseline_samples`, times 8 for the
batch figure): warpLabels and the erosion on the host (the numpy restatements: OpenCV is not available), labels2Dto3D / getMasks /
softmax-BCE as PyTorch-ROCm ops, and descriptor_loss_sparse's Python body -- cell warp and draws on the CPU, index tensors copied to
the device, index_select / grid_sample gathers.  Wall clock around a device synchronisation for the baseline (it has host work in
it).  A record, not a gate.  Needs a GPU.  Prints one JSON line."""
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
from image_matching_amd import homoadapt, sptrain, synth      # noqa: E402
from image_matching_amd.engine import Engine                  # noqa: E402
from tests import sptrain_ref as R                            # noqa: E402
from tests import util                                        # noqa: E402

B, H, W, M, RN, KPTS, RADIUS = 8, 480, 640, 1000, 100, 600, 3
HC, WC = H // 8, W // 8


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


def torch_detector_loss(semi, labels, mask):
    """utils/utils.py:456-468, Train_model_frontend.py:362-377, Train_model_heatmap.py:72-81 as torch ops on the device"""
    def s2d(x):
        b, h, w = x.shape
        return x.reshape(b, h // 8, 8, w // 8, 8).permute(0, 2, 4, 1, 3).reshape(b, 64, h // 8, w // 8)
    t = s2d(labels)
    dust = 1 - t.sum(1)
    dust[dust < 1.] = 0
    t = torch.cat([t, dust[:, None]], 1)
    t = t / t.sum(1, keepdim=True)
    m = s2d(mask).prod(1)
    loss = torch.nn.BCELoss(reduction="none")(torch.softmax(semi, 1), t)
    return (loss.sum(1) * m).sum() / (m.sum() + 1e-10)


def torch_desc_loss(da, db, hom, method):
    """sparse_loss.py:98-174 for one image the reference's way: the warp and the draws on the CPU, gathers on the device"""
    d = da.shape[0]
    pa, pb = R.desc_pairs(R.scale_cells(hom, HC, WC)[0], HC, WC)
    choice = np.random.permutation(len(pa))[:M] if len(pa) >= M else np.concatenate([np.arange(len(pa)), np.random.choice(len(pa), M - len(pa))])
    ia, ib = torch.from_numpy(pa[choice].astype(np.int64)), torch.from_numpy(pb[choice].astype(np.int64))
    non = (torch.rand(M, RN) * WC).floor() + (torch.rand(M, RN) * HC).floor() * WC
    fa, fb = da.view(d, -1).t(), db.view(d, -1).t()
    a1 = torch.index_select(fa, 0, ia.cuda())
    if method == "2d":
        def sample(desc, idx):
            uv = torch.stack([idx % WC, idx // WC], 1).float()
            g = (uv / torch.tensor([WC, HC]).float() * 2 - 1).cuda()
            return torch.nn.functional.grid_sample(desc[None], g[None, :, None], mode="bilinear", align_corners=True)[0, :, :, 0].t()
        ma, mb = sample(da, ia), sample(db, ib)
    else:
        ma, mb = a1, torch.index_select(fb, 0, ib.cuda())
    match = torch.clamp(1 - (ma * mb).sum(-1), min=0).sum() / M
    na = torch.index_select(fa, 0, ia.repeat_interleave(RN).cuda())
    nb = torch.index_select(fb, 0, non.long().view(-1).cuda())
    v = torch.clamp((na * nb).sum(-1) - 0.2, min=0)
    return match + v.sum() / (len(torch.nonzero(v)) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--baseline_samples", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sptrain_time needs a GPU (no CPU fallback)")
    batches, n_base = max(a.batches, 20), max(a.baseline_samples, 20)
    rng = np.random.default_rng(0)
    images = torch.from_numpy(np.stack([synth.synth_pair(i, H, W)[0] for i in range(B)]).astype(np.float32)).cuda()
    mats = [homoadapt.sample_homographies(2, i, **R.WARPED_PAIR_PARAMS) for i in range(B)]
    hom = torch.from_numpy(np.stack([m[0][1] for m in mats]))
    inv = torch.from_numpy(np.stack([m[1][1] for m in mats])).cuda()
    pts_np = np.stack([rng.random((B, KPTS)) * (W - 1), rng.random((B, KPTS)) * (H - 1)], 2).astype(np.float32)
    pts, counts = torch.from_numpy(pts_np).cuda(), torch.full((B,), KPTS, dtype=torch.int32).cuda()
    res, base = {}, {}
    for d in (128, 256):
        eng = Engine(util.sp_config(d, 1024), util.sg_config(d), "cuda")
        eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(d))
        warped = eng.warp_homography(images, inv)
        mask0 = eng.warp_homography((H, W), inv, mode="nearest")
        x = torch.cat([images, warped])[:, None].contiguous()
        semi, desc = eng.superpoint_dense(x)
        labels = eng.warp_labels(pts, counts, None, H, W, want_res=False)[0]
        wl = eng.warp_labels(pts, counts, hom, H, W)[0]
        mask = eng.erode_mask(mask0, RADIUS)
        choice, non = sptrain.draw(eng, hom, HC, WC, M, RN)
        ones = torch.ones_like(labels)
        if d == 128:
            res["warp_labels"] = events_ms(lambda: (eng.warp_labels(pts, counts, None, H, W, want_res=False), eng.warp_labels(pts, counts, hom, H, W)), batches)
            res["erode_mask"] = events_ms(lambda: eng.erode_mask(mask0, RADIUS), batches)
            res["detector_loss"] = events_ms(lambda: (eng.detector_loss(semi[:B], labels, ones), eng.detector_loss(semi[B:], wl, mask)), batches)
        res[f"desc_loss_sparse_d{d}"] = {m: events_ms(lambda m=m: eng.desc_loss_sparse(desc[:B], desc[B:], hom, choice, non, 1.0, 0.2, m), batches)
                                         for m in ("1d", "2d")}
        res[f"draws_d{d}"] = events_ms(lambda: sptrain.draw(eng, hom, HC, WC, M, RN), batches)
        res[f"dense_d{d}"] = events_ms(lambda: eng.superpoint_dense(x), batches)
        res[f"sp_train_losses_d{d}"] = events_ms(lambda: eng.sp_train_losses(images, pts, counts, hom, inv, choice, non, RADIUS, 1.0, 0.2, "2d"), batches)
        new = (res["warp_labels"]["median_ms"] + res["erode_mask"]["median_ms"] + res["detector_loss"]["median_ms"]
               + res[f"desc_loss_sparse_d{d}"]["2d"]["median_ms"])
        res[f"new_stages_over_dense_d{d}"] = round(new / res[f"dense_d{d}"]["median_ms"], 4)
        # ---- the reference's way, per image at batch 1
        hom0, mask_np = hom[0].numpy(), mask0[:1].cpu().numpy()
        if d == 128:
            base["warp_labels_host"] = wall_ms(lambda: (R.points_to_2d(pts_np[0], H, W), R.warp_labels(pts_np[0], R.scale_pixels(hom0, H, W)[0], H, W)), n_base)
            base["erode_host"] = wall_ms(lambda: R.erode(mask_np, RADIUS), n_base)
            base["detector_loss_torch"] = wall_ms(lambda: (torch_detector_loss(semi[:1], labels[:1], ones[:1]),
                                                           torch_detector_loss(semi[B:B + 1], wl[:1], mask[:1])), n_base)
        base[f"desc_loss_torch_d{d}"] = {m: wall_ms(lambda m=m: torch_desc_loss(desc[0], desc[B], hom0, m), n_base) for m in ("1d", "2d")}
        build = eng.lib.imx_version().decode()
        del eng
    print(json.dumps({"tool": "sptrain_time", "build": build, "device": torch.cuda.get_device_name(0), "batch": B, "H": H, "W": W, "M": M, "R": RN,
                      "points_per_image": KPTS, "erosion_radius": RADIUS,
                      "timing": "HIP events on the stream, median of the batches after a warm-up; baseline: wall clock around a device synchronisation, "
                                "median per image at batch 1",
                      "ms_per_batch_of_8": res, "baseline_ms_per_image": base,
                      "baseline_ms_per_batch_of_8": {k: ({m: round(v[m] * B, 2) for m in v} if isinstance(v, dict) else round(v * B, 2)) for k, v in base.items()}}))


if __name__ == "__main__":
    main()
