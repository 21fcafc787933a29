#!/usr/bin/env python
"""Times the value-and-gradient calls of the two SuperPoint training losses (include/imx_train.h) on the GPU: a batch of 8 warped pairs
at 480 x 640, d = 128 and 256, M = 1000 matches x R = 100 non-matches.  HIP events on the stream, a warm-up, then the median of
`--batches` (at least 20) batches, the variants alternating inside one process.  Per entry point:

  value            the value-only call of the same build (imx_detector_loss / imx_desc_loss_sparse)
  value_and_grad   the value-and-gradient call (imx_detector_loss_grad / imx_desc_loss_sparse_grad)
  torch_backward   the same loss as PyTorch-ROCm ops on the device, forward and loss.backward(), the reference's way: for the detector loss
                   softmax + BCELoss on cell targets and masks prepared on the device outside the timed region; for the descriptor loss
                   tests/spgrad_ref.py's ops per image, index tensors built from host arrays inside the timed call
  dense            the two dense SuperPoint forwards of the same batch, and each call's share of them

A record, not a gate.  Needs a GPU.  Prints one JSON line (kept as profiles/spgrad_time.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from image_matching_amd import _lib as L                      # noqa: E402
from image_matching_amd import homoadapt, sptrain, synth      # noqa: E402
from image_matching_amd.engine import Engine                  # noqa: E402
from tests import spgrad_ref as G                             # noqa: E402
from tests import sptrain_ref as R                            # noqa: E402
from tests import util                                        # noqa: E402

B, H, W, M, RN, KPTS, RADIUS = 8, 480, 640, 1000, 100, 600, 3
HC, WC = H // 8, W // 8


def events_ms(fns, batches, warmup=3):
    """the variants of `fns` (name -> callable) alternate inside every batch; median and minimum per variant"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(batches):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "batches": len(t)} for k, t in times.items()}


def main():
    torch.set_grad_enabled(True)
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spgrad_time needs a GPU (no CPU fallback)")
    batches = max(a.batches, 20)
    rng = np.random.default_rng(0)
    images = torch.from_numpy(np.stack([synth.synth_pair(i, H, W)[0] for i in range(B)]).astype(np.float32)).cuda()
    mats = [homoadapt.sample_homographies(2, i, **R.WARPED_PAIR_PARAMS) for i in range(B)]
    hom = torch.from_numpy(np.stack([m[0][1] for m in mats]))
    inv = torch.from_numpy(np.stack([m[1][1] for m in mats])).cuda()
    pts_np = np.stack([rng.random((B, KPTS)) * (W - 1), rng.random((B, KPTS)) * (H - 1)], 2).astype(np.float32)
    pts, counts = torch.from_numpy(pts_np).cuda(), torch.full((B,), KPTS, dtype=torch.int32).cuda()
    res = {}
    for d in (128, 256):
        eng = Engine(util.sp_config(d, 1024), util.sg_config(d), "cuda")
        eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(d))
        warped = eng.warp_homography(images, inv)
        x = torch.cat([images, warped])[:, None].contiguous()
        semi, desc = eng.superpoint_dense(x)
        wl = eng.warp_labels(pts, counts, hom, H, W)[0]
        mask = eng.erode_mask(eng.warp_homography((H, W), inv, mode="nearest"), RADIUS)
        choice, non = sptrain.draw(eng, hom, HC, WC, M, RN)
        pairs, nv = eng.desc_pairs(hom, HC, WC)
        pairs_h, nv_h, ch_h, non_h = pairs.cpu().numpy(), nv.cpu().numpy(), choice.cpu().numpy(), non.cpu().numpy().astype(np.int64)
        wl_h, mask_h = wl.cpu().numpy(), mask.cpu().numpy()

        # the reference's training step has the 65-channel targets and the cell masks on the device before the loss (labels2Dto3D, getMasks):
        # they are formed once, outside the timed region; the timed call is the written form, softmax then BCELoss, and its backward
        t3, m3 = R.cell_targets(wl_h, torch.float32).cuda(), R.cell_masks(mask_h, torch.float32).cuda()
        bce = torch.nn.BCELoss(reduction="none")

        def torch_det():
            s = semi[B:].clone().requires_grad_(True)
            loss = (bce(torch.softmax(s, 1), t3).sum(1) * m3).sum() / (m3.sum() + 1e-10)      # Train_model_heatmap.py:72-81
            loss.backward()
            return s.grad

        def torch_desc(method):
            a_, b_ = desc[:B].clone().requires_grad_(True), desc[B:].clone().requires_grad_(True)
            total = sum(G.desc_loss_t(a_[i], b_[i], pairs_h[i, :nv_h[i], 0], pairs_h[i, :nv_h[i], 1], ch_h[i], non_h[i], 1.0, 0.2, method)
                        for i in range(B) if nv_h[i] > 0) / B
            total.backward()
            return a_.grad, b_.grad
        row = {"dense": events_ms({"dense": lambda: eng.superpoint_dense(x)}, batches)["dense"]}
        if d == 128:
            res["detector_loss"] = events_ms({"value": lambda: eng.detector_loss(semi[B:], wl, mask),
                                              "value_and_grad": lambda: eng.detector_loss_grad(semi[B:], wl, mask),
                                              "torch_backward": torch_det}, batches)
        for m in ("1d", "2d"):
            row[m] = events_ms({"value": lambda m=m: eng.desc_loss_sparse(desc[:B], desc[B:], hom, choice, non, 1.0, 0.2, m),
                                "value_and_grad": lambda m=m: eng.desc_loss_sparse_grad(desc[:B], desc[B:], hom, choice, non, 1.0, 0.2, m),
                                "torch_backward": lambda m=m: torch_desc(m)}, batches)
        for k in [k for k in ("1d", "2d")] + (["detector_loss"] if d == 128 else []):
            r = row[k] if k in row else res[k]
            r["grad_over_value"] = round(r["value_and_grad"]["median_ms"] / r["value"]["median_ms"], 3)
            r["torch_over_grad"] = round(r["torch_backward"]["median_ms"] / r["value_and_grad"]["median_ms"], 3)
            r[f"share_of_dense_d{d}"] = round(r["value_and_grad"]["median_ms"] / row["dense"]["median_ms"], 4)
        res[f"desc_loss_sparse_d{d}"] = row
        build = eng.lib.imx_version().decode()
        del eng
    print(json.dumps({"tool": "spgrad_time", "build": build, "device": torch.cuda.get_device_name(0), "batch": B, "H": H, "W": W, "M": M, "R": RN,
                      "timing": "HIP events on the stream, median of the batches after a warm-up, the variants alternating.  torch_backward, detector: softmax + "
                                "BCELoss (the written form) and backward() on cell targets and masks already on the device, a clone of semi included; "
                                "descriptor: tests/spgrad_ref.py's ops per image, which build their index tensors from host arrays inside the timed call, as "
                                "the reference does, and read the hard-negative count back",
                      "ms_per_batch_of_8": res}))


if __name__ == "__main__":
    main()
