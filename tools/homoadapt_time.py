#!/usr/bin/env python
"""Times pseudo-label export by homographic adaptation (one image, N views) on the GPU, both sides in one run, alternating:

  new       homoadapt.export_image: imx_homography_adapt + imx_heatmap_points, one copy of the rows back; per-kernel split
            through imx_set_timing in a separate, untimed-for-the-headline pass
  baseline  what the library offered before: the dense SuperPoint forward (imx_superpoint_dense, both heads) on the N warped
            images, and around it the reference's glue as it is written (utils/utils.py:388-454,491-518: warp of the repeated
            image, nearest-mode masks of a ones stack, softmax / pixel shuffle, two batched warps, two sums, a division) as
            PyTorch ops on the GPU, a device-to-host copy of the map and the host getPtsFromHeatmap (tests/homoadapt_ref.py)

Shapes: 480x640 with N = 50 and N = 100, 240x320 with N = 100.  Every shape: `--rounds` (2) alternations new / baseline; in each, a
warm-up and then repeats for `--seconds / --rounds` (1 s) per side, wall clock around a device synchronisation (the baseline has
host work in it, so device events alone would flatter it); the figure of a round is the median of its repeats and the headline
of a side (`new_ms`, `baseline_ms`) the MINIMUM of its rounds' medians.  `ha_masks_recompute` is the same call with the masks
re-evaluated inside the combine instead of stored (one round).  Needs a GPU;
there is no CPU fallback.  Prints one JSON line."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from image_matching_amd import _lib as L                      # noqa: E402
from image_matching_amd import homoadapt, synth               # noqa: E402
from image_matching_amd.engine import Engine                  # noqa: E402
from tests import homoadapt_ref as R                          # noqa: E402
from tests import util                                        # noqa: E402

THR, NMS, TOP_K = 0.015, 4, 1200


def torch_warp(img, mats, mode):
    """inv_warp_image_batch as the reference writes it, on img's device"""
    B, _, H, W = img.shape
    dev = img.device
    xs, ys = torch.linspace(-1, 1, W, device=dev), torch.linspace(-1, 1, H, device=dev)
    pts = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W), torch.ones(H, W, device=dev)], -1).reshape(-1, 3)
    w = (mats.reshape(B * 3, 3) @ pts.t()).reshape(B, 3, -1).transpose(2, 1)
    grid = (w[:, :, :2] / w[:, :, 2:]).reshape(B, H, W, 2)
    return F.grid_sample(img, grid, mode=mode, align_corners=True)


def baseline(eng, img, hom, inv):
    N, (H, W) = hom.shape[0], img.shape
    warped = torch_warp(img.repeat(N, 1, 1, 1), inv, "bilinear")
    mask = torch_warp(torch.ones(N, 1, H, W, device=img.device), inv, "nearest")
    semi, _ = eng.superpoint_dense(warped)
    heat = F.pixel_shuffle(torch.softmax(semi, 1)[:, :-1], 8)
    num = torch_warp(heat * mask, hom, "bilinear").sum(0)
    den = torch_warp(mask, hom, "bilinear").sum(0)
    out = (num / den).detach().cpu().squeeze().numpy()
    pts = R.points(out, THR, NMS)
    pts = R.subpixel(out, pts).T
    return pts[:TOP_K]


def new(eng, img, hom, inv):
    return homoadapt.export_image(eng, img, hom, inv, THR, NMS, TOP_K, True)


def sclk_mhz():
    for f in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input")):
        try:
            with open(f) as fh:
                return round(int(fh.read()) / 1e6)
        except (OSError, ValueError):
            continue
    return None


def measure(fn, min_s, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times, t_end = [], time.perf_counter() + min_s
    while time.perf_counter() < t_end or len(times) < 3:
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "repeats": len(times), "sclk_mhz_after": sclk_mhz()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0, help="minimum timed seconds per figure")
    ap.add_argument("--rounds", type=int, default=2, help="alternations new / baseline per shape (the figures of a side are pooled by the minimum median)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("homoadapt_time needs a GPU (no CPU fallback)")
    eng = Engine(util.sp_config(128, 64), util.sg_config(128), "cuda")
    eng.load_state_dict(L.NET_SUPERPOINT, util.sp_sd(128))
    shapes = []
    for H, W, N in ((480, 640, 50), (480, 640, 100), (240, 320, 100)):
        img = torch.from_numpy(synth.synth_pair(12, H, W)[0].astype(np.float32)).cuda()
        hom, inv = (torch.from_numpy(m).cuda() for m in homoadapt.sample_homographies(N, 12, **homoadapt.EXPORT_PARAMS))
        k_new, k_base = len(new(eng, img, hom, inv)), len(baseline(eng, img, hom, inv))
        rec = {"H": H, "W": W, "N": N, "points_new": k_new, "points_baseline": k_base, "new": [], "baseline": []}
        for _ in range(a.rounds):
            rec["new"].append(measure(lambda: new(eng, img, hom, inv), a.seconds / a.rounds))
            rec["baseline"].append(measure(lambda: baseline(eng, img, hom, inv), a.seconds / a.rounds))
        # per-kernel split of the new path (events around every launch: its own pass, not the headline)
        eng.set_timing(True)
        eng.timing_reset()
        reps = 5
        for _ in range(reps):
            new(eng, img, hom, inv)
        rows = eng.timing_report()
        eng.set_timing(False)
        eng.timing_reset()
        split = {name: round(ms / reps, 4) for name, _, ms in rows}
        net = sum(v for k, v in split.items() if k.startswith("conv"))
        rec["kernels_ms"] = split
        # the A/B of the masks: stored by the warp launch and read by the combine (default) against re-evaluated inside the combine
        eng.set_option("ha_masks", "recompute")
        ab = measure(lambda: new(eng, img, hom, inv), a.seconds / a.rounds)
        eng.set_timing(True)
        eng.timing_reset()
        for _ in range(reps):
            new(eng, img, hom, inv)
        rows = {name: round(ms / reps, 4) for name, _, ms in eng.timing_report()}
        eng.set_timing(False)
        eng.set_option("ha_masks", "stored")
        rec["ha_masks_recompute"] = {"new_ms": ab["median_ms"], "ha_warp": rows["ha_warp"], "ha_combine": rows["ha_combine"]}
        rec["network_ms"] = round(net, 4)
        rec["non_network_ms"] = round(sum(split.values()) - net, 4)
        rec["new_ms"] = min(r["median_ms"] for r in rec["new"])
        rec["baseline_ms"] = min(r["median_ms"] for r in rec["baseline"])
        rec["speedup"] = round(rec["baseline_ms"] / rec["new_ms"], 2)
        shapes.append(rec)
    print(json.dumps({"tool": "homoadapt_time", "build": eng.lib.imx_version().decode(), "device": torch.cuda.get_device_name(0),
                      "threshold": THR, "nms_dist": NMS, "top_k": TOP_K, "subpixel": True, "timing": "wall clock around a device synchronisation; per round the median of its repeats, headline = minimum over the rounds",
                      "shapes": shapes}))


if __name__ == "__main__":
    main()
