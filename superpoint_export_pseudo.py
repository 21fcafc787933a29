#!/usr/bin/env python
"""Pseudo-label export by homographic adaptation -- MI355X-native drop-in for the reference CLI
(superpoint_export_pseudo.py:18-120): same flags and defaults, the yaml keys it reads (data.preprocessing.resize,
data.homography_adaptation.{num, homographies.params}, model.{nms, detection_threshold, top_k, subpixel.enable},
pretrained), images from datasets/ALLSS/<export_task>/, and <save_output>/<exper_name>/<export_task>/<name>.npz holding
`pts` (K,3) rows (x, y, conf) [+ <name>.png with --outputImg].  Per image: one imx_homography_adapt and one
imx_heatmap_points on the GPU, one copy of the rows back.  Image reading / resizing and the homography sampler are host
plumbing with their own arithmetic and random stream (OpenCV / scipy in the reference): unpinned.

Extra flag (not in the reference): --synthetic N exports N synthetic images with synthetic weights (no dataset needed)."""
import argparse
import logging
import os
from pathlib import Path

import numpy as np
import torch
import yaml

from image_matching_amd import homoadapt, hostops, synth
from image_matching_amd.superpoint.models.model_wrap import SuperPointFrontend_torch

SYNTHETIC_CONFIG = {
    'data': {'preprocessing': {'resize': [240, 320]},
             'homography_adaptation': {'enable': True, 'num': 16, 'homographies': {'params': dict(homoadapt.EXPORT_PARAMS)}}},
    'model': {'name': 'superpoint_train', 'params': {}, 'detection_threshold': 0.015, 'nms': 4, 'top_k': 1200,
              'subpixel': {'enable': True}},
    'pretrained': None,
}


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--command", type=str, default='export_detector_homoAdapt')
    parser.add_argument("--config", type=str, default='superpoint/configs/magicpoint_allss_export.yaml')
    parser.add_argument("--exper_name", type=str, default='magicpoint_synth_homoAdapt_allss_50_[640,480]')
    parser.add_argument("--export_task", type=str, default='train', help="export mode: train or val")
    parser.add_argument("--save_output", type=str, default='Results/ALLSS', help="export mode: train or val")
    parser.add_argument("--eval", action="store_true", default=False, help="turn on eval mode")
    parser.add_argument("--outputImg", action="store_true", default=True, help="output image for visualization")
    parser.add_argument("--debug", action="store_true", default=False, help="turn on debuging mode")
    # not in the reference
    parser.add_argument("--synthetic", type=int, default=0, help="export this many synthetic images (no dataset, synthetic weights)")
    return parser


def samples(args, size_hw):
    """(name, image (H,W) float32 in [0,1]) per image (datasets/ALLSS.py:63-76,141-144)."""
    H, W = size_hw
    if args.synthetic > 0:
        for i in range(args.synthetic):
            yield f"synthetic_{i:04d}", synth.synth_pair(i, H, W)[0].astype(np.float32)
        return
    for p in sorted(Path('datasets/ALLSS/' + args.export_task).iterdir()):
        img = hostops.imread_gray(str(p))
        if img.shape != (H, W):
            img = hostops.resize(img, (W, H))
        yield p.stem, img.astype(np.float32) / 255.0


def draw_keypoints(img, pts):
    """gray (H,W) in [0,255] -> BGR uint8 with a green dot per point"""
    out = np.repeat(np.clip(np.rint(img), 0, 255).astype(np.uint8)[:, :, None], 3, 2)
    x = np.clip(np.rint(pts[:, 0]).astype(int), 0, out.shape[1] - 1)
    y = np.clip(np.rint(pts[:, 1]).astype(int), 0, out.shape[0] - 1)
    out[y, x] = (0, 255, 0)
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(format="[%(asctime)s %(levelname)s] %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO)
    if args.synthetic > 0:
        config = SYNTHETIC_CONFIG
    else:
        with open(args.config, "r") as f:
            config = yaml.safe_load(f)
    device = torch.device("cuda:0")
    fe = SuperPointFrontend_torch(config=config, weights_path=config["pretrained"], nms_dist=config["model"]["nms"],
                                  conf_thresh=config["model"]["detection_threshold"], nn_thresh=0.7, cuda=False, device=device)
    fe.net_parallel()
    engine = fe._engine()
    ha = config['data']['homography_adaptation']
    if not ha.get('enable', False):
        raise SystemExit("data.homography_adaptation.enable is false: nothing to export")
    top_k = config["model"]["top_k"] or 0
    save_output = os.path.join(args.save_output, args.exper_name, args.export_task)
    os.makedirs(save_output, exist_ok=True)
    count = 0
    for i, (name, img) in enumerate(samples(args, config['data']['preprocessing']['resize'])):
        logging.info(f"name: {name}")
        hom, inv = homoadapt.sample_homographies(ha['num'], i, **ha['homographies']['params'])
        pts = homoadapt.export_image(engine, torch.from_numpy(img), hom, inv, fe.conf_thresh, fe.nms_dist, top_k,
                                     config["model"]["subpixel"]["enable"])
        np.savez_compressed(Path(save_output, "{}.npz".format(name)), pts=pts)
        if args.outputImg:
            hostops.imwrite(os.path.join(save_output, name + ".png"), draw_keypoints(img * 255, pts))
        count += 1
    print("output pseudo ground truth: ", count)


if __name__ == "__main__":
    main()
