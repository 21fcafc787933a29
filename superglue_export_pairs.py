#!/usr/bin/env python
"""SuperGlue training pairs in bulk, and a validation pass, on the GPU -- the data half of the reference's second workflow
(superpoint_glue_train.py: `GlueSparse.__getitem__` at batch 1 inside the training loop, the loss gathered entry by entry).

Per image of <image_path>/train: a random perspective warp, SuperPoint on both images, the ground-truth assignment
(datasets/GlueSparse.py:24-104), `--batch` samples per pass, written as <out_dir>/<name>.npz holding the sample's arrays
(image0, image1, M, keypoints0/1, scores0/1, descriptors0/1 (d,N), matches (2,n), all_matches (2,n_all)).  With SuperGlue weights
(--pretrain_weights indoor | outdoor, or --superglue_checkpoint <file with a 'net' entry>) the same pass scores them: mean loss
(superglue_train.py:289-299), precision and recall of matches0 against the ground truth.  There is no backward pass here: train
with the reference's module on the exported pairs, validate checkpoints here.  --grads prints, beside the loss, the norms of its gradient at the
score matrix and at bin_score through the unrolled Sinkhorn (include/imx_train.h), on the forward's own score matrix copied out of the
workspace (the debug tap 'scores_in': a host round trip, this is a validation tool); the backward of the network's layers is PyTorch's.

The SuperPoint and SuperGlue flags are those of superpoint_glue_train.py; --out_dir, --batch, --seed, --superglue_checkpoint, --grads and
--synthetic N (N synthetic images, synthetic weights, no dataset) are not in the reference."""
import argparse
import os
from pathlib import Path

import numpy as np
import torch

from image_matching_amd import synth
from image_matching_amd.datasets.GlueSparse import GlueSparse
from image_matching_amd.superglue.models.superglue_train import SuperGlue


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--image_path', type=str, default='datasets/ALLSS/', help='Path to the directory of training imgs.')
    # model hyper parameter
    parser.add_argument('--superpoint_weights', type=str, default="superpoint/models/weights/superPointNet_allss_descriptor_128.pth.tar")
    parser.add_argument('--descriptor_dim', type=int, default=128, help='The dimension of feature descriptor')
    parser.add_argument('--keypoint_encoder', type=int, nargs='+', default=[32, 64, 128], help='The dimension of keypoint encoder')
    parser.add_argument('--max_keypoints', type=int, default=1200, help='Maximum number of keypoints detected by Superpoint (\'-1\' keeps all keypoints)')
    parser.add_argument('--keypoint_threshold', type=float, default=0.005, help='SuperPoint keypoint detector confidence threshold')
    parser.add_argument('--nms_radius', type=int, default=4, help='SuperPoint Non Maximum Suppression (NMS) radius (Must be positive)')
    parser.add_argument('--sinkhorn_iterations', type=int, default=30, help='Number of Sinkhorn iterations performed by SuperGlue')
    parser.add_argument('--match_threshold', type=float, default=0.2, help='SuperGlue match threshold')
    parser.add_argument('--resize', type=int, nargs=2, default=[640, 480], help='The size of image')
    parser.add_argument('--pretrain_weights', type=str, default='', help='SuperGlue official weights')
    # not in the reference
    parser.add_argument('--superglue_checkpoint', type=str, default='', help="a checkpoint of the reference's training loop (its 'net' entry) to validate")
    parser.add_argument('--out_dir', type=str, default='Results/ALLSS/superglue_pairs', help='where the .npz samples go')
    parser.add_argument('--batch', type=int, default=16, help='samples per pass')
    parser.add_argument('--seed', type=int, default=0, help='seed of the warp sampler')
    parser.add_argument('--synthetic', type=int, default=0, help='export this many synthetic images (no dataset, synthetic weights)')
    parser.add_argument('--grads', action='store_true', help='print the norms of d loss / d scores and d loss / d bin_score beside the loss')
    return parser


class SyntheticPairs(GlueSparse):
    """the dataset over N synthetic images instead of a directory; `first`: the number of its first image (a validation set beside a
    training set starts where that one ends), `superpoint`: another dataset's SuperPoint to share instead of building one"""

    def __init__(self, n, sp_config, resize, device, first=0, superpoint=None):
        from image_matching_amd.superpoint.models.superpoint_test import SuperPoint
        self.device, self.resize, self.first = device, resize, int(first)
        self.files = [f"synthetic_{i:04d}" for i in range(self.first, self.first + n)]
        if superpoint is not None:
            self.superpoint = superpoint
            return
        self.superpoint = SuperPoint(sp_config).to(device)
        self.superpoint.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth.make_superpoint_state_dict(sp_config['descriptor_dim']).items()})

    def _read(self, index):
        from image_matching_amd import trainpairs
        img = synth.synth_pair(self.first + index, self.resize[1], self.resize[0])[0]
        image = np.clip(np.rint(img.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        return image, trainpairs.sample_matrix(np.random.default_rng([self.seed, index]), image.shape[:2])


def write_samples(out_dir, out, host):
    """one .npz per sample: the arrays of the reference's __getitem__ dict, cut to the sample's counts"""
    for b, name in enumerate(out['file_name']):
        n0, n1, n, na = (int(host[k][b]) for k in ('counts0', 'counts1', 'n_matches', 'n_all'))
        am = host['all_matches'][b][:, :na]
        np.savez_compressed(Path(out_dir, Path(name).stem + '.npz'), image0=host['image0'][b], image1=host['warped'][b], M=out['M'][b],
                            keypoints0=host['keypoints0'][b, :n0], keypoints1=host['keypoints1'][b, :n1],
                            scores0=host['scores0'][b, :n0], scores1=host['scores1'][b, :n1],
                            descriptors0=host['descriptors0'][b, :n0].T, descriptors1=host['descriptors1'][b, :n1].T,
                            matches=am[:, :n], all_matches=am)


def main(argv=None):
    opt = build_parser().parse_args(argv)
    device = torch.device('cuda:0')
    synthetic = opt.synthetic > 0
    if synthetic and opt.max_keypoints == 1200:
        opt.max_keypoints, opt.resize = 256, [320, 240]
    sp_config = {'weights': None if synthetic else opt.superpoint_weights, 'descriptor_dim': opt.descriptor_dim, 'nms_radius': opt.nms_radius,
                 'keypoint_threshold': opt.keypoint_threshold, 'max_keypoints': opt.max_keypoints}
    sg_config = {'descriptor_dim': opt.descriptor_dim, 'keypoint_encoder': opt.keypoint_encoder,
                 'sinkhorn_iterations': opt.sinkhorn_iterations, 'match_threshold': opt.match_threshold}
    if opt.max_keypoints <= 0:
        raise SystemExit("--max_keypoints must be positive: the batched export writes fixed-size tensors")
    if synthetic:
        ds = SyntheticPairs(opt.synthetic, sp_config, opt.resize, device)
    else:
        ds = GlueSparse(os.path.join(opt.image_path, 'train'), sp_config, opt.resize, device)
    ds.seed = opt.seed
    superglue = None
    if synthetic or opt.pretrain_weights in ['indoor', 'outdoor'] or opt.superglue_checkpoint:
        superglue = SuperGlue({**sg_config, 'weights': '' if synthetic else opt.pretrain_weights}, _shared=ds.superpoint._shared).to(device)
        if synthetic:
            sd = synth.make_superglue_state_dict(opt.descriptor_dim, opt.keypoint_encoder, variant="t")
            superglue.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        elif opt.superglue_checkpoint:
            superglue.load_state_dict(torch.load(opt.superglue_checkpoint, map_location='cpu')['net'])
    os.makedirs(opt.out_dir, exist_ok=True)
    H, W = opt.resize[1], opt.resize[0]
    losses, stats, written, skipped = [], np.zeros(3, np.int64), 0, 0
    grad_losses, grad_norms, grad_bins = [], [], []
    for start in range(0, len(ds), opt.batch):
        out = ds.batch(range(start, min(start + opt.batch, len(ds))))
        tensors = {k: v for k, v in out.items() if isinstance(v, torch.Tensor)}
        if superglue is not None:
            eng = ds.superpoint._shared.get_engine([0, 1])
            m0, _, _, _ = eng.superglue(out['keypoints0'], out['scores0'], out['descriptors0'].transpose(1, 2), (H, W),
                                        out['keypoints1'], out['scores1'], out['descriptors1'].transpose(1, 2), (H, W),
                                        n0=out['counts0'], n1=out['counts1'])
            tensors['loss'], tensors['stats'] = eng.match_loss(out['all_matches'], out['n_all'], m0, out['gt0'])
            if opt.grads:
                scores = torch.from_numpy(eng.fetch('scores_in')).to(device)     # (B,N0p,N1p): the forward's scores, padding never read
                g = eng.ot_match_loss_grad(scores, float(superglue.state_dict()['bin_score']), out['all_matches'], out['n_all'],
                                           opt.sinkhorn_iterations, n0=out['counts0'], n1=out['counts1'])
                tensors['grad_loss'], tensors['grad_bin'] = g['loss'], g['grad_bin']
                tensors['grad_norm'] = g['grad_scores'].flatten(1).norm(dim=1)
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in tensors.items()}
        write_samples(opt.out_dir, out, host)
        written += len(out['file_name'])
        keep = host['n_all'] > 0                     # a pair with a side without keypoints is the reference's skip sample
        skipped += int((~keep).sum())
        if superglue is not None:
            losses += list(host['loss'][keep])
            stats += host['stats'][keep].sum(0)
            if opt.grads:
                grad_losses += list(host['grad_loss'][keep])
                grad_norms += list(host['grad_norm'][keep])
                grad_bins += list(host['grad_bin'][keep])
    print(f"wrote {written} samples to {opt.out_dir} ({skipped} without keypoints on a side)")
    if superglue is not None and losses:
        n_gt, n_pred, n_ok = (int(v) for v in stats)
        print(f"validation over {len(losses)} pairs: loss {float(np.mean(losses)):.4f}  precision {n_ok / max(n_pred, 1):.4f}  recall {n_ok / max(n_gt, 1):.4f}  "
              f"({n_ok} correct of {n_pred} predicted, {n_gt} ground-truth matches)")
        if opt.grads:
            print(f"gradients over {len(grad_losses)} pairs: loss {float(np.mean(grad_losses)):.4f} (the recorded Sinkhorn of imx_ot_match_loss_grad)  "
                  f"mean |d loss / d scores| {float(np.mean(grad_norms)):.6f}  mean d loss / d bin_score {float(np.mean(grad_bins)):.6f}")


if __name__ == '__main__':
    main()
