#!/usr/bin/env python
"""SuperPoint + SuperGlue registration with a choice of the fitted model -- not in the reference, whose registration scripts
(superpoint_glue_test.py, superpoint_glue_official_test.py) fit a 4-DoF similarity only.  The flags, the directory convention
(<img_dir>/source1/*, <img_dir>/template1/<one image>) and the outputs (<Result_dir>/<exper_name>/Transform/trans_<file>,
.../Match/<file>) are those of the script named by --models, plus

    --transform similarity    that script's own loop (superpoint_glue_test.run_registration), untouched
    --transform homography    a full homography by RANSAC on the GPU (imx_estimate_homography, the cv2.findHomography(..., cv2.RANSAC)
                              counterpart) on the device-compacted matches, rescaled to the original image as S^-1 H S with
                              S = diag(resize_scale, resize_scale, 1), the warp through imx_warp_perspective_u8, the drawn matches
                              filtered by the inlier mask.  It needs --ransac gpu.  With at most 3 or more than 8192 matches, or a
                              failed call, the fit falls back to the host's similarity as gpu_affine_partial's callers do.
    --models trained|official the BN SuperPoint + SuperGlue of superpoint_glue_test.py (default) or the official pair of
                              superpoint_glue_official_test.py

    python superpoint_glue_register.py --synthetic 2 --transform homography --resize_scale 0.5 --max_keypoints 512"""
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

import superpoint_glue_test as trained
from image_matching_amd import hostops, synth

torch.set_grad_enabled(False)

HOMOGRAPHY_THRESH = 3.0    # px at the network's resolution: cv2.findHomography's default ransacReprojThreshold


def build_parser(models='trained'):
    """the parser of the script `models` names, plus --transform and --models"""
    if models == 'official':
        import superpoint_glue_official_test as base
    else:
        base = trained
    p = base.build_parser()
    p.add_argument('--transform', choices=['similarity', 'homography'], default='similarity',
                   help="the fitted model: 'similarity' = the reference's partial-affine fit, 'homography' = RANSAC homography on the GPU "
                        "(imx_estimate_homography; needs --ransac gpu)")
    p.add_argument('--models', choices=['trained', 'official'], default=models, help='whose flags, defaults and networks')
    return p


def models_of(argv):
    """the value of --models in argv ('trained' when absent): it decides which parser reads the rest"""
    argv = list(sys.argv[1:] if argv is None else argv)
    for i, a in enumerate(argv):
        if a == '--models' and i + 1 < len(argv):
            return argv[i + 1]
        if a.startswith('--models='):
            return a.split('=', 1)[1]
    return 'trained'


def load_matching(opt):
    """the Matching of the script opt.models names, with that script's synthetic weights where a checkpoint is absent"""
    tt = lambda sd: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    if opt.models == 'official':
        import superpoint_glue_official_test as official
        from image_matching_amd.superglue.models.matching import Matching
        config = official.make_config(opt)
        matching = Matching(config).eval().to('cuda')
        if config['superpoint']['weights_path'] is None:
            matching.superpoint.load_state_dict(tt(synth.synth_state_dict(synth.superpoint_official_shapes(opt.descriptor_dim), 77)))
        if config['superglue']['weights'] is None and opt.descriptor_dim in synth.SG_CONFIGS:
            matching.superglue.load_state_dict(tt(synth.make_superglue_state_dict(opt.descriptor_dim)))
        return matching
    from image_matching_amd.superglue.models.matching_test import Matching
    config = trained.make_config(opt)
    matching = Matching(config).eval().to('cuda')
    if config['superpoint']['weights'] is None and opt.descriptor_dim in (128, 256):
        matching.superpoint.load_state_dict(tt(synth.make_superpoint_state_dict(opt.descriptor_dim)))
    if config['superglue']['weights'] is None and opt.descriptor_dim in synth.SG_CONFIGS \
            and list(config['superglue']['keypoint_encoder']) == synth.SG_CONFIGS[opt.descriptor_dim][0]:
        matching.superglue.load_state_dict(tt(synth.make_superglue_state_dict(opt.descriptor_dim)))
    return matching


def gpu_homography(eng, pred, thresh):
    """RANSAC homography fit on the GPU over the matched pairs only, compacted on the device as in superpoint_glue_test.gpu_affine_partial,
    with its slot limit and its fall-back rule: (H (3,3) float64 or None, mask (n,1)), or (None, None) when the GPU path does not apply."""
    from image_matching_amd.engine import ImxError
    m0 = pred['matches0'][0].long()
    sel = m0 > -1
    n = int(sel.sum())
    if n <= 3 or n > trained.RANSAC_GPU_MAX:
        return None, None
    mk0 = pred['keypoints0'][0][sel][None].float().contiguous()
    mk1 = pred['keypoints1'][0][m0[sel]][None].float().contiguous()
    ident = torch.arange(n, device=m0.device, dtype=torch.int64)[None]
    try:
        H, inl, ninl, _ = eng.estimate_homography(mk0, mk1, ident, ransac_thresh=thresh)
    except ImxError as e:
        print(f"[imx] GPU RANSAC unavailable ({e}); falling back to the host fit")
        return None, None
    return (H[0].cpu().numpy() if int(ninl[0]) > 0 else None), inl[0].cpu().numpy()[:, None]


def run_registration(opt, matching, device):
    """superpoint_glue_test.run_registration with the model opt.transform names.  'similarity' IS that function; 'homography' is its
    per-pair loop with the homography fit and the perspective warp in place of the similarity's.  Returns its list of
    (file, keypoints0, keypoints1, matches, inliers, matrix): the matrix is (3,3) here, in the original image's pixels."""
    if opt.transform != 'homography':
        return trained.run_registration(opt, matching, device)
    if opt.ransac != 'gpu':
        raise SystemExit("--transform homography needs --ransac gpu: the fit is imx_estimate_homography and the warp imx_warp_perspective_u8")
    source_dir, template_dir = opt.img_dir + 'source1/', opt.img_dir + 'template1/'
    template_img_path = template_dir + os.listdir(template_dir)[0]
    results, Matrix = [], None
    for filename in sorted(os.listdir(source_dir)):
        source_original, source_image, template_image = trained.load_pair(source_dir + filename, template_img_path, opt.resize_scale)
        source_tensor = torch.from_numpy(source_image)[None].float().to(device)
        template_tensor = torch.from_numpy(template_image)[None].float().to(device)
        start = time.perf_counter()
        pred = matching({'image0': source_tensor, 'image1': template_tensor})
        engine = matching._shared.engine       # (made by the first forward)
        kpts0, kpts1 = pred['keypoints0'][0].cpu().numpy(), pred['keypoints1'][0].cpu().numpy()
        matches, confidence = pred['matches0'][0].cpu().numpy(), pred['matching_scores0'][0].cpu().numpy()
        valid = matches > -1
        mkpts0, mkpts1 = kpts0[valid], kpts1[matches[valid]]
        if len(mkpts0) > 3:
            M, mask = gpu_homography(engine, pred, HOMOGRAPHY_THRESH)
            if mask is None:       # more matched pairs than the kernel takes, or a failed GPU call: the host's similarity, as the homography it is
                M, mask = hostops.estimate_affine_partial_2d(mkpts0, mkpts1, ransac_thresh=7)
                if M is not None:
                    M = np.concatenate([np.asarray(M, np.float64), [[0.0, 0.0, 1.0]]])
            if M is not None:      # a failed fit keeps the last matrix, as the similarity loop does
                Matrix = np.array(M, dtype=np.float64)
                if opt.resize_scale is not None:       # to the original image: S^-1 H S
                    S = np.diag([opt.resize_scale, opt.resize_scale, 1.0])
                    Matrix = np.linalg.inv(S) @ Matrix @ S
                flag = (mask > 0).ravel().tolist()
                mkpts0, mkpts1 = mkpts0[flag], mkpts1[flag]
        print("Time used:", time.perf_counter() - start)
        results.append((filename, len(kpts0), len(kpts1), int(valid.sum()), len(mkpts0), None if Matrix is None else Matrix.copy()))

        if Matrix is not None:     # imx_warp_perspective_u8: cv2.warpPerspective(source, H, (W, H))
            src_u8 = torch.from_numpy(np.rint(source_original.squeeze() * 255).astype(np.uint8))
            Transform = engine.warp_perspective_u8(src_u8, Matrix[None])[0].cpu().numpy()
            Transform_dir = os.path.join(opt.Result_dir, opt.exper_name, 'Transform/')
            os.makedirs(Transform_dir, exist_ok=True)
            hostops.imwrite(Transform_dir + 'trans_{}'.format(filename), Transform)
        if opt.match_viz:
            import matplotlib.cm as cm
            color = cm.jet(confidence[valid])[:len(mkpts0)] if len(mkpts0) else np.zeros((0, 4))
            text = ['SuperGlue', 'Keypoints: {}:{}'.format(len(kpts0), len(kpts1)), 'Matches: {}'.format(len(mkpts0))]
            small_text = ['Keypoint Threshold: {:.4f}'.format(matching.superpoint.config['keypoint_threshold']),
                          'Match Threshold: {:.2f}'.format(matching.superglue.config['match_threshold']), ' ']
            Match_dir = os.path.join(opt.Result_dir, opt.exper_name, 'Match/')
            os.makedirs(Match_dir, exist_ok=True)
            out_file = str(Path(Match_dir, filename))
            print('\nWriting image to {}'.format(out_file))
            hostops.make_matching_plot_fast(source_image.squeeze() * 255, template_image.squeeze() * 255, kpts0, kpts1, mkpts0, mkpts1, color,
                                            text, path=out_file, show_keypoints=opt.show_keypoints, small_text=small_text)
    return results


def main(argv=None):
    opt = build_parser(models_of(argv)).parse_args(argv)
    print(opt)
    if not torch.cuda.is_available():
        raise SystemExit("superpoint_glue_register.py (imx): needs an MI355X / ROCm GPU; there is no CPU path")
    if opt.transform == 'homography' and opt.ransac != 'gpu':
        raise SystemExit("--transform homography needs --ransac gpu: the fit is imx_estimate_homography and the warp imx_warp_perspective_u8")
    if opt.synthetic > 0:
        trained.write_synthetic_dataset(opt.img_dir, opt.synthetic, opt.resize_scale or 1.0)
    return run_registration(opt, load_matching(opt), 'cuda')


if __name__ == '__main__':
    main()
