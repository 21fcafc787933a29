"""The reference's superpoint_train_descriptor.py on the GPU: the shipped training configuration
(superpoint/configs/superpoint_allss_train_heatmap.yaml: photometric augmentation, soft `gaussian_label` targets, warped pairs, sparse
descriptor loss) through datasets/ALLSS_train.py and superpoint/Train_model_heatmap_loop.py to checkpoints in the reference's layout.
The script's three flags, plus --synthetic N, which needs no dataset (N synthetic images whose pseudo-labels come from homographic
adaptation on a synthetic-weight network), --size, --iters K (train_iter; the intervals are cut to fit) and --val_metrics (at every
validation_interval: repeatability, localisation error, matching score and homography correctness of the deployed network, and a best
checkpoint; the config's validation_metrics key with enable set).

    python superpoint_train_descriptor.py --synthetic 4 --iters 6 --config tests/golden/superpoint_allss_train_heatmap.yaml

Scalars go to tensorboardX's SummaryWriter where that package is installed, otherwise to <output_dir>/<exper_name>/scalars.jsonl.
Ctrl-C saves a checkpoint, as the reference does.  One GPU."""
import argparse
import json
import logging
import os

import numpy as np
import torch

from image_matching_amd.scalars import JsonlWriter, make_writer  # noqa: F401  (shared with superpoint_glue_train.py)


if __name__ == '__main__':
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", type=str, default='superpoint/configs/superpoint_allss_train_heatmap.yaml')
    parser.add_argument("--exper_name", type=str, default='superpoint_allss_descriptor_128')
    parser.add_argument("--output_dir", type=str, default='Results/ALLSS/')
    parser.add_argument("--synthetic", type=int, default=0, help="train on N synthetic images instead of datasets/ALLSS/train")
    parser.add_argument("--size", type=int, nargs=2, default=None, help="H W of the synthetic images (default: 120 160)")
    parser.add_argument("--iters", type=int, default=0, help="train_iter; validation, save and tensorboard intervals are cut to at most half of it")
    parser.add_argument("--val_metrics", action="store_true", help="validation_metrics.enable: measure the deployed network at every validation_interval")
    args = parser.parse_args()

    import yaml
    from image_matching_amd import homoadapt, synth
    from image_matching_amd.datasets.ALLSS_train import ALLSSTrain
    from image_matching_amd.superpoint.Train_model_heatmap_loop import BatchLoader, Train_model_heatmap

    logging.basicConfig(format='[%(asctime)s %(levelname)s] %(message)s', datefmt='%m/%d/%Y %H:%M:%S', level=logging.INFO)
    output_dir = os.path.join(args.output_dir, args.exper_name)
    checkpoints_dir = os.path.join(output_dir, 'checkpoints')
    os.makedirs(checkpoints_dir, exist_ok=True)
    writer = make_writer(output_dir)

    with open(args.config, 'r') as f:
        config = yaml.safe_load(f)
    if args.iters:
        config['train_iter'] = args.iters
        for k in ('validation_interval', 'save_interval', 'tensorboard_interval'):
            config[k] = max(1, min(int(config[k]), args.iters // 2))
    if args.val_metrics:
        config['validation_metrics'] = dict(config.get('validation_metrics') or {}, enable=True)
    with open(os.path.join(output_dir, 'config.yml'), 'w') as f:
        yaml.dump(config, f, default_flow_style=False)

    data_cfg = {k: v for k, v in config['data'].items() if k not in ('dataset', 'root', 'root_split_txt')}
    if args.synthetic:
        from image_matching_amd import _lib as L
        from image_matching_amd.superpoint.models.superpoint_train import SuperPoint
        H, W = args.size or (120, 160)
        labeller = SuperPoint(config['model']['descriptor_length']).to('cuda')       # synthetic weights: the pseudo-labels need some detector
        eng = labeller._shared.get_engine([L.NET_SUPERPOINT])
        images = np.stack([synth.synth_pair(i, H, W)[0] for i in range(args.synthetic)]).astype(np.float32)
        hom, inv = homoadapt.sample_homographies(16, 0, **homoadapt.EXPORT_PARAMS)
        points = [homoadapt.export_image(eng, torch.from_numpy(im).to(eng.device), hom, inv, config['model']['detection_threshold'],
                                         config['model']['nms'], top_k=600) for im in images]
        train_set = ALLSSTrain(task='train', images=images, points=points, **data_cfg)
        val_set = ALLSSTrain(task='val', images=images, points=points, **data_cfg)
    else:
        train_set = ALLSSTrain(task='train', **data_cfg)
        val_set = ALLSSTrain(task='val', **data_cfg)

    train_agent = Train_model_heatmap(config, save_path=checkpoints_dir, device='cuda')
    train_agent.writer = writer
    train_agent.train_loader = BatchLoader(train_set, config['model']['batch_size'])
    train_agent.val_loader = BatchLoader(val_set, config['model']['eval_batch_size'])
    train_agent.loadModel()
    train_agent.dataParallel()

    try:
        train_agent.train()
    except KeyboardInterrupt:
        print("press ctrl + c, save model!")
        train_agent.saveModel()
    torch.cuda.synchronize()
    print(json.dumps({"n_iter": train_agent.n_iter, "checkpoints": sorted(os.listdir(checkpoints_dir)),
                      "last": train_agent.history[-1][2] if train_agent.history else None}))
