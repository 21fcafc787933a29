"""Drop-in for the part of the reference's SuperPointFrontend_torch (superpoint/models/model_wrap.py:17-309) that
pseudo-label export uses: constructor, loadModel, net_parallel, run(..., onlyHeatmap=True), the heatmap property,
getPtsFromHeatmap and soft_argmax_points.  Training-side paths raise.  PointTracker is not provided."""
import os

import numpy as np
import torch

from .superpoint_train import SuperPoint

_NOT_HERE = ("is training-side and outside the homographic-adaptation export this class was ported for "
             "(issue: 'Homographic adaptation: pseudo-label export on the GPU')")


class SuperPointFrontend_torch(object):
    def __init__(self, config, weights_path, nms_dist, conf_thresh, nn_thresh,
                 cuda=False, trained=False, device='cpu', grad=False, load=True):
        self.config = config
        self.name = 'SuperPoint'
        self.cuda = cuda
        self.nms_dist = nms_dist
        self.conf_thresh = conf_thresh
        self.nn_thresh = nn_thresh
        self.cell = 8
        self.border_remove = 4
        self.sparsemap = None
        self._heatmap = None
        self.pts = None
        self.pts_subpixel = None
        self.patches = None
        d = torch.device(device)
        self.device = d if d.type == "cuda" else torch.device("cuda")     # GPU only
        self.subpixel = bool(self.config['model']['subpixel']['enable'])
        self.net = None
        if load:
            self.loadModel(weights_path)

    def loadModel(self, weights_path):
        model = self.config['model']['name']
        if model != 'superpoint_train':
            raise ValueError(f"model {model!r}: only 'superpoint_train' is provided")
        self.net = SuperPoint(**(self.config['model'].get('params') or {})).to(self.device)
        if weights_path is None:    # asked for explicitly (the CLI's --synthetic, tests): the constructor's synthetic weights stay
            print("[imx] no weights path given: using synthetic weights")
            return
        # the output of this class is training ground truth: a missing checkpoint (or a Git-LFS pointer) is an error, never a
        # silent substitution
        if not os.path.exists(weights_path) or os.path.getsize(weights_path) <= 4096:
            raise FileNotFoundError(f"SuperPoint checkpoint {weights_path!r} not found (or a Git-LFS pointer); pass weights_path=None "
                                    "to run on synthetic weights deliberately")
        checkpoint = torch.load(weights_path, map_location=lambda storage, loc: storage)
        self.net.load_state_dict(checkpoint['model_state_dict'])

    def net_parallel(self):
        pass

    @property
    def heatmap(self):
        return self._heatmap

    @heatmap.setter
    def heatmap(self, heatmap):
        self._heatmap = heatmap

    def _engine(self):
        return self.net._shared.get_engine([self.net._net])

    def run(self, inp, onlyHeatmap=False, train=True):
        """inp [batch, 1, H, W] in [0,1] -> heatmap [batch, 1, H, W] (onlyHeatmap=True, train=False)."""
        if train:
            raise NotImplementedError("run(train=True) " + _NOT_HERE)
        if not onlyHeatmap:
            raise NotImplementedError("run(onlyHeatmap=False) " + _NOT_HERE)
        heatmap = self._engine().superpoint_heatmap(inp.to(self.device))
        self.heatmap = heatmap
        return heatmap

    def getPtsFromHeatmap(self, heatmap):
        """heatmap np / tensor (H, W) (any singleton dims) -> np float64 (3, K)."""
        h = heatmap.detach() if isinstance(heatmap, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(heatmap, dtype=np.float32))
        h = h.squeeze()
        rows = self._engine().heatmap_points_host(h, self.conf_thresh, self.nms_dist)
        return np.ascontiguousarray(rows.T, dtype=np.float64)

    def soft_argmax_points(self, pts, patch_size=5):
        """pts [np (3, K)] on self.heatmap -> [np (3, K)] with x, y moved to the centroid of the 5x5 patch."""
        if patch_size != 5:
            raise NotImplementedError("soft_argmax_points: patch_size 5 only")
        h = self.heatmap
        h = (h.detach() if isinstance(h, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(h, dtype=np.float32))).squeeze()
        p = pts[0]
        # the refined rows of exactly these points: the same extraction with the refinement on returns them in the same order
        ref = np.ascontiguousarray(self._engine().heatmap_points_host(h, self.conf_thresh, self.nms_dist, subpixel=True).T, dtype=np.float64)
        if ref.shape != p.shape or not np.array_equal(ref[2], p[2]):
            raise ValueError("soft_argmax_points: pts are not the points of self.heatmap at this threshold and nms_dist")
        self.pts_subpixel = [ref]
        return self.pts_subpixel.copy()
