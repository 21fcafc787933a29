"""Drop-in for the reference's SuperGlue training dataset (datasets/GlueSparse.py:10-104): same constructor, `__len__`, and
`__getitem__` dict (keys, container types, dtypes, the skip dict of :52-61).  The warp, both SuperPoint forwards, the projection,
the distances and the assignment of :32-82 run in libimx; `batch(indices)` does the same for many samples in one pass and returns
stacked device tensors.  Reading and resizing go through hostops; the corner sampler is host plumbing with its own seeded stream
(`seed`, per index) -- the reference draws from numpy's global stream."""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import _lib as L
from .. import hostops, trainpairs
from ..superpoint.models.superpoint_test import SuperPoint


class GlueSparse(Dataset):
    """Warped image pairs with SuperPoint keypoints and their ground-truth assignment, computed by libimx."""
    seed = 0

    def __init__(self, train_path, sp_config, resize, device):
        self.device = device
        self.resize = resize
        self.files = [train_path + '/' + f for f in os.listdir(train_path)]
        self.superpoint = SuperPoint(sp_config).to(device)
        self.superpoint.eval()

    @classmethod
    def beside(cls, other, path):
        """(not in the reference) a dataset over another directory that shares `other`'s SuperPoint, size and device: a validation set
        beside a training set runs on the same engine and weights instead of loading a second copy"""
        self = cls.__new__(cls)
        self.__dict__.update(other.__dict__)          # everything the constructor set, whatever it sets: only the file list differs
        self.files = [path + '/' + f for f in os.listdir(path)]
        return self

    def __len__(self):
        return len(self.files)

    def _engine(self):
        return self.superpoint._shared.get_engine([L.NET_SUPERPOINT])

    def _read(self, index):
        image = hostops.imread_gray(self.files[index])
        image = hostops.resize(np.ascontiguousarray(image, np.uint8), (self.resize[0], self.resize[1]))
        return image, trainpairs.sample_matrix(np.random.default_rng([self.seed, index]), image.shape[:2])

    def _pairs(self, images, mats):
        """the engine's dict for a stack of images; max_keypoints < 0 (keep all) sizes the outputs from the counts (one sync)"""
        eng = self._engine()
        src = torch.from_numpy(np.stack(images))
        if eng.max_keypoints > 0:
            return eng.train_pairs(src, mats)
        B = len(images)
        src = src.to(eng.device)
        warped = eng.warp_perspective_u8(src, mats)
        x = torch.empty(2 * B, 1, *src.shape[1:], dtype=torch.float32, device=eng.device)
        eng.ingest(src, out=x[:B])
        eng.ingest(warped, out=x[B:])
        kpts, scores, desc, n = eng.superpoint(x)
        counts = torch.tensor(n, dtype=torch.int32, device=eng.device)
        out = {"warped": warped, "keypoints0": kpts[:B], "keypoints1": kpts[B:], "scores0": scores[:B], "scores1": scores[B:],
               "descriptors0": desc[:B], "descriptors1": desc[B:], "counts0": counts[:B].contiguous(), "counts1": counts[B:].contiguous()}
        out.update(eng.gt_matches(out["keypoints0"], out["keypoints1"], mats, out["counts0"], out["counts1"]))
        return out

    def __getitem__(self, index):
        image, M = self._read(index)
        host = trainpairs.to_host(self._pairs([image], M[None]))
        return trainpairs.reference_sample(host, 0, image, host['warped'][0], self.files[index], self.device)

    def batch(self, indices):
        """Many samples in one pass: the engine's stacked device tensors (Engine.train_pairs) plus 'image0' (B,H,W) uint8,
        'M' (B,3,3) float64 (host) and 'file_name' (list).  Images must share one size (they do after `resize`)."""
        indices = list(indices)
        images, mats = zip(*(self._read(i) for i in indices))
        out = self._pairs(list(images), np.stack(mats))
        out['image0'] = torch.from_numpy(np.stack(images)).to(out['warped'].device)
        out['M'] = np.stack(mats)
        out['file_name'] = [self.files[i] for i in indices]
        return out
