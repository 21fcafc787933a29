"""Drop-in for the reference's descriptor-training dataset (datasets/ALLSS.py:11-260) with `warped_pair` enabled: the same
constructor, `__len__` and the `__getitem__` dict (keys, shapes, dtypes) given images and the `.npz` pseudo-labels that
superpoint_export_pseudo.py writes; `batch(indices)` does many samples in one pass and returns stacked device tensors.  The warp,
the valid mask and its erosion, and both label maps run in libimx.  The homographies come from
image_matching_amd.homoadapt.sample_homographies (its own seeded stream: unpinned).  `photometric.enable` and
`gaussian_label.enable` raise: both need imgaug, a host step this project does not restate."""
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import Dataset

from .. import homoadapt, hostops, sptrain


def _merge(base, over):
    out = dict(base)
    for k, v in over.items():
        out[k] = _merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


class ALLSS(Dataset):
    default_config = {
        'labels': None, 'cache_in_memory': False, 'validation_size': 100, 'truncate': None,
        'preprocessing': {'resize': [240, 320]}, 'num_parallel_calls': 10,
        'augmentation': {'photometric': {'enable': False, 'primitives': 'all', 'params': {}, 'random_order': True},
                         'homographic': {'enable': False, 'params': {}, 'valid_border_margin': 0}},
        'warped_pair': {'enable': False, 'params': {}, 'valid_border_margin': 0},
        'homography_adaptation': {'enable': False},
        'gaussian_label': {'enable': False},
    }
    seed = 0

    def __init__(self, export=False, transform=None, task='train', images=None, points=None, device='cuda', **config):
        """`images` (n,H,W) float32 in [0,1] with `points` (a list of (k,2+) arrays, (x, y) first) replace the directory scan of the
        reference (datasets/ALLSS/<task>, labels/<task>/<name>.npz): what --synthetic and the tests use."""
        self.config = _merge(self.default_config, config)
        self.transforms = transform
        self.action = 'train' if task == 'train' else 'val'
        self.device = device
        if self.config['augmentation']['photometric']['enable']:
            raise NotImplementedError("augmentation.photometric needs imgaug, which is on no machine of this project: disable it")
        if self.config['gaussian_label']['enable']:
            raise NotImplementedError("gaussian_label needs imgaug's GaussianBlur, which is on no machine of this project: disable it")
        self.sizer = self.config['preprocessing']['resize']
        self.cell_size = 8
        self._images, self._points = images, points
        self.samples = []
        if images is not None:
            self.samples = [{'image': i, 'name': str(i), 'points': i} for i in range(len(images))]
        else:
            base_path = Path('datasets/ALLSS/' + task)
            for p in sorted(base_path.iterdir()) if base_path.exists() else []:
                if self.config['labels']:
                    lab = Path(self.config['labels'], task, '{}.npz'.format(p.stem))
                    if lab.exists():
                        self.samples.append({'image': str(p), 'name': p.stem, 'points': str(lab)})
                else:
                    self.samples.append({'image': str(p), 'name': p.stem})

    def __len__(self):
        return len(self.samples)

    def _read(self, index):
        s = self.samples[index]
        if self._images is not None:
            p = np.asarray(self._points[index], np.float32)
            return np.asarray(self._images[index], np.float32), p.reshape(-1, p.shape[-1] if p.ndim == 2 else 2)[:, :2]
        img = hostops.resize(np.ascontiguousarray(hostops.imread_gray(s['image']), np.uint8), (self.sizer[1], self.sizer[0]))
        pts = np.load(s['points'])['pts'][:, :2] if 'points' in s else np.zeros((0, 2))
        return img.astype('float32') / 255.0, np.asarray(pts, np.float32)

    def batch(self, indices):
        """Stacked device tensors for many samples: image (B,1,H,W), pts (B,Kcap,2) / counts (B) int32, homographies / inv_homographies
        (B,3,3), labels_2D (B,1,H,W), valid_mask (B,H,W), warped_img (B,1,H,W), warped_labels (B,1,H,W), warped_res (B,2,H,W),
        warped_valid_mask (B,H,W), labels_res (B,2,H,W), valid_border_margin, name.  No host synchronisation."""
        indices = list(indices)
        imgs, pts = zip(*(self._read(i) for i in indices))
        B, (H, W) = len(imgs), imgs[0].shape
        eng = sptrain.plain_engine(self.device)
        cap = max(1, max(len(p) for p in pts))
        padded = np.zeros((B, cap, 2), np.float32)
        for b, p in enumerate(pts):
            padded[b, :len(p)] = p
        counts = torch.tensor([len(p) for p in pts], dtype=torch.int32)
        wp = self.config['warped_pair']
        mats = [homoadapt.sample_homographies(2, [self.seed, i], **wp['params']) for i in indices]
        hom = torch.from_numpy(np.stack([m[0][1] for m in mats]))
        inv = torch.from_numpy(np.stack([m[1][1] for m in mats]))
        image = torch.from_numpy(np.stack(imgs)).to(eng.device)
        pts_d, counts_d = torch.from_numpy(padded).to(eng.device), counts.to(eng.device)
        labels, _, _ = eng.warp_labels(pts_d, counts_d, None, H, W, want_res=False)
        out = {'image': image[:, None], 'pts': pts_d, 'counts': counts_d, 'labels_2D': labels[:, None],
               'valid_mask': torch.ones(B, H, W, device=eng.device), 'labels_res': torch.zeros(B, 2, H, W, device=eng.device),
               'name': [self.samples[i]['name'] for i in indices], 'valid_border_margin': int(wp['valid_border_margin'])}
        if wp['enable']:
            wl, wres, _ = eng.warp_labels(pts_d, counts_d, hom, H, W)
            out.update({'homographies': hom.to(eng.device), 'inv_homographies': inv.to(eng.device),
                        'warped_img': eng.warp_homography(image, inv.to(eng.device))[:, None], 'warped_labels': wl[:, None], 'warped_res': wres,
                        'warped_valid_mask': eng.erode_mask(eng.warp_homography((H, W), inv.to(eng.device), mode='nearest'),
                                                            int(wp['valid_border_margin']))})
        return out

    def __getitem__(self, index):
        """The reference's dict for one sample (ALLSS.py:136-255): host tensors with its shapes."""
        b = self.batch([index])
        keep = ('image', 'valid_mask', 'labels_2D', 'labels_res', 'warped_img', 'warped_labels', 'warped_res', 'warped_valid_mask',
                'homographies', 'inv_homographies')
        out = dict(self.samples[index])
        out.update({k: b[k][0].cpu() for k in keep if k in b})
        out['valid_mask'] = out['valid_mask'][None]
        if 'warped_valid_mask' in out:
            out['warped_valid_mask'] = out['warped_valid_mask'][None]
        out.update({'name': self.samples[index]['name'], 'scene_name': "./"})
        return out
