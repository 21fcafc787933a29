"""datasets/ALLSS.py with `augmentation.photometric.enable` served: ALLSSPhotometric augments `image` and `warped_img` of a training batch
on the GPU (Engine.photometric: libimx_photo.so), with separately drawn parameters, in the pass that makes them.  The warped image is
warped from the un-augmented original and augmented afterwards, as the reference does (datasets/ALLSS.py:219-224).  Only task='train'
is augmented (the reference sets enable_photo_val = False).  ALLSS itself stays as it is: it still raises on the flag; this class
strips the flag before it gets there.  `gaussian_label.enable` still raises."""
import copy

from .. import photometric, sptrain
from .ALLSS import ALLSS


class ALLSSPhotometric(ALLSS):
    def __init__(self, export=False, transform=None, task='train', images=None, points=None, device='cuda', **config):
        config = copy.deepcopy(config)
        photo = config.get('augmentation', {}).get('photometric', {})
        self.enable_photo = bool(photo.get('enable', False)) and task == 'train'
        if 'enable' in photo:
            photo['enable'] = False
        super().__init__(export=export, transform=transform, task=task, images=images, points=points, device=device, **config)
        self.photo_config = self.config['augmentation']['photometric']

    def batch(self, indices):
        """ALLSS.batch with `image` and, where warped_pair is enabled, `warped_img` augmented: parameters and Philox keys of sample i are
        drawn under (seed, i, 0) for the image and (seed, i, 1) for the warped image.  Everything else is ALLSS.batch's, bit for bit.
        No host synchronisation."""
        indices = list(indices)
        out = super().batch(indices)
        if not self.enable_photo:
            return out
        eng = sptrain.plain_engine(self.device)
        names = [k for k in ('image', 'warped_img') if k in out]
        H, W = out['image'].shape[-2:]
        for which, k in enumerate(names):
            params = photometric.sample_params(self.photo_config, [(i, which) for i in indices], self.seed, (H, W))
            out[k] = eng.photometric(out[k].contiguous(), params)
        return out
