"""Drop-in for the reference's utils/photometric.py: `ImgAugTransform(**config)` and `customizedTransform()` with its call signatures,
a (H,W,1) numpy image in and numpy out -- the import swap.  The arithmetic runs in libimx_photo.so (include/imx_photo.h) on the GPU, one
image per call; a training loop wants datasets/ALLSS_photo.py, which does a whole batch in one pass.  The random draws come from
image_matching_amd.photometric.sample_params under `seed` below and a call counter: unpinned."""
import itertools

import numpy as np
import torch

from .. import photometric, sptrain

seed = 0
_calls = itertools.count()
_PIXEL_STAGES = ('random_brightness', 'random_contrast', 'additive_gaussian_noise', 'additive_speckle_noise', 'motion_blur')


def _engine():
    return sptrain.plain_engine('cuda')


class ImgAugTransform:
    def __init__(self, **config):
        """config['photometric']: 'enable' and, when set, 'params' (random_brightness, random_contrast, additive_gaussian_noise,
        additive_speckle_noise, motion_blur).  Disabled: iaa.Noop, the quantisation alone.  'GaussianBlur' is not served."""
        photo = config['photometric']
        self.config = {'params': {}, 'primitives': 'all'}
        if photo['enable']:
            params = photo['params']
            if params.get('GaussianBlur', False):
                raise NotImplementedError("GaussianBlur needs imgaug's 8-bit fixed-point blur, which this project does not restate")
            self.config['params'] = {k: params[k] for k in _PIXEL_STAGES if params.get(k, False)}

    def __call__(self, img):
        img = np.asarray(img, np.float32)
        H, W = img.shape[:2]
        eng = _engine()
        p = photometric.sample_params(self.config, [next(_calls)], seed, (H, W))
        x = torch.from_numpy(np.ascontiguousarray(img.reshape(1, H, W))).to(eng.device)
        up = lambda name, i32=False: torch.from_numpy(p[name].view(np.int32) if i32 else p[name]).to(eng.device)
        out = eng.photo_pixels(x, up('lut'), up('noise_scale'), up('thresh', True), up('table'), up('blur_kernel'), up('blur_on'), up('key', True))
        return (out.cpu().numpy().astype(np.float32) / 255).reshape(img.shape)


class customizedTransform:
    def __init__(self):
        pass

    def additive_shade(self, image, nb_ellipses=20, transparency_range=[-0.5, 0.8], kernel_size_range=[250, 350]):
        """image (H,W,1) or (H,W) with levels 0..255 (rounded to the nearest level); returns the shaded levels, float32, same shape."""
        image = np.asarray(image, np.float32)
        H, W = image.shape[:2]
        eng = _engine()
        cfg = {'params': {'additive_shade': dict(nb_ellipses=nb_ellipses, transparency_range=transparency_range,
                                                 kernel_size_range=kernel_size_range)}}
        p = photometric.sample_params(cfg, [next(_calls)], seed, (H, W))
        a = torch.from_numpy(np.clip(np.rint(image), 0, 255).astype(np.uint8).reshape(1, H, W)).to(eng.device)
        up = lambda name: torch.from_numpy(p[name]).to(eng.device)
        out = eng.photo_shade(a, up('ellipses'), up('n_ellipses'), up('taps'), p['ksize'], up('transparency'), up('shade_on'))
        return (out.cpu().numpy() * np.float32(255)).reshape(image.shape)

    def __call__(self, img, **config):
        # as the reference: a missing 'additive_shade' raises KeyError; a falsy one still divides by 255, a second time for an image that
        # ImgAugTransform already returned in [0,1] (utils/photometric.py:111-115)
        if config['photometric']['params']['additive_shade']:
            params = config['photometric']['params']
            img = self.additive_shade(img * 255, **params['additive_shade'])
        return img / 255
