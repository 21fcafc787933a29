"""datasets/ALLSS.py with `gaussian_label.enable` served as the shipped training configuration sets it: ALLSSTrain adds the soft label
maps the reference trains the detector on (datasets/ALLSS.py:229-249) to a batch, made on the GPU (Engine.warp_labels_bi:
libimx_sploop.so).  ALLSS and ALLSSPhotometric stay as they are: both still raise on the flag; this class strips it before they see it.

The reference pushes the bilinear splat `labels_bi` (datasets/data_tools.py:9-34) through ImgAugTransform (utils/photometric.py:72-77):
an 8-bit quantisation, imgaug's GaussianBlur(sigma), and back to float.  The blur itself is NOT restated (OpenCV's fixed-point 8-bit
blur is on no machine of this project).  The flag is served only where the blur is provably the identity on 8-bit images, which
covers the shipped sigma = 0.2: see check_gaussian_label.  What remains is floor(255 w) / 255.  No parity claim against imgaug or OpenCV."""
import copy
import math

from .. import homoadapt, sptrain
from .ALLSS_photo import ALLSSPhotometric

IMGAUG_SIGMA_EPS = 1e-3           # imgaug's blur_gaussian_ returns the image unchanged below this sigma
MAX_DEFECT = 0.25                 # of an 8-bit level


def blur_defect(sigma):
    """255 (1 - w0^2), w0 = 1 / (1 + 2 sum_{x=1..3} exp(-x^2 / 2 sigma^2)) the centre tap of a normalised Gaussian: the 2-D kernel puts
    weight w0^2 on the pixel itself and 1 - w0^2 on the others, whose values lie in [0, 255], so the blurred value differs from the
    pixel's by at most this many levels before rounding.  Below half a level (this module asks for a quarter) the rounded result is
    the pixel itself, whatever the kernel's width beyond three taps a side adds (at the sigmas that pass, under 1e-30)."""
    w0 = 1.0 / (1.0 + 2.0 * sum(math.exp(-x * x / (2.0 * sigma * sigma)) for x in (1, 2, 3)))
    return 255.0 * (1.0 - w0 * w0)


def check_gaussian_label(cfg):
    """cfg = the `gaussian_label` section.  Returns sigma where the flag can be served, otherwise raises NotImplementedError naming the bound."""
    bound = (f"gaussian_label is served only where GaussianBlur is the identity on 8-bit images: params.GaussianBlur.sigma a single number "
             f"below {IMGAUG_SIGMA_EPS} or with 255 (1 - w0^2) <= {MAX_DEFECT} (sigma up to about 0.24; the shipped 0.2 gives 0.0038)")
    sigma = ((cfg.get('params') or {}).get('GaussianBlur') or {}).get('sigma')
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
        raise NotImplementedError(f"{bound}; got sigma = {sigma!r}")
    sigma = float(sigma)
    if not (0 <= sigma < IMGAUG_SIGMA_EPS or blur_defect(sigma) <= MAX_DEFECT):
        raise NotImplementedError(f"{bound}; sigma = {sigma} gives {blur_defect(sigma):.4g}")
    return sigma


class ALLSSTrain(ALLSSPhotometric):
    def __init__(self, export=False, transform=None, task='train', images=None, points=None, device='cuda', **config):
        config = copy.deepcopy(config)
        g = config.get('gaussian_label') or {}
        self.gaussian_label = bool(g.get('enable', False))           # both tasks, as in the reference
        if self.gaussian_label:
            self.gaussian_sigma = check_gaussian_label(g)
            g['enable'] = False
        super().__init__(export=export, transform=transform, task=task, images=images, points=points, device=device, **config)

    def batch(self, indices):
        """ALLSSPhotometric.batch plus, with gaussian_label enabled: labels_2D_gaussian (B,1,H,W) (= labels_2D: 1 -> 255 -> 1) and,
        where warped_pair is enabled, warped_labels_bi (B,1,H,W) (the bilinear splat) and warped_labels_gaussian (B,1,H,W) (its 8-bit
        round trip).  Everything else is the base class's, bit for bit.  No host synchronisation."""
        indices = list(indices)
        out = super().batch(indices)
        self._last_batch = out
        if not self.gaussian_label:
            return out
        out['labels_2D_gaussian'] = out['labels_2D']
        wp = self.config['warped_pair']
        if wp['enable']:
            eng = sptrain.plain_engine(self.device)
            H, W = out['image'].shape[-2:]
            # the host matrices ALLSS.batch warped the hard labels by, drawn again under the same (seed, index): scaled on the host, like them
            hom = [homoadapt.sample_homographies(2, [self.seed, i], **wp['params'])[0][1] for i in indices]
            out['warped_labels_bi'] = eng.warp_labels_bi(out['pts'], out['counts'], hom, H, W, levels=0)[0][:, None]
            out['warped_labels_gaussian'] = eng.warp_labels_bi(out['pts'], out['counts'], hom, H, W, levels=255)[0][:, None]
        return out

    def __getitem__(self, index):
        """The reference's dict for one sample with its three soft-label entries, (1,H,W) host tensors each."""
        out = super().__getitem__(index)                               # (ALLSS.__getitem__ makes the sample through self.batch)
        for k in ('labels_2D_gaussian', 'warped_labels_bi', 'warped_labels_gaussian'):
            if k in self._last_batch:
                out[k] = self._last_batch[k][0].cpu()
        return out
