"""Photometric augmentation of SuperPoint's training data (the reference's utils/photometric.py, applied by datasets/ALLSS.py:116-128),
host plumbing: the per-image random PARAMETERS, drawn here from `augmentation.photometric.params`, and the small tables the kernels of
libimx_photo.so take (include/imx_photo.h).  Every per-pixel draw happens in the kernel.

The draws are valid samples of the reference's distributions but NOT its stream (imgaug and numpy's global generator): unpinned, like
homoadapt.sample_homographies.  Each image has a generator of its own, seeded with (seed, id), so its parameters and its Philox key do
not depend on the batch it is drawn in."""
import numpy as np

STAGES = ('random_brightness', 'random_contrast', 'additive_gaussian_noise', 'additive_speckle_noise', 'motion_blur', 'additive_shade')
KSIZE_MAX = 351          # include/imx_photo.h: the reference's default kernel_size_range ends at 350, made odd


def replacement_table():
    """The 256 quantiles of imgaug's impulse value Beta(1/2, 1/2) * 255 (iaa.ImpulseNoise = SaltAndPepper), at (j + 1/2) / 256: the
    arcsine law's quantile function is sin^2(pi u / 2)."""
    j = np.arange(256, dtype=np.float64)
    return np.rint(255.0 * np.sin(np.pi * (j + 0.5) / 512.0) ** 2).astype(np.uint8)


def compose_lut(delta, alpha):
    """iaa.Add(delta) then iaa.LinearContrast(alpha) on the 256 levels as one table, in float32:
    trunc(clip(127 + alpha (clip(q + delta, 0, 255) - 127), 0, 255))."""
    f = np.float32
    q = np.clip(np.arange(256, dtype=f) + f(delta), f(0), f(255))
    return np.clip(f(127) + f(alpha) * (q - f(127)), f(0), f(255)).astype(np.uint8)


def gaussian_taps(ksize):
    """cv2.getGaussianKernel(ksize, 0): sigma = 0.3 ((ksize - 1) / 2 - 1) + 0.8, exp(-x^2 / (2 sigma^2)) normalised in float64, as fp32."""
    ksize = int(ksize)
    if ksize < 3 or ksize > KSIZE_MAX or ksize % 2 == 0:
        raise ValueError(f"ksize must be odd and in [3, {KSIZE_MAX}], got {ksize}")
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1.0) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def motion_kernel(angle_deg):
    """iaa.MotionBlur(3)'s kernel: the vertical line through the centre of a 3x3 matrix, rotated about the centre by the angle with
    bilinear weights (zero outside), normalised to sum 1.  Row-major (9,) fp32."""
    t = np.deg2rad(float(angle_deg))
    c, s = np.cos(t), np.sin(t)
    line = np.zeros((3, 3))
    line[:, 1] = 1.0
    k = np.zeros((3, 3))
    for y in range(3):
        for x in range(3):
            u, v = x - 1.0, y - 1.0
            sx, sy = c * u + s * v + 1.0, -s * u + c * v + 1.0        # the source position of this output element
            x0, y0 = int(np.floor(sx)), int(np.floor(sy))
            for yy, wy in ((y0, 1.0 - (sy - y0)), (y0 + 1, sy - y0)):
                for xx, wx in ((x0, 1.0 - (sx - x0)), (x0 + 1, sx - x0)):
                    if 0 <= xx < 3 and 0 <= yy < 3:
                        k[y, x] += wy * wx * line[yy, xx]
    return (k / k.sum()).astype(np.float32).reshape(9)


def _enabled(config, name):
    prim = config.get('primitives', 'all')
    return bool(config.get('params', {}).get(name, False)) and (prim == 'all' or name in prim)


def sample_params(config, ids, seed, shape):
    """Per-image parameters for Engine.photometric: `config` is the `augmentation.photometric` dict ('params', 'primitives'), `ids` one
    id per image (an int or a tuple of ints: image b draws from numpy's default_rng([seed, *id])), `shape` = (H, W) of the images (the
    ellipses of the shade are placed in it).  A stage that is not in `params`, or not in `primitives`, gets its identity.  Returns a
    dict of host arrays: lut (B,256) u8, noise_scale (B) f32, thresh (B) u32, table (256) u8, blur_kernel (B,9) f32, blur_on (B) i32,
    key (B,2) u32, ellipses (B,E,5) f32, n_ellipses (B) i32, taps (B,Kcap) f32, ksize (B) i32, transparency (B) f32, shade_on (B) i32."""
    H, W = int(shape[0]), int(shape[1])
    par = config.get('params', {})
    on = {name: _enabled(config, name) for name in STAGES}
    if on['motion_blur'] and int(par['motion_blur']['max_kernel_size']) != 3:
        raise NotImplementedError("motion_blur.max_kernel_size other than 3: the kernel correlates with a 3x3 matrix only (the reference "
                                  "itself builds no augmenter for a larger value)")
    shade = dict(nb_ellipses=20, transparency_range=[-0.5, 0.8], kernel_size_range=[250, 350])       # additive_shade's defaults
    if on['additive_shade'] and isinstance(par['additive_shade'], dict):
        shade.update(par['additive_shade'])
    B = len(ids)
    E = max(1, int(shade['nb_ellipses'])) if on['additive_shade'] else 1
    out = {'lut': np.zeros((B, 256), np.uint8), 'noise_scale': np.zeros(B, np.float32), 'thresh': np.zeros(B, np.uint32),
           'table': replacement_table(), 'blur_kernel': np.zeros((B, 9), np.float32), 'blur_on': np.zeros(B, np.int32),
           'key': np.zeros((B, 2), np.uint32), 'ellipses': np.zeros((B, E, 5), np.float32), 'n_ellipses': np.zeros(B, np.int32),
           'ksize': np.full(B, 3, np.int32), 'transparency': np.zeros(B, np.float32), 'shade_on': np.zeros(B, np.int32)}
    out['blur_kernel'][:, 4] = 1.0
    taps = []
    for b, ident in enumerate(ids):
        rng = np.random.default_rng([int(seed)] + [int(i) for i in np.atleast_1d(ident)])
        out['key'][b] = rng.integers(0, 2 ** 32, 2, dtype=np.uint64).astype(np.uint32)
        delta, alpha = 0, 1.0
        if on['random_brightness']:
            c = int(par['random_brightness']['max_abs_change'])
            delta = int(rng.integers(-c, c + 1))
        if on['random_contrast']:
            alpha = rng.uniform(*par['random_contrast']['strength_range'])
        out['lut'][b] = compose_lut(delta, alpha)
        if on['additive_gaussian_noise']:
            out['noise_scale'][b] = rng.uniform(*par['additive_gaussian_noise']['stddev_range'])
        if on['additive_speckle_noise']:
            out['thresh'][b] = int(np.ceil(rng.uniform(*par['additive_speckle_noise']['prob_range']) * 2 ** 24))
        if on['motion_blur'] and rng.random() < 0.5:
            out['blur_on'][b] = 1
            out['blur_kernel'][b] = motion_kernel(rng.uniform(0.0, 360.0))
        if on['additive_shade']:                      # utils/photometric.py:88-100
            min_dim = min(H, W) / 4
            n = int(shade['nb_ellipses'])
            for i in range(n):
                ax = int(max(rng.random() * min_dim, min_dim / 5))
                ay = int(max(rng.random() * min_dim, min_dim / 5))
                max_rad = max(ax, ay)
                x = rng.integers(max_rad, W - max_rad)
                y = rng.integers(max_rad, H - max_rad)
                out['ellipses'][b, i] = (x, y, ax, ay, rng.random() * 90)
            out['n_ellipses'][b] = n
            out['transparency'][b] = rng.uniform(*shade['transparency_range'])
            k = int(rng.integers(*shade['kernel_size_range']))
            k += 1 - k % 2                            # kernel_size has to be odd
            if k < 3 or k > KSIZE_MAX:
                raise ValueError(f"additive_shade.kernel_size_range gives ksize {k}: outside [3, {KSIZE_MAX}]")
            out['ksize'][b] = k
            out['shade_on'][b] = 1
        taps.append(gaussian_taps(out['ksize'][b]))
    out['taps'] = np.zeros((B, int(out['ksize'].max()) if B else 3), np.float32)
    for b, t in enumerate(taps):
        out['taps'][b, :len(t)] = t
    return out
