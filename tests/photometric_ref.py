"""The project's own statement of what the kernels of csrc/photo_aug.hip compute (include/imx_photo.h): Philox4x32-10
in numpy integers, every stage in float64, and the 3x3 blur also in the stated float32 order.  One image at a time.  Neither imgaug nor
OpenCV is on any machine of this project, so this file restates their published arithmetic; it is not a parity claim."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter (...,4) and key (2,) or (...,2) of unsigned 32-bit values -> (...,4) uint32 (Salmon et al., SC'11; Random123)."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64) & MASK32, c.shape[:-1] + (2,))
    x0, x1, x2, x3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0, p1 = np.uint64(M0) * x0, np.uint64(M1) * x2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
        x0, x1, x2, x3 = hi1 ^ x1 ^ k0, lo1, hi0 ^ x3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack([x0, x1, x2, x3], axis=-1).astype(np.uint32)


def pixel_draws(H, W, key):
    """(H,W,4) uint32: the draws of every pixel of an image, counter (y W + x, 0, 0, 0)"""
    idx = np.arange(H * W, dtype=np.uint64)
    ctr = np.stack([idx & MASK32, idx >> np.uint64(32), np.zeros_like(idx), np.zeros_like(idx)], axis=-1)
    return philox4x32_10(ctr, key).reshape(H, W, 4)


def reflect101(i, n):
    """cv::BORDER_REFLECT_101 of integer index arrays, any number of bounces; n >= 2"""
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def quantise(img):
    """(img * 255).astype(uint8) on [0,1]: the float32 product, clamped, truncated"""
    return np.clip(np.asarray(img, np.float32) * np.float32(255), 0, 255).astype(np.uint8)


def noise_value(H, W, noise_scale, key):
    """noise_scale z in float64, z = sqrt(-2 ln u1) cos(2 pi u2), per pixel: what step 3 rounds"""
    r = pixel_draws(H, W, key).astype(np.float64)
    u1 = (np.floor(r[..., 0] / 256) + 1) / 2 ** 24
    u2 = np.floor(r[..., 1] / 256) / 2 ** 24
    return float(np.float32(noise_scale)) * np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)


def exempt(H, W, noise_scale, key, delta=1e-4):
    """(H,W) bool: noise_scale z lies within delta of a half-integer, where float32 may round the other way"""
    v = noise_value(H, W, noise_scale, key)
    return np.abs(v - np.floor(v) - 0.5) < delta


def pixels_noisy(img, lut, noise_scale, thresh, table, key):
    """steps 1 to 4 of imx_photo_pixels for one image (H,W) -> uint8"""
    H, W = img.shape
    r = pixel_draws(H, W, key)
    a = np.asarray(lut, np.uint8)[quantise(img)].astype(np.float64)
    a = np.clip(a + np.rint(noise_value(H, W, noise_scale, key)), 0, 255)
    hit = (r[..., 2] >> np.uint32(8)) < np.uint32(thresh)
    return np.where(hit, np.asarray(table, np.uint8)[r[..., 3] >> np.uint32(24)], a).astype(np.uint8)


def blur3(noisy, kernel, dtype=np.float32):
    """step 5: the uint8 image correlated with the 3x3 kernel under BORDER_REFLECT_101, taps in row-major order, one product and one add
    per tap from +0 in `dtype`, then round to nearest even, saturated"""
    H, W = noisy.shape
    k = np.asarray(kernel, np.float32).reshape(3, 3).astype(dtype)
    src = noisy.astype(dtype)
    ys, xs = np.arange(H), np.arange(W)
    acc = np.zeros((H, W), dtype)
    for dy in range(3):
        for dx in range(3):
            tap = src[reflect101(ys + dy - 1, H)][:, reflect101(xs + dx - 1, W)]
            acc = (acc + (k[dy, dx] * tap).astype(dtype)).astype(dtype)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def ellipse_form(H, W, ellipses):
    """(n,H,W) float64: ((dx cos + dy sin) / ax)^2 + ((dy cos - dx sin) / ay)^2 of every pixel for every ellipse (cx, cy, ax, ay, degrees)"""
    e = np.asarray(ellipses, np.float32).astype(np.float64).reshape(-1, 5)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    t = np.pi * (e[:, 4] / 180.0)
    cs, sn = np.cos(t)[:, None, None], np.sin(t)[:, None, None]
    dx, dy = x[None] - e[:, 0, None, None], y[None] - e[:, 1, None, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        u, v = (dx * cs + dy * sn) / e[:, 2, None, None], (dy * cs - dx * sn) / e[:, 3, None, None]
        return u * u + v * v


def shade_mask(H, W, ellipses):
    """255 inside the union of the ellipses, 0 elsewhere"""
    f = ellipse_form(H, W, ellipses)
    return np.where((f <= 1.0).any(axis=0), 255.0, 0.0) if len(f) else np.zeros((H, W))


def blur_separable(m, taps):
    """rows, then columns, BORDER_REFLECT_101, float64"""
    t = np.asarray(taps, np.float32).astype(np.float64)
    k = len(t)
    H, W = m.shape
    cols = reflect101(np.arange(W)[:, None] + np.arange(k)[None] - k // 2, W)       # (W,k)
    rows = reflect101(np.arange(H)[:, None] + np.arange(k)[None] - k // 2, H)       # (H,k)
    r = (m[:, cols] * t).sum(-1)
    return (r[rows, :] * t[None, :, None]).sum(1)


def shade(a_u8, ellipses, taps, transparency, on=True):
    """imx_photo_shade for one image in float64: a_u8 (H,W) uint8, ellipses (n,5) (the image's own count of them), taps (ksize,)"""
    a = a_u8.astype(np.float64)
    if not on:
        return a / 255
    H, W = a.shape
    m = blur_separable(shade_mask(H, W, ellipses), taps)
    return np.clip(a * (1 - float(np.float32(transparency)) * m / 255), 0, 255) / 255


# ---------------------------------------------------------------------------------------------------------------- fixtures of the GPU tests
# (tests/test_gpu_photometric.py runs them; tests/test_photometric_host.py checks, from this file alone, that each stays under the cap of
# exempt pixels and that no pixel of a shade fixture sits on an ellipse's boundary)

PIXEL_SHAPES = ((1, 5, 7), (3, 37, 53), (2, 70, 131), (2, 64, 64))
PIXEL_SEEDS = {(1, 5, 7): 1, (3, 37, 53): 2, (2, 70, 131): 3, (2, 64, 64): 4}
EXEMPT_DELTA, EXEMPT_CAP = 1e-4, 2e-3
BOUNDARY_MARGIN = 1e-9
SHADE_CASES = ((3, 24, 40), (101, 24, 40), (151, 120, 160), (351, 64, 96))      # (ksize, H, W)
LINE_30 = (0.0, 0.16277118, 0.13084322, 0.04361441, 0.32554236, 0.04361441, 0.13084322, 0.16277118, 0.0)   # photometric.motion_kernel(30)
DYADIC = (0.25, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.25)                          # exact ties: sums are multiples of 1/4


def pixel_case(shape, seed=None):
    """Inputs of imx_photo_pixels with blur off: per-image parameters differ within the batch; the LAST image of a batch of two or more
    has noise 0 and threshold 0 (its output is lut[q]).  A few pixels sit at 0 and 1."""
    B, H, W = shape
    rng = np.random.default_rng(PIXEL_SEEDS[shape] if seed is None else seed)
    img = rng.random((B, H, W), dtype=np.float32)
    img.reshape(-1)[:3] = (0.0, 1.0, 0.5)
    c = {'img': img, 'lut': rng.integers(0, 256, (B, 256)).astype(np.uint8), 'noise_scale': rng.uniform(0.5, 10.0, B).astype(np.float32),
         'thresh': np.ceil(rng.uniform(0.0, 0.05, B) * 2 ** 24).astype(np.uint32), 'table': rng.integers(0, 256, 256).astype(np.uint8),
         'blur_kernel': np.tile(np.asarray(LINE_30, np.float32), (B, 1)), 'blur_on': np.zeros(B, np.int32),
         'key': rng.integers(0, 2 ** 32, (B, 2), dtype=np.uint64).astype(np.uint32)}
    if B > 1:
        c['noise_scale'][-1], c['thresh'][-1] = 0.0, 0
    return c


def shade_case(ksize, H, W):
    """Inputs of imx_photo_shade, four images: 20 ellipses drawn as utils/photometric.py:88-100 draws them, 0 ellipses, one ellipse that
    covers the image, and 20 ellipses with the on/off word clear.  Taps: cv2.getGaussianKernel(ksize, 0)'s formula, normalised in float64."""
    rng = np.random.default_rng(1000 + ksize)
    B, E = 4, 20
    ell = np.zeros((B, E, 5), np.float32)
    min_dim = min(H, W) / 4
    for b in (0, 3):
        i = 0
        while i < E:
            ax, ay = (int(max(rng.random() * min_dim, min_dim / 5)) for _ in range(2))
            r = max(ax, ay)
            ell[b, i] = (rng.integers(r, W - r), rng.integers(r, H - r), ax, ay, rng.random() * 90)
            # an ellipse with a pixel within BOUNDARY_MARGIN of its boundary is drawn again: there the decision rests on the last bit of
            # sin and cos (a circle through a lattice point, say), which no two libraries need to share
            i += int(np.abs(ellipse_form(H, W, ell[b, i]) - 1.0).min() > BOUNDARY_MARGIN)
    ell[2, 0] = (W / 2, H / 2, H + W, H + W, 30.0)
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1.0) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return {'img': rng.integers(0, 256, (B, H, W)).astype(np.uint8), 'ellipses': ell, 'n_ellipses': np.asarray([20, 0, 1, 20], np.int32),
            'taps': np.tile((g / g.sum()).astype(np.float32), (B, 1)), 'ksize': np.full(B, ksize, np.int32),
            'transparency': np.asarray([0.8, 0.5, -0.5, 0.3], np.float32), 'on': np.asarray([1, 1, 1, 0], np.int32)}


# ---------------------------------------------------------------------------------------------------------------- workload-size cases
# (tests/test_gpu_sp_workload_paths.py runs them; tests/test_sp_workload_paths_host.py checks what they promise.)  The lists above stay
# as they are: host tests and fixtures hang on them.

def gaussian_taps(ksize):
    """cv2.getGaussianKernel(ksize, 0)'s formula, normalised in float64, as shade_case forms its taps"""
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1.0) + 0.8
    x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def _draw_ellipses(rng, H, W, E, draw):
    """E ellipses from draw(i) -> (cx, cy, ax, ay, degrees); one with a pixel within BOUNDARY_MARGIN of its boundary is drawn again"""
    ell, i = np.zeros((E, 5), np.float32), 0
    while i < E:
        ell[i] = draw(i)
        i += int(np.abs(ellipse_form(H, W, ell[i]) - 1.0).min() > BOUNDARY_MARGIN)
    return ell


def shade_case_wide(ksize, H, W, first_column=256):
    """The four images of shade_case -- 20 ellipses, 0 ellipses, one ellipse that covers the image, 20 ellipses with the on/off word
    clear -- for images wider than one row segment of the row pass and only a few rows high.  shade_case cannot draw those: with
    min(H, W) / 4 < 2 its integer axes are 0 or 1, and a circle of radius 1 about a lattice point always has pixels on its boundary, so
    its redraw rule never ends.  Here the axes are real numbers and the centres lie anywhere in the image.  Ellipse 0 of images 0 and 3
    is small and centred so that every pixel of it lies in a column >= first_column."""
    rng = np.random.default_rng(2000 + ksize)
    B, E = 4, 20
    assert W > first_column
    ell = np.zeros((B, E, 5), np.float32)
    far = max(0.95, min(H, W - first_column) / 2.5)

    def draw(i):
        if i == 0:                                                  # a radius below 1 about a lattice point: that pixel alone
            ax, ay = rng.uniform(0.6, far, 2)
            r = int(max(ax, ay))
            return rng.integers(first_column + r, W - r), rng.integers(0, H), ax, ay, rng.random() * 90
        ax, ay = rng.uniform(0.6, max(H, W) / 32, 2)
        return rng.integers(0, W), rng.integers(0, H), ax, ay, rng.random() * 90
    for b in (0, 3):
        ell[b] = _draw_ellipses(rng, H, W, E, draw)
    ell[2, 0] = (W / 2, H / 2, H + W, H + W, 30.0)
    return {'img': rng.integers(1, 256, (B, H, W)).astype(np.uint8), 'ellipses': ell, 'n_ellipses': np.asarray([20, 0, 1, 20], np.int32),
            'taps': np.tile(gaussian_taps(ksize), (B, 1)), 'ksize': np.full(B, ksize, np.int32),
            'transparency': np.asarray([0.8, 0.5, -0.5, 0.3], np.float32), 'on': np.asarray([1, 1, 1, 0], np.int32)}


SHADE_BATCH_KSIZES = (3, 51, 101)


def shade_batch_case(B, H, W, off=(), empty=()):
    """B images for one imx_photo_shade call: ksize cycles through SHADE_BATCH_KSIZES (neighbours always differ, and an image's ksize
    differs from that of the image 64 or 128 places before it), the taps beyond an image's ksize are NaN (never read), 20 ellipses drawn
    as shade_case draws them, transparency in +-[0.2, 0.8]; the images `off` have the on/off word clear, the images `empty` 0 ellipses."""
    rng = np.random.default_rng(3000 + B)
    E, kcap = 20, max(SHADE_BATCH_KSIZES)
    min_dim = min(H, W) / 4
    ell = np.zeros((B, E, 5), np.float32)

    def draw(i):
        ax, ay = (int(max(rng.random() * min_dim, min_dim / 5)) for _ in range(2))
        r = max(ax, ay)
        return rng.integers(r, W - r), rng.integers(r, H - r), ax, ay, rng.random() * 90
    ksize = np.asarray([SHADE_BATCH_KSIZES[b % 3] for b in range(B)], np.int32)
    taps = np.full((B, kcap), np.nan, np.float32)
    for b in range(B):
        ell[b] = _draw_ellipses(rng, H, W, E, draw)
        taps[b, :ksize[b]] = gaussian_taps(int(ksize[b]))
    n_ell, on = np.full(B, E, np.int32), np.ones(B, np.int32)
    n_ell[list(empty)], on[list(off)] = 0, 0
    return {'img': rng.integers(1, 256, (B, H, W)).astype(np.uint8), 'ellipses': ell, 'n_ellipses': n_ell, 'taps': taps, 'ksize': ksize,
            'transparency': (rng.uniform(0.2, 0.8, B) * rng.choice([-1.0, 1.0], B)).astype(np.float32), 'on': on}


def shade_one(c, b, dtype=np.float64):
    """image b of a shade case through shade (float64) or shade_f32"""
    fn = shade if dtype == np.float64 else shade_f32
    return fn(c['img'][b], c['ellipses'][b, :c['n_ellipses'][b]], c['taps'][b, :c['ksize'][b]], c['transparency'][b], bool(c['on'][b]))


def _fma32(a, b, c):
    """round32(a b + c) of float32 arrays: the product is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def shade_f32(a_u8, ellipses, taps, transparency, on=True):
    """imx_photo_shade for one image in the float32 order DESIGN.md section 21 states: the mask decided in float64, each blur pass one
    fused multiply-add per tap from +0 with the taps ascending, rows before columns, then 1 - t m / 255 and the product, the clamp and
    the division by 255, each operation rounded to float32 on its own"""
    f = np.float32
    a = a_u8.astype(f)
    if not on:
        return a / f(255)
    H, W = a.shape
    t = np.asarray(taps, f)
    k = len(t)
    m = shade_mask(H, W, ellipses).astype(f)
    cols = reflect101(np.arange(W)[:, None] + np.arange(k)[None] - k // 2, W)
    rows = reflect101(np.arange(H)[:, None] + np.arange(k)[None] - k // 2, H)
    r = np.zeros((H, W), f)
    for j in range(k):
        r = _fma32(np.broadcast_to(t[j], (H, W)), m[:, cols[:, j]], r)
    s = np.zeros((H, W), f)
    for j in range(k):
        s = _fma32(np.broadcast_to(t[j], (H, W)), r[rows[:, j], :], s)
    v = (a / f(255)) * f(255)
    scale = f(1) - (f(transparency) * s) / f(255)
    return np.clip(v * scale, f(0), f(255)) / f(255)
