"""The photometric augmentation on the GPU (imx_photo_pixels, imx_photo_shade, Engine.photo_pixels / photo_shade / photometric and
datasets/ALLSS_photo.py) against the project's restatement of its arithmetic (tests/photometric_ref.py).

photo_pixels with the blur off equals the float64 statement except at EXEMPT pixels, where one level either way is allowed: a pixel is
exempt when noise_scale z of the reference lies within 1e-4 of a half-integer (|noise_scale z| <= 10 sqrt(-2 ln 2^-24) = 57.7, so 1e-4
is 14 float32 ulp there; logf, sqrtf, cospif and three products stay below about 6).  tests/test_photometric_host.py holds every fixture
to at most 2e-3 exempt pixels per image.  With the blur on, the blur of the device's own noisy image equals the float32-order statement
bit for bit.  photo_shade: |out - float64| <= (2 (ksize + 2) + 8) 2^-24 -- two passes of non-negative taps that sum to 1 over values
with |t m / 255| <= 1, one rounding per fma, and the eight roundings of the shading itself -- on outputs in [0,1].  Needs an MI355X; a
few seconds in all."""
import ctypes

import numpy as np
import pytest
import torch

from tests import photometric_ref as R
from tests import util

pytestmark = pytest.mark.gpu
PIXEL_KEYS = ('img', 'lut', 'noise_scale', 'thresh', 'table', 'blur_kernel', 'blur_on', 'key')
SHADE_KEYS = ('img', 'ellipses', 'n_ellipses', 'taps', 'ksize', 'transparency', 'on')


@pytest.fixture(scope="module")
def eng():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


def dev(a, offset=0):
    """the array on the device; uint32 travels as its int32 bit pattern; `offset` elements of the same type in front of it"""
    a = np.ascontiguousarray(a)
    a = a.view(np.int32) if a.dtype == np.uint32 else a
    if not offset:
        return torch.from_numpy(a).to("cuda")
    flat = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
    flat[offset:] = torch.from_numpy(a).to("cuda").reshape(-1)
    return flat[offset:].view(a.shape)


def pick(c, sel):
    """the images `sel` of a case (the shared table stays whole)"""
    return {k: (v if k == 'table' else np.ascontiguousarray(v[list(sel)])) for k, v in c.items()}


def pixels(eng, c, offset=0):
    out = eng.photo_pixels(dev(c['img'], offset), *(dev(c[k]) for k in PIXEL_KEYS[1:]))
    return out.cpu().numpy()


def shade(eng, c, offset=0):
    out = eng.photo_shade(dev(c['img'], offset), dev(c['ellipses']), dev(c['n_ellipses']), dev(c['taps']), c['ksize'], dev(c['transparency']),
                          dev(c['on']))
    return out.cpu().numpy()


def forms_of(eng, fn):
    eng.timing_reset()
    eng.set_timing(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {(name, form) for name, _, _, form in eng.timing_report(forms=True)}
    finally:
        eng.set_timing(False)
        eng.timing_reset()


@pytest.fixture(scope="module")
def shade_refs():
    """case -> the float64 statement of its four images, computed once"""
    out = {}
    for case in R.SHADE_CASES:
        c = R.shade_case(*case)
        out[case] = np.stack([R.shade(c['img'][b], c['ellipses'][b, :c['n_ellipses'][b]], c['taps'][b, :c['ksize'][b]], c['transparency'][b],
                                      bool(c['on'][b])) for b in range(4)])
    return out


@pytest.mark.parametrize("shape", R.PIXEL_SHAPES)
def test_pixels_blur_off_against_float64(eng, shape):
    c = R.pixel_case(shape)
    got = pixels(eng, c)
    B, H, W = shape
    assert got.shape == shape and got.dtype == np.uint8
    for b in range(B):
        ref = R.pixels_noisy(c['img'][b], c['lut'][b], c['noise_scale'][b], c['thresh'][b], c['table'], c['key'][b])
        ex = R.exempt(H, W, c['noise_scale'][b], c['key'][b], R.EXEMPT_DELTA)
        d = np.abs(got[b].astype(int) - ref.astype(int))
        print(f"{shape} image {b}: exempt {ex.mean():.2e}, differing {np.count_nonzero(d)}, largest {d.max()}")
        assert ex.mean() <= R.EXEMPT_CAP
        assert (d[~ex] == 0).all() and (d[ex] <= 1).all()
    if B > 1:       # noise 0, threshold 0, blur off: the table alone
        assert np.array_equal(got[-1], c['lut'][-1][R.quantise(c['img'][-1])])


@pytest.mark.parametrize("kernel", (R.LINE_30, R.DYADIC), ids=("line30", "dyadic"))
@pytest.mark.parametrize("shape", R.PIXEL_SHAPES)
def test_blur_of_the_devices_own_noisy_image_bit_for_bit(eng, shape, kernel):
    c = R.pixel_case(shape)
    noisy = pixels(eng, c)
    c['blur_kernel'] = np.tile(np.asarray(kernel, np.float32), (shape[0], 1))
    c['blur_on'] = np.ones(shape[0], np.int32)
    c['blur_on'][1:2] = 0                       # the second image of a batch stays as it was
    got = pixels(eng, c)
    for b in range(shape[0]):
        want = R.blur3(noisy[b], kernel, np.float32) if c['blur_on'][b] else noisy[b]
        assert np.array_equal(got[b], want), (shape, b)
    if kernel is R.DYADIC:                      # the case does contain exact ties
        acc = sum(np.float32(k) * np.roll(noisy[0].astype(np.float32), s, (0, 1)) for k, s in ((0.25, (1, 1)), (0.5, (0, 0)), (0.25, (-1, -1))))
        assert shape[1] * shape[2] < 100 or (np.modf(acc)[0] == 0.5).any()


@pytest.mark.parametrize("case", R.SHADE_CASES, ids=lambda c: f"k{c[0]}-{c[1]}x{c[2]}")
def test_shade_against_float64(eng, shade_refs, case):
    c = R.shade_case(*case)
    got = shade(eng, c)
    assert got.dtype == np.float32 and got.shape == c['img'].shape
    bound = (2 * (case[0] + 2) + 8) * 2.0 ** -24
    err = np.abs(got.astype(np.float64) - shade_refs[case]).reshape(4, -1).max(1)
    print(f"{case}: largest error / bound per image {err / bound}")
    assert (err <= bound).all()
    plain = c['img'].astype(np.float32) / np.float32(255)
    assert np.array_equal(got[1], plain[1])     # 0 ellipses
    assert np.array_equal(got[3], plain[3])     # on/off word clear
    assert (got[0] != plain[0]).any() and (got[2] != plain[2]).any()


def test_an_image_has_the_bits_it_has_in_any_batch(eng, shade_refs):
    """alone, at another position, and after a larger call on the same handle (stale workspace)"""
    c = R.pixel_case((3, 37, 53))
    c['blur_on'] = np.asarray([1, 0, 1], np.int32)
    whole = pixels(eng, c)
    for b in range(3):
        assert np.array_equal(pixels(eng, pick(c, [b]))[0], whole[b])
    assert np.array_equal(pixels(eng, pick(c, [2, 1, 0])), whole[::-1])
    big, small = R.shade_case(*R.SHADE_CASES[2]), R.shade_case(*R.SHADE_CASES[1])
    small['ksize'] = np.asarray([101, 3, 51, 101], np.int32)                  # ksize differs within the batch: taps beyond it are not read
    whole = shade(eng, small)
    shade(eng, big)
    for b in range(4):
        assert np.array_equal(shade(eng, pick(small, [b]))[0], whole[b])
    shade(eng, big)
    assert np.array_equal(shade(eng, pick(small, [3, 2, 1, 0])), whole[::-1])
    assert np.array_equal(whole[0], shade(eng, R.shade_case(*R.SHADE_CASES[1]))[0])


def test_an_offset_pointer_or_an_odd_width_gives_the_same_bits(eng):
    c = R.pixel_case((2, 64, 64))
    c['blur_on'] = np.asarray([1, 0], np.int32)
    assert forms_of(eng, lambda: pixels(eng, c)) == {("photo_pixels", "x4")}
    assert forms_of(eng, lambda: pixels(eng, c, offset=1)) == {("photo_pixels", "x1")}
    assert np.array_equal(pixels(eng, c), pixels(eng, c, offset=1))
    # an odd width changes the counters (pixel index = y W + x), so it has no aligned twin: the widths 7, 53 and 131 run the dword form
    # against the same statements as the 16-byte form in the tests above
    odd = R.pixel_case((2, 70, 131))
    assert forms_of(eng, lambda: pixels(eng, odd)) == {("photo_pixels", "x1")}
    s = R.shade_case(*R.SHADE_CASES[0])
    assert np.array_equal(shade(eng, s), shade(eng, s, offset=4))


def test_error_codes_launch_nothing(eng):
    from image_matching_amd import _lib
    from image_matching_amd.engine import ImxError
    lib = _lib.load_photo_library()
    assert lib.imx_photo_pixels(None, 1, 8, 8, *([None] * 10)) != 0
    assert lib.imx_photo_shade(None, 1, 8, 8, 1, 3, *([None] * 9)) != 0
    s = pick(R.shade_case(*R.SHADE_CASES[0]), [0, 1])
    for bad, text in ((4, "ksize"), (5, "ksize"), (1, "ksize")):                # even; above Kcap = 3; below 3
        s['ksize'] = np.asarray([3, bad], np.int32)
        with pytest.raises(ImxError, match=text):
            shade(eng, s)
    with pytest.raises(ImxError, match="shape"):
        eng.photo_pixels(torch.zeros(1, 1, 8, device="cuda"), *(dev(pick(R.pixel_case((1, 5, 7)), [0])[k]) for k in PIXEL_KEYS[1:]))
    # an output that aliases an input, through the C ABI
    c = R.pixel_case((1, 5, 7))
    t = {k: dev(c[k]) for k in PIXEL_KEYS}
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = t['img'].clone()
    rc = lib.imx_photo_pixels(eng.handle, 1, 5, 7, *(ptr(t[k]) for k in PIXEL_KEYS), ptr(t['img']), stream)
    assert rc != 0 and b"aliases" in eng.lib.imx_last_error(eng.handle)
    s = R.shade_case(*R.SHADE_CASES[0])
    out = torch.full((4, 24, 40), 7.0, device="cuda")
    ks = np.ascontiguousarray(s['ksize'])
    held = {k: dev(s[k]) for k in SHADE_KEYS if k != 'ksize'}
    args = [ptr(held[k]) if k != 'ksize' else ks.ctypes.data_as(ctypes.c_void_p) for k in SHADE_KEYS]
    ks[2] = 4
    assert lib.imx_photo_shade(eng.handle, 4, 24, 40, 20, 3, *args, ptr(out), stream) != 0
    ks[2] = 3
    assert lib.imx_photo_shade(eng.handle, 4, 24, 40, 20, 3, *args[:6], ptr(out), ptr(out), stream) != 0        # out aliases `on`
    assert b"aliases" in eng.lib.imx_last_error(eng.handle)
    torch.cuda.synchronize()
    assert torch.equal(t['img'], before) and (out == 7.0).all()


def allss_sets(H, W, photo):
    from image_matching_amd import synth
    from image_matching_amd.datasets.ALLSS import ALLSS
    from image_matching_amd.datasets.ALLSS_photo import ALLSSPhotometric
    rng = np.random.default_rng(5)
    images = np.stack([synth.synth_pair(i, H, W)[0] for i in range(3)]).astype(np.float32)
    points = [np.stack([rng.uniform(0, W - 1, 30), rng.uniform(0, H - 1, 30)], 1).astype(np.float32) for _ in range(3)]
    warp = {'enable': True, 'valid_border_margin': 3,
            'params': dict(translation=True, rotation=True, scaling=True, perspective=True, scaling_amplitude=0.2, perspective_amplitude_x=0.2,
                           perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=1.57, allow_artifacts=True)}
    plain = ALLSS(task='train', images=images, points=points, warped_pair=warp)
    aug = ALLSSPhotometric(task='train', images=images, points=points, warped_pair=warp, augmentation={'photometric': photo})
    return plain, aug


SHIPPED_PHOTO = {'enable': True, 'primitives': ['random_brightness', 'random_contrast', 'additive_speckle_noise', 'additive_gaussian_noise',
                                                'additive_shade', 'motion_blur'],
                 'params': {'random_brightness': {'max_abs_change': 50}, 'random_contrast': {'strength_range': [0.5, 1.5]},
                            'additive_gaussian_noise': {'stddev_range': [0, 10]}, 'additive_speckle_noise': {'prob_range': [0, 0.0035]},
                            'additive_shade': {'transparency_range': [-0.5, 0.5], 'kernel_size_range': [100, 150]},
                            'motion_blur': {'max_kernel_size': 3}}}
IDENTITY_PHOTO = {'enable': True, 'primitives': 'all',
                  'params': {'random_brightness': {'max_abs_change': 0}, 'random_contrast': {'strength_range': [1.0, 1.0]},
                             'additive_gaussian_noise': {'stddev_range': [0, 0]}, 'additive_speckle_noise': {'prob_range': [0, 0]},
                             'additive_shade': {'transparency_range': [0.0, 0.0], 'kernel_size_range': [100, 150]}}}


def test_allss_photometric_batch(eng):
    from image_matching_amd.sptrain_model import SuperPointTrainable
    H, W = 120, 160
    plain, aug = allss_sets(H, W, SHIPPED_PHOTO)
    a, b = plain.batch(range(3)), aug.batch(range(3))
    assert set(a) == set(b)
    for k in a:
        if k in ('image', 'warped_img'):
            assert b[k].shape == a[k].shape and b[k].dtype == torch.float32
            assert not torch.equal(a[k], b[k]) and float(b[k].min()) >= 0.0 and float(b[k].max()) <= 1.0
        elif isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k       # labels, masks, homographies: bit for bit
        else:
            assert a[k] == b[k], k
    # the same draws again; the two images of a sample are drawn separately
    again = aug.batch(range(3))
    assert torch.equal(again['image'], b['image']) and torch.equal(again['warped_img'], b['warped_img'])
    from image_matching_amd import photometric
    p0, p1 = (photometric.sample_params(aug.photo_config, [(i, w) for i in range(3)], aug.seed, (H, W)) for w in (0, 1))
    assert not np.array_equal(p0['key'], p1['key']) and not np.array_equal(p0['lut'], p1['lut'])
    assert torch.equal(aug.batch([1])['image'][0], b['image'][1])            # a sample's bits do not depend on the batch it is in
    # every range collapsed to the identity: the quantisation alone
    _, ident = allss_sets(H, W, IDENTITY_PHOTO)
    c = ident.batch(range(3))
    for k in ('image', 'warped_img'):
        assert float((c[k] - a[k]).abs().max()) <= 1.0 / 255
    # task='val' is not augmented
    from image_matching_amd.datasets.ALLSS_photo import ALLSSPhotometric
    val = ALLSSPhotometric(task='val', images=plain._images, points=plain._points, warped_pair=plain.config['warped_pair'],
                           augmentation={'photometric': SHIPPED_PHOTO})
    assert torch.equal(val.batch(range(3))['image'], a['image'])
    torch.manual_seed(0)
    net = SuperPointTrainable(eng, descriptor_length=128).train()
    with torch.no_grad():
        out = net(b['image'])
    assert torch.isfinite(out['semi']).all() and torch.isfinite(out['desc']).all()
