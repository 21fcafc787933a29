"""The host side of the photometric augmentation: Philox4x32-10 of tests/photometric_ref.py against Random123's known answers, the
parameter sampler's ranges and tables (image_matching_amd.photometric), the import swap's signatures, ALLSSPhotometric's constructor, and
what the GPU tests take for granted about their own fixtures -- the share of exempt pixels and the distance of every pixel from every
ellipse's boundary, both computed from the reference alone.  No GPU."""
import inspect

import numpy as np
import pytest

from tests import photometric_ref as R

SHIPPED = {'enable': True, 'primitives': 'all',
           'params': {'random_brightness': {'max_abs_change': 50}, 'random_contrast': {'strength_range': [0.5, 1.5]},
                      'additive_gaussian_noise': {'stddev_range': [0, 10]}, 'additive_speckle_noise': {'prob_range': [0, 0.0035]},
                      'additive_shade': {'transparency_range': [-0.5, 0.5], 'kernel_size_range': [100, 150]},
                      'motion_blur': {'max_kernel_size': 3}}}


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        assert tuple(int(v) for v in R.philox4x32_10(ctr, key)) == want
    both = R.philox4x32_10([kat[0][0], kat[2][0]], [kat[0][1], kat[2][1]])      # vectorised, a key per counter
    assert [tuple(int(v) for v in row) for row in both] == [kat[0][2], kat[2][2]]
    assert tuple(int(v) for v in R.pixel_draws(2, 3, (0, 0))[0, 0]) == kat[0][2]


def test_lut_edges_and_tables():
    from image_matching_amd import photometric as P
    q = np.arange(256)
    assert np.array_equal(P.compose_lut(0, 1.0), q)
    assert np.array_equal(P.compose_lut(50, 1.0), np.minimum(q + 50, 255))
    assert np.array_equal(P.compose_lut(-50, 1.0), np.maximum(q - 50, 0))
    assert np.array_equal(P.compose_lut(0, 0.5), np.trunc(127 + 0.5 * (q - 127.0)))          # exact in float32: halves
    assert np.array_equal(P.compose_lut(0, 1.5), np.trunc(np.clip(127 + 1.5 * (q - 127.0), 0, 255)))
    lut = P.compose_lut(50, 1.5)                                                            # both clips at work
    assert lut[0] == int(127 + 1.5 * (50 - 127)) and lut[255] == 255 and (np.diff(lut.astype(int)) >= 0).all()
    assert P.compose_lut(-50, 0.5)[0] == int(127 - 0.5 * 127) and P.compose_lut(-50, 0.5)[255] == int(127 + 0.5 * (205 - 127))
    table = P.replacement_table()
    assert table.dtype == np.uint8 and table[0] == 0 and table[255] == 255 and (np.diff(table.astype(int)) >= 0).all()
    assert np.array_equal(table, 255 - table[::-1])                                         # the arcsine law is symmetric
    for k in (3, 101, 151, 351):
        t = P.gaussian_taps(k)
        assert t.dtype == np.float32 and len(t) == k and abs(float(t.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.array_equal(t, t[::-1]) and (t >= 0).all() and t.argmax() == k // 2
    for bad in (2, 4, 353, 1):
        with pytest.raises(ValueError):
            P.gaussian_taps(bad)
    assert np.allclose(P.motion_kernel(30.0), R.LINE_30, atol=1e-7)
    for angle in (0.0, 30.0, 77.0, 180.0, 301.5):
        k = P.motion_kernel(angle)
        assert k.shape == (9,) and abs(float(k.sum()) - 1.0) < 1e-6 and (k >= 0).all() and np.allclose(k, k[::-1], atol=1e-7)
    assert np.allclose(P.motion_kernel(0.0).reshape(3, 3)[:, 1], 1 / 3)


def test_sampler_ranges_and_independence():
    from image_matching_amd import photometric as P
    ids = [(i, w) for i in range(40) for w in (0, 1)]
    p = P.sample_params(SHIPPED, ids, 0, (240, 320))
    B = len(ids)
    assert p['lut'].shape == (B, 256) and p['lut'].dtype == np.uint8 and p['table'].shape == (256,)
    assert p['noise_scale'].dtype == np.float32 and (p['noise_scale'] >= 0).all() and (p['noise_scale'] <= 10).all()
    assert p['thresh'].dtype == np.uint32 and (p['thresh'] <= np.ceil(0.0035 * 2 ** 24)).all() and p['thresh'].max() > 0
    assert p['key'].shape == (B, 2) and p['key'].dtype == np.uint32 and len({tuple(k) for k in p['key']}) == B
    assert set(np.unique(p['blur_on'])) == {0, 1} and np.allclose(p['blur_kernel'].sum(1), 1.0, atol=1e-6)
    assert (p['ksize'] % 2 == 1).all() and (p['ksize'] >= 101).all() and (p['ksize'] <= 151).all()
    assert p['taps'].shape == (B, p['ksize'].max()) and np.allclose(p['taps'].astype(np.float64).sum(1), 1.0, atol=1e-6)
    assert (np.abs(p['transparency']) <= 0.5).all() and (p['n_ellipses'] == 20).all() and (p['shade_on'] == 1).all()
    e = p['ellipses']
    assert e.shape == (B, 20, 5) and (e[..., 2:4] >= 12).all() and (e[..., 2:4] <= 60).all() and (e[..., 4] >= 0).all() and (e[..., 4] < 90).all()
    r = e[..., 2:4].max(-1)
    assert (e[..., 0] >= r).all() and (e[..., 0] < 320 - r).all() and (e[..., 1] >= r).all() and (e[..., 1] < 240 - r).all()
    # an image's parameters depend on (seed, id) alone: not on the batch, not on its place in it
    one = P.sample_params(SHIPPED, [ids[5]], 0, (240, 320))
    for k in p:
        if k == 'table':
            continue
        width = one[k].shape[1] if k == 'taps' else None
        assert np.array_equal(one[k][0], p[k][5][:width] if width else p[k][5]), k
    assert not np.array_equal(P.sample_params(SHIPPED, [ids[5]], 1, (240, 320))['key'], one['key'])
    # primitives select the stages; an unselected stage is the identity
    few = P.sample_params(dict(SHIPPED, primitives=['random_brightness']), ids[:4], 0, (240, 320))
    assert not few['noise_scale'].any() and not few['thresh'].any() and not few['blur_on'].any() and not few['shade_on'].any()
    assert all(any(np.array_equal(l, P.compose_lut(d, 1.0)) for d in range(-50, 51)) for l in few['lut'])
    none = P.sample_params({'params': {}}, ids[:2], 0, (240, 320))
    assert np.array_equal(none['lut'][0], np.arange(256)) and not none['shade_on'].any()
    with pytest.raises(NotImplementedError, match="max_kernel_size"):
        P.sample_params({'params': {'motion_blur': {'max_kernel_size': 5}}}, ids[:1], 0, (240, 320))
    # additive_shade's defaults: kernel_size_range [250, 350], made odd (an empty dict is falsy: the stage is off, as in the reference)
    default = P.sample_params({'params': {'additive_shade': {'nb_ellipses': 20}}}, ids[:8], 0, (480, 640))
    assert not P.sample_params({'params': {'additive_shade': {}}}, ids[:2], 0, (480, 640))['shade_on'].any()
    assert (default['ksize'] >= 251).all() and (default['ksize'] <= 351).all()


def test_dropins_keep_the_references_signatures():
    from image_matching_amd.datasets.ALLSS import ALLSS
    from image_matching_amd.datasets.ALLSS_photo import ALLSSPhotometric
    from image_matching_amd.utils.photometric import ImgAugTransform, customizedTransform
    assert [p.kind for p in inspect.signature(ImgAugTransform.__init__).parameters.values()][1] == inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(customizedTransform.additive_shade).parameters) == ['self', 'image', 'nb_ellipses', 'transparency_range',
                                                                                      'kernel_size_range']
    assert list(inspect.signature(customizedTransform.__call__).parameters) == ['self', 'img', 'config']
    ImgAugTransform(photometric={'enable': False})
    ImgAugTransform(photometric=SHIPPED)
    with pytest.raises(NotImplementedError, match="GaussianBlur"):
        ImgAugTransform(photometric={'enable': True, 'params': {'GaussianBlur': {'sigma': 0.2}}})
    img = np.full((4, 4, 1), 0.5, np.float32)
    with pytest.raises(KeyError):
        customizedTransform()(img, photometric={'params': {}})
    # present but falsy: the reference divides by 255 all the same
    assert np.array_equal(customizedTransform()(img, photometric={'params': {'additive_shade': False}}), img / 255)
    # ALLSSPhotometric constructs where ALLSS raises, and ALLSS still raises
    kw = dict(images=np.zeros((1, 16, 16), np.float32), points=[np.zeros((0, 2), np.float32)], augmentation={'photometric': SHIPPED})
    with pytest.raises(NotImplementedError, match="imgaug"):
        ALLSS(task='train', **kw)
    ds = ALLSSPhotometric(task='train', **kw)
    assert ds.enable_photo and len(ds) == 1 and ds.photo_config['params'] == SHIPPED['params'] and SHIPPED['enable'] is True
    assert not ALLSSPhotometric(task='val', **kw).enable_photo
    assert list(inspect.signature(ALLSSPhotometric.__init__).parameters)[:3] == ["self", "export", "transform"]
    with pytest.raises(NotImplementedError, match="imgaug"):
        ALLSSPhotometric(task='train', gaussian_label={'enable': True}, **kw)


def test_float32_order_blur_against_float64():
    """the two statements of the 3x3 blur agree wherever the float64 sum is not within 1e-4 of a half-integer"""
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (37, 53)).astype(np.uint8)
    for kernel in (R.LINE_30, R.DYADIC):
        a, b = R.blur3(img, kernel, np.float32), R.blur3(img, kernel, np.float64)
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 1 and (a != b).mean() < 1e-2
    assert np.array_equal(R.blur3(img, R.DYADIC, np.float32), R.blur3(img, R.DYADIC, np.float64))      # dyadic weights: exact in both
    assert np.array_equal(R.blur3(img, (0, 0, 0, 0, 1, 0, 0, 0, 0)), img)
    assert np.array_equal(R.reflect101(np.arange(-7, 9), 3), [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0])


@pytest.mark.parametrize("shape", R.PIXEL_SHAPES)
def test_pixel_fixtures_stay_under_the_exemption_cap(shape):
    """at most 2e-3 of an image's pixels may be exempt (expected: 2 delta = 2e-4)"""
    c = R.pixel_case(shape)
    for b in range(shape[0]):
        share = R.exempt(shape[1], shape[2], c['noise_scale'][b], c['key'][b], R.EXEMPT_DELTA).mean()
        assert share <= R.EXEMPT_CAP, (shape, b, share)
    if shape[0] > 1:
        assert c['noise_scale'][-1] == 0 and c['thresh'][-1] == 0 and len({float(s) for s in c['noise_scale']}) == shape[0]


@pytest.mark.parametrize("case", R.SHADE_CASES)
def test_shade_fixtures_keep_off_the_ellipse_boundaries(case):
    """no pixel within 1e-9 of a boundary, where the mask would rest on the last bit of sin and cos; the halo of (101; 24x40) and
    (351; 64x96) exceeds the image"""
    c = R.shade_case(*case)
    k, H, W = case
    for b in range(4):
        n = c['n_ellipses'][b]
        if n:
            assert np.abs(R.ellipse_form(H, W, c['ellipses'][b, :n]) - 1.0).min() > R.BOUNDARY_MARGIN
    assert list(c['n_ellipses']) == [20, 0, 1, 20] and list(c['on']) == [1, 1, 1, 0]
    assert R.shade_mask(H, W, c['ellipses'][2, :1]).min() == 255 and 0 < R.shade_mask(H, W, c['ellipses'][0]).mean() < 255
    assert abs(float(c['taps'][0].astype(np.float64).sum()) - 1.0) < 1e-6
