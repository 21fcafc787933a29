"""The batched RANSAC homography fit and the corner error on the GPU (libimx_homog.so: imx_estimate_homography,
imx_homography_corner_error; Engine.estimate_homography, Engine.homography_corner_error) against tests/homography_ref.py.

The rules, all derived from the reference alone (see homography_ref's docstring):
  the mask   a point the reference is certain about (outside the band gamma_h round the threshold) is in / out of the mask accordingly;
             a case with more than 1 % of the winner's points undecided is rejected as a bad case, not passed
  the winner best_h is not certainly beaten: no h' with nL(h') > nU(best_h) and no h' < best_h with nL(h') >= nU(best_h)
  the refit  the kernel's H and the reference's refit on the kernel's OWN reported inlier set, same refine_iters, agree to 1e-7 px at
             the four image corners (derived in the issue and in DESIGN.md: four orders above what two float64 solutions differ by,
             three below an fp32 accumulation)
Needs an MI355X; each test takes a few seconds at the most."""
import functools

import numpy as np
import pytest
import torch

from tests import homography_ref as R
from tests import util

pytestmark = pytest.mark.gpu
THR, HYP, SEED = 3.0, 300, 11
COUNTS = (257, 100, 40)
W, H = 640, 480


@pytest.fixture(scope="module")
def eng():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


@functools.lru_cache(maxsize=None)
def planted(noise):
    """B = 3, K0 = K1 = 257, counts0 = (257, 100, 40), a third unmatched, every seventh match 30 to 130 px off -> the case and the
    reference's view of each pair (computed once, read-only)"""
    case = R.planted_case(3 if noise else 2, 3, 257, 257, COUNTS, size=(W, H), noise=noise)
    pairs = tuple(R.Pair(case["kpts0"][b], case["kpts1"][b], case["matches0"][b], COUNTS[b], THR, HYP, SEED) for b in range(3))
    return case, pairs


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def run(eng, kpts0, kpts1, matches0, counts0=None, thr=THR, hyp=HYP, seed=SEED, refine=3):
    out = eng.estimate_homography(cuda(kpts0), cuda(kpts1), cuda(matches0), None if counts0 is None else cuda(np.asarray(counts0, np.int32)),
                                  ransac_thresh=thr, hypotheses=hyp, refine_iters=refine, seed=seed)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check_pair(pair, Hk, mask, ninl, best, refine=3, size=(W, H)):
    """the three rules for one pair; returns the refit's corner disagreement in px"""
    assert best >= 0 and Hk[2, 2] == 1.0 and np.all(np.isfinite(Hk))
    pair.check_winner(int(best))
    compacted = pair.check_mask(int(best), mask)
    assert int(ninl) == int(mask.sum()) == int(compacted.sum())
    ref = pair.refit(compacted, refine)
    assert ref is not None
    d = float(R.corner_distances(Hk, ref, *size).max())
    print(f"refit corner disagreement {d:.3e} px = {d / R.REFIT_BAR:.2e} of the bar")
    assert d <= R.REFIT_BAR, d
    return d


def assert_failure(Hk, mask, ninl, best):
    assert not Hk.any() and not mask.any() and int(ninl) == 0 and int(best) == -1


def test_planted_without_noise_the_mask_is_the_planted_set(eng):
    case, pairs = planted(0.0)
    Hk, mask, ninl, best = run(eng, case["kpts0"], case["kpts1"], case["matches0"], COUNTS)
    for b, pair in enumerate(pairs):
        check_pair(pair, Hk[b], mask[b], ninl[b], best[b])
        assert np.array_equal(mask[b].astype(bool), case["planted"][b]), b
        assert int(ninl[b]) == int(case["planted"][b].sum())
        assert R.corner_distances(Hk[b], case["H_gt"][b], W, H).max() < 1e-3       # fp32 coordinates of an exact warp


def test_planted_with_noise(eng):
    case, pairs = planted(0.5)
    Hk, mask, ninl, best = run(eng, case["kpts0"], case["kpts1"], case["matches0"], COUNTS)
    for b, pair in enumerate(pairs):
        check_pair(pair, Hk[b], mask[b], ninl[b], best[b])
        assert R.corner_distances(Hk[b], case["H_gt"][b], W, H).max() < 3.0


@pytest.mark.parametrize("K", [8192, 8193], ids=["staged_in_lds", "staged_in_the_workspace"])
def test_staging_limit(eng, K):
    case = R.planted_case(40 + K, 1, K, K, (K,), size=(W, H), noise=0.5)
    pair = R.Pair(case["kpts0"][0], case["kpts1"][0], case["matches0"][0], K, THR, 64, SEED)
    Hk, mask, ninl, best = run(eng, case["kpts0"], case["kpts1"], case["matches0"], None, hyp=64)
    check_pair(pair, Hk[0], mask[0], ninl[0], best[0])


def test_exactly_four_matches_are_reproduced(eng):
    rng = np.random.default_rng(5)
    k0 = np.array([[[30, 40], [600, 25], [580, 440], [45, 420], [300, 200], [10, 10]]], np.float32)
    k1 = (k0[:, ::-1] + rng.uniform(-25, 25, k0.shape)).astype(np.float32)
    m = np.array([[5, 4, 3, 2, -1, -1]], np.int64)         # four matches (slot i of side 0 is slot 5 - i of side 1), K0 = K1 = 6
    Hk, mask, ninl, best = run(eng, k0, k1, m, None, hyp=8)
    assert int(ninl[0]) == 4 and best[0] >= 0 and np.array_equal(mask[0], [1, 1, 1, 1, 0, 0])
    idx = np.nonzero(m[0] >= 0)[0]
    q = R.project(Hk[0], k0[0, idx].astype(np.float64))[0]
    assert np.abs(q - k1[0, m[0, idx]].astype(np.float64)).max() <= 1e-7


def test_fewer_than_four_matches_fail(eng):
    rng = np.random.default_rng(6)
    k0, k1 = rng.uniform(0, 600, (2, 9, 2)).astype(np.float32), rng.uniform(0, 600, (2, 9, 2)).astype(np.float32)
    m = np.full((2, 9), -1, np.int64)
    m[0, [1, 4, 7]] = [3, 0, 8]                             # n = 3 and n = 0
    Hk, mask, ninl, best = run(eng, k0, k1, m, None, hyp=16)
    for b in range(2):
        assert_failure(Hk[b], mask[b], ninl[b], best[b])
    # ... and matches past counts0 do not count: five matches, two of them below the count
    m[1, :5] = [0, 1, 2, 3, 4]
    Hk, mask, ninl, best = run(eng, k0, k1, m, (9, 2), hyp=16)
    assert_failure(Hk[1], mask[1], ninl[1], best[1])


def test_degenerate_geometry_fails(eng):
    rng = np.random.default_rng(7)
    K = 40
    t = rng.uniform(0, 500, K)
    line = np.stack([t, 0.5 * t + 20], -1)
    same = np.tile([[123.25, 77.5]], (K, 1))
    k0 = np.stack([line, same]).astype(np.float32)
    k1 = np.stack([line + 5, same]).astype(np.float32)
    m = np.tile(np.arange(K, dtype=np.int64), (2, 1))
    Hk, mask, ninl, best = run(eng, k0, k1, m, None, hyp=64)
    for b in range(2):
        assert_failure(Hk[b], mask[b], ninl[b], best[b])


def test_duplicated_matches(eng):
    """every keypoint of a noisy planted pair listed three times: the hypotheses that draw a duplicate are degenerate, nothing is NaN, the
    rules hold"""
    case, _ = planted(0.5)
    k0, m = np.tile(case["kpts0"][1:2, :100], (1, 3, 1)), np.tile(case["matches0"][1:2, :100], (1, 3))
    pair = R.Pair(k0[0], case["kpts1"][1], m[0], None, THR, HYP, SEED)
    Hk, mask, ninl, best = run(eng, k0, case["kpts1"][1:2], m, None)
    assert np.all(np.isfinite(Hk))
    check_pair(pair, Hk[0], mask[0], ninl[0], best[0])


def test_invariance(eng):
    """equal bits for H, the mask, the count and best_h: alone, at position 0 and 2 of a batch of 3, with K0 padded by 31 slots of NaN past
    counts0, after an intervening call of another shape, and called twice"""
    case, _ = planted(0.5)
    k0, k1, m = case["kpts0"], case["kpts1"], case["matches0"]
    whole = run(eng, k0, k1, m, COUNTS)
    again = run(eng, k0, k1, m, COUNTS)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(whole, again)), "called twice"
    for b in range(3):
        want = tuple(bits(t[b]) for t in whole)
        alone = run(eng, k0[b:b + 1], k1[b:b + 1], m[b:b + 1], COUNTS[b:b + 1])
        assert all(np.array_equal(bits(t[0]), w) for t, w in zip(alone, want)), ("alone", b)
        for pos in (0, 2):
            order = [x for x in range(3) if x != b]
            order.insert(pos, b)
            moved = run(eng, k0[order], k1[order], m[order], [COUNTS[x] for x in order])
            assert all(np.array_equal(bits(t[pos]), w) for t, w in zip(moved, want)), ("position", b, pos)
    # K0 padded by 31 slots past counts0, NaN coordinates and live-looking matches in the padding
    k0p = np.concatenate([k0, np.full((3, 31, 2), np.nan, np.float32)], 1)
    mp = np.concatenate([m, np.zeros((3, 31), np.int64)], 1)
    padded = run(eng, k0p, k1, mp, COUNTS)
    assert np.array_equal(bits(padded[0]), bits(whole[0])) and np.array_equal(padded[1][:, :257], whole[1])
    assert not padded[1][:, 257:].any() and np.array_equal(padded[2], whole[2]) and np.array_equal(padded[3], whole[3])
    # an intervening call of another shape (it regrows the workspace), on the same handle
    big = R.planted_case(9, 2, 8300, 8300, (8300, 8300), size=(W, H), noise=0.5)
    run(eng, big["kpts0"], big["kpts1"], big["matches0"], None, hyp=8)
    after = run(eng, k0, k1, m, COUNTS)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(whole, after)), "after another shape"


def test_corner_error(eng):
    case, _ = planted(0.5)
    rng = np.random.default_rng(8)
    H_gt = case["H_gt"]
    H_est = H_gt + rng.normal(0, 1e-4, H_gt.shape) * np.abs(H_gt)
    H_est[1] = 0.0
    err = eng.homography_corner_error(cuda(H_est), H_gt, (H, W))
    torch.cuda.synchronize()
    err = err.cpu().numpy()
    assert err.dtype == np.float64 and np.isposinf(err[1])
    for b in (0, 2):
        assert abs(err[b] - R.corner_error(H_est[b], H_gt[b], W, H)) <= 1e-9
    same = eng.homography_corner_error(cuda(H_gt), cuda(H_gt), (H, W)).cpu().numpy()
    assert np.all(same == 0.0)


def test_wrappers_refuse_wrong_arguments(eng):
    from image_matching_amd.engine import ImxError
    case, _ = planted(0.5)
    k0, k1, m = cuda(case["kpts0"]), cuda(case["kpts1"]), cuda(case["matches0"])
    for bad in ((k0.cpu(), k1, m), (k0.double(), k1, m), (k0, k1, m.int()), (k0[:, :100], k1, m), (k0, k1[:2], m)):
        with pytest.raises(ImxError):
            eng.estimate_homography(*bad)
    with pytest.raises(ImxError):
        eng.estimate_homography(k0, k1, m, ransac_thresh=float("nan"))
    with pytest.raises(ImxError):
        eng.estimate_homography(k0, k1, m, hypotheses=0)
    with pytest.raises(ImxError):
        eng.homography_corner_error(torch.zeros(3, 3, 3, device="cuda"), case["H_gt"], (H, W))
