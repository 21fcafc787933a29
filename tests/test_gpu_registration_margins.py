"""The registration post-step at its decision boundaries (csrc/registration.hip; needs an MI355X): RANSAC with residuals spread across
the threshold and exactly on it, every size round the two steps of its coordinate staging (64 KB / 128 KB of dynamic LDS, HBM scratch),
degenerate samples and the stride of the hypothesis loop; the 2-NN matcher on exact ties, on counts round one lane stride and on
near-duplicates.  The reference is tests/registration_ref.py (float64, derived bands), not the fp32 restatement: that one is the bit-exact
partner on separated data only (tests/test_gpu_registration.py)."""
import numpy as np
import pytest
import torch

from tests import registration_ref as R
from tests import util

pytestmark = pytest.mark.gpu

GRADED = {bt.name: bt for bt in R.graded_batches() + R.hypothesis_count_batches()}
LATTICE = {bt.name: bt for bt in R.lattice_batches()}


def _engine(d=128, K=1024):
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(d, K), util.sg_config(d), "cuda")


def _ransac(eng, bt):
    k0 = torch.from_numpy(np.stack([c[0] for c in bt.cases])).cuda()
    k1 = torch.from_numpy(np.stack([c[1] for c in bt.cases])).cuda()
    m = torch.from_numpy(np.stack([c[2] for c in bt.cases])).cuda()
    counts = None if bt.counts0 is None else torch.tensor(bt.counts0, dtype=torch.int32, device="cuda")
    M, inl, ninl = eng.estimate_affine_partial(k0, k1, m, counts0=counts, ransac_thresh=bt.thresh, hypotheses=bt.hypotheses, seed=bt.seed)
    return M.cpu().numpy(), inl.cpu().numpy(), ninl.cpu().numpy()


@pytest.mark.parametrize("name", list(GRADED))
def test_ransac_graded_residuals_pass_the_exact_checker(name):
    """Gaussian noise of 3 px plus graded outliers: residuals on both sides of the threshold at every distance, best and second-best
    counts 0 to 3 apart.  The output must be one a correct fp32 evaluation can give (registration_ref.check_ransac_output): single
    pairs, three pairs with a transform each, counts0 cutting two pairs, K = 6000 (96 KB of LDS), and hypothesis counts round the
    256-thread stride of the hypothesis loop."""
    bt = GRADED[name]
    M, inl, ninl = _ransac(_engine(), bt)
    for b in range(len(bt.cases)):
        info = R.check_ransac_output(bt.bands(b), M[b], inl[b], ninl[b])
        print(f"[registration-margins] {name} pair {b}: hypothesis {info['h']} won with {int(ninl[b])} of {info['n']} (next definite count {info['second']}), {info['undecided']} undecided")


@pytest.mark.parametrize("name", list(LATTICE))
def test_ransac_lattice_cases_decide_the_threshold_exactly(name):
    """Integer coordinates under an integer similarity, a fifth of the points moved by integer vectors of length sqrt 41 .. sqrt 53, some
    exactly 7 px: on a clean hypothesis the kernel's arithmetic is exact, so the mask must equal e^2 < 49 evaluated in integers --
    `<=`, a threshold or a residual slightly off, or a count that skips points would all show.  K = 4096 .. 8193: the first launches
    above 64 KB of dynamic LDS, both sides of the LDS / scratch switch, and a second pair in the scratch."""
    bt = LATTICE[name]
    bands = [bt.bands(b) for b in range(len(bt.cases))]
    for b, c in enumerate(bt.cases):
        ok, text = R.lattice_premise(c, bands[b])
        assert ok, f"{name} pair {b}: the case's premise fails: {text}"
    M, inl, ninl = _ransac(_engine(128, 1024 if len(bt.cases[0][2]) <= 8192 else -1), bt)
    for b, c in enumerate(bt.cases):
        want = R.lattice_expected_mask(c)
        diff = np.nonzero(inl[b] != want)[0]
        assert not len(diff), f"{name} pair {b}: the mask differs from e^2 < 49 in integers on {len(diff)} rows, first {int(diff[0])}: got {int(inl[b][diff[0]])}"
        assert int(ninl[b]) == int(want.sum())
        Mr, maskr, nr = bt.oracle(b)
        assert np.array_equal(maskr, want) and nr == int(want.sum())
        np.testing.assert_allclose(M[b], Mr, atol=R.RANSAC_ATOL, rtol=R.RANSAC_RTOL)
        R.check_ransac_output(bands[b], M[b], inl[b], ninl[b])


def test_ransac_degenerate_samples_then_a_normal_call():
    """Every matched kpts0 row the same point: every hypothesis has den = 0, the output is all zero; only some rows the same: the
    degenerate hypotheses are skipped; the handle then answers a normal call correctly."""
    eng = _engine()
    all_same, some_same = R.degenerate_cases()
    for case, must_be_zero in ((all_same, True), (some_same, False)):
        k0, k1, m = (torch.from_numpy(x)[None].cuda() for x in case)
        M, inl, ninl = eng.estimate_affine_partial(k0, k1, m, ransac_thresh=7.0, hypotheses=64, seed=3)
        M, inl, ninl = M.cpu().numpy(), inl.cpu().numpy(), ninl.cpu().numpy()
        bands = R.hypothesis_bands(*case, 0, 7.0, 64, 3)
        assert bands.n >= 4
        info = R.check_ransac_output(bands, M[0], inl[0], ninl[0])
        if must_be_zero:
            assert not bands.live and int(ninl[0]) == 0 and not inl.any() and (M == 0).all()
        else:
            assert info["h"] is not None and int(ninl[0]) >= 4
    bt = GRADED["g300"]
    M, inl, ninl = _ransac(eng, bt)
    R.check_ransac_output(bt.bands(0), M[0], inl[0], ninl[0])


# ---------------------------------------------------------------------------------------------- 2-NN matcher
def _knn(eng, a, b, ratio, n0=None, n1=None):
    """a (B,N0,d), b (B,N1,d) numpy -> numpy outputs; the library sees (B,d,N) strided views"""
    ta, tb = torch.from_numpy(np.ascontiguousarray(a)).cuda().transpose(1, 2), torch.from_numpy(np.ascontiguousarray(b)).cuda().transpose(1, 2)
    cnt = lambda n: None if n is None else torch.tensor(n, dtype=torch.int32, device="cuda")
    m, d1, d2 = eng.knn_ratio_match(ta, tb, ratio=ratio, n0=cnt(n0), n1=cnt(n1))
    return m.cpu().numpy(), d1.cpu().numpy(), d2.cpu().numpy()


def test_knn_exact_ties_keep_the_lowest_index_and_equal_distances():
    """Bit-equal columns of desc1 64 apart (one lane of the wave: the scan's in-lane rule), 1 and 37 apart (the cross-lane merge), in
    the first 64-block and with the copy in the last, partial one, and two triples; the query is a noisy copy of the column.  Both
    distances are the same number bit for bit, so the 0.7 ratio test rejects every row and a ratio of 1.5 accepts the LOWEST tied index."""
    a, b = R.tie_case(64)
    eng = _engine(64, 64)
    m, d1, d2 = _knn(eng, a[None], b[None], 0.7)
    assert np.array_equal(d1.view(np.int32), d2.view(np.int32)), (d1, d2)
    assert (m == -1).all(), m
    m15, e1, e2 = _knn(eng, a[None], b[None], 1.5)
    assert np.array_equal(e1.view(np.int32), d1.view(np.int32)) and np.array_equal(e2.view(np.int32), d2.view(np.int32))
    assert m15[0].tolist() == [g[0] for g in R.TIE_GROUPS], m15
    R.check_knn_output(a, b, 1.5, m15[0], e1[0], e2[0], "ties")


def test_knn_small_and_edge_counts():
    """N1 and n1 of 2, 3, 63, 64, 65 and 129 (64 = one lane stride of the scan), N0 of 1, 3, 4 and 5 (four query rows per workgroup),
    as plain shapes and as counts inside padded tensors whose padding columns are copies of the queries; n1 = 1 matches nothing."""
    eng = _engine(64, 64)
    d, worst = 64, 0.0
    for t, N1 in enumerate(R.EDGE_N1):
        for N0 in R.EDGE_N0:
            a, b = R.planted_case(N0, N1, d, 0)
            m, d1, d2 = _knn(eng, a[None], b[None], 0.95)
            worst = max(worst, R.check_knn_output(a, b, 0.95, m[0], d1[0], d2[0], f"{N0}x{N1}")[0])
    n1 = list(R.EDGE_N1) + [1]
    n0 = [1, 3, 4, 5, 5, 2, 3]
    B, N0c, N1c = len(n1), 5, 129
    A, Bm = np.zeros((B, N0c, d), np.float32), np.zeros((B, N1c, d), np.float32)
    cases = [R.planted_case(n0[i], n1[i], d, 1) for i in range(B)]
    for i, (a, b) in enumerate(cases):
        A[i, :n0[i]], Bm[i, :n1[i]] = a, b
        A[i, n0[i]:] = a[0]
        Bm[i, n1[i]:] = a[np.arange(N1c - n1[i]) % n0[i]]          # a column past the count at distance 0 from a query
    m, d1, d2 = _knn(eng, A, Bm, 0.95, n0, n1)
    for i, (a, b) in enumerate(cases):
        assert (m[i, n0[i]:] == -1).all() and not d1[i, n0[i]:].any() and not d2[i, n0[i]:].any(), f"pair {i}: rows past n0"
        if n1[i] < 2:
            assert (m[i] == -1).all() and not d1[i].any() and not d2[i].any(), f"pair {i}: n1 = 1 must match nothing, distances 0"
        else:
            worst = max(worst, R.check_knn_output(a, b, 0.95, m[i, :n0[i]], d1[i, :n0[i]], d2[i, :n0[i]], f"pair {i}: n0 {n0[i]} n1 {n1[i]}")[0])
    a, b = R.planted_case(5, 2, d, 2)
    m, d1, d2 = _knn(eng, a[None], b[None, :1], 0.95)              # N1 = 1 as a shape
    assert (m == -1).all() and not d1.any() and not d2.any()
    print(f"[registration-margins] 2-NN edge counts: worst fraction of the squared-distance bar used {worst:.3f}")


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("s", R.NEAR_DUPLICATE_S)
def test_knn_near_duplicates_stay_inside_the_squared_distance_bar(d, s):
    """desc1 = normalize(desc0 + s noise): the nearest distance is about s sqrt(d) and |a|^2 + |b|^2 - 2ab cancels.  The bar is on the
    SQUARED distance, (d + 4) 2^-24 (|a|^2 + |b|^2): the a-priori bound of an fp32 evaluation in any summation order (derived, not
    measured); the ratio decision is required wherever float64's survives moving both squared distances by it.  An exact duplicate
    need not come back at distance 0 -- only within sqrt(bar), about 3e-3 at d = 64 and 6e-3 at d = 256."""
    a, b = R.near_duplicate_case(d, s)
    m, d1, d2 = _knn(_engine(d, 64), a[None], b[None], 0.7)
    worst, undecided = R.check_knn_output(a, b, 0.7, m[0], d1[0], d2[0], f"d={d} s={s}")
    print(f"[registration-margins] near-duplicates d={d} s={s}: {worst:.3f} of the squared-distance bar used, {undecided} rows undecided, largest dist1 {d1.max():.3e}")
    assert (m[0] == np.arange(len(a))).all()


def test_knn_refuses_mismatched_descriptors_and_counts_before_any_library_call():
    """The library reads descriptor_dim channels of B pairs from both sides through raw pointers: other shapes are refused by the
    engine.  The descriptors here have MORE channels than the handle (256 on 128), and the library entry point is blocked for the
    duration, so nothing can read past a tensor even if a check were missing."""
    from image_matching_amd.engine import ImxError
    eng = _engine(128, 64)
    real = eng.lib

    class Blocked:
        def __getattr__(self, name):
            if name == "imx_knn_ratio_match":
                raise AssertionError("knn_ratio_match reached the library with arguments it must refuse")
            return getattr(real, name)
    g = torch.Generator().manual_seed(0)
    wide = torch.nn.functional.normalize(torch.randn(2, 256, 40, generator=g), dim=1).cuda()
    good = torch.nn.functional.normalize(torch.randn(2, 128, 40, generator=g), dim=1).cuda()
    cnt = torch.tensor([40, 17], dtype=torch.int32, device="cuda")
    eng.lib = Blocked()
    try:
        for args, kw in (((wide, good), {}), ((good, wide), {}), ((wide, wide), {}), ((good, good[:1]), {}), ((good[:1], good), {}),
                         ((good, good), {"n0": cnt.long()}), ((good, good), {"n1": cnt.float()}), ((good, good), {"n0": cnt[:1]}),
                         ((good, good), {"n1": torch.cat([cnt, cnt])}), ((good, good), {"n0": cnt.cpu()}), ((good, good), {"n1": [40, 17]}),
                         ((good[0], good[0]), {})):
            with pytest.raises(ImxError, match="knn_ratio_match"):
                eng.knn_ratio_match(*args, **kw)
    finally:
        eng.lib = real
    m, d1, d2 = eng.knn_ratio_match(good, good, ratio=0.7, n0=cnt, n1=cnt)      # the same handle still answers
    assert m[0].tolist() == list(range(40)) and m[1, :17].tolist() == list(range(17)) and (m[1, 17:] == -1).all()
