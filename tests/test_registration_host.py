"""The exact-arithmetic reference of the registration post-step (tests/registration_ref.py) on the CPU: the oracle's own output passes
it on every case the GPU tests use, the lattice premise and the 1 % cap hold there, the checker rejects every mutation a subtly
wrong kernel would produce, and the float64 2-NN helper agrees with itself on ties."""
import numpy as np
import pytest

from tests import registration_ref as R

BATCHES = {bt.name: bt for bt in R.graded_batches() + R.hypothesis_count_batches() + R.lattice_batches()}


@pytest.fixture(scope="module")
def evaluated():
    """name -> [(bands, oracle output) per pair], computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            bt = BATCHES[name]
            cache[name] = [(bt.bands(b), bt.oracle(b)) for b in range(len(bt.cases))]
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(BATCHES))
def test_oracle_output_passes_the_checker_on_every_gpu_case(evaluated, name):
    """oracle/ransac_ref.py's output satisfies (a) to (d) within the 1 % cap; on lattice cases the premise holds and the mask is the
    integer one; the unfused fp32 residuals stay inside the derived band (printed, asserted below 1)."""
    bt = BATCHES[name]
    for b, (bands, (M, mask, n)) in enumerate(evaluated(name)):
        info = R.check_ransac_output(bands, M, mask, n)
        use = R.fp32_band_usage(bands)
        gam = [q.gamma for q in bands.live if not q.exact] or [0.0]
        print(f"[registration-host] {name} pair {b}: n {bands.n}, winner {info['h']} with {n} inliers (next definite count {info['second']}), "
              f"{info['undecided']} undecided, gamma {min(gam):.4f}..{max(gam):.4f} px, |e_fp32 - e_f64| / gamma <= {use:.4f}")
        assert use < 1.0
        if bt.lattice:
            ok, text = R.lattice_premise(bt.cases[b], bands)
            assert ok, f"{name} pair {b}: {text}"
            assert np.array_equal(mask, R.lattice_expected_mask(bt.cases[b])) and n == int(mask.sum())
            assert all(q.exact for q in bands.live if not (bt.cases[b][4][bands.valid][q.i] or bt.cases[b][4][bands.valid][q.j]))


def test_lstsq_fit_agrees_with_the_oracles_closed_form(evaluated):
    for name in ("g1024", "g700", "g300"):
        bands, (M, mask, n) = evaluated(name)[0]
        mk = mask[bands.valid] == 1
        assert np.abs(R.fit_similarity(bands.src[mk], bands.dst[mk]) - M).max() < 2e-5


def _raises(bands, M, mask, n, *words):
    with pytest.raises(R.RansacCheckError) as e:
        R.check_ransac_output(bands, M, mask, n)
    text = str(e.value)
    assert text.startswith(f"pair {bands.b}"), text
    for w in words:
        assert w in text, (w, text)
    return text


def test_checker_rejects_le_for_lt_on_a_lattice_case(evaluated):
    """e^2 <= thr^2 takes in the points exactly on the 7-px circle"""
    bt = BATCHES["l400"]
    bands, (M, mask, n) = evaluated("l400")[0]
    h = R.check_ransac_output(bands, M, mask, n)["h"]
    inl = bands.hyp[h].e <= 7.0
    assert int(inl.sum()) > n
    wrong = np.zeros_like(mask)
    wrong[bands.valid[inl]] = 1
    assert not np.array_equal(wrong, R.lattice_expected_mask(bt.cases[0]))
    _raises(bands, R.fit_similarity(bands.src[inl], bands.dst[inl]), wrong, int(inl.sum()), "hypothesis", "point", "definitely outside")


def test_checker_rejects_a_threshold_one_percent_off(evaluated):
    """caught wherever a residual lies between the two thresholds (not every case has one: g1024 and g300 have none for their winner)"""
    for name in ("g700", "g6000"):
        bt = BATCHES[name]
        bands, _ = evaluated(name)[0]
        c = bt.cases[0]
        M, mask, n = R.ransac_ref.estimate_affine_partial(c[0], c[1], c[2], b=0, thresh=bt.thresh * 1.01, hypotheses=bt.hypotheses, seed=bt.seed)
        _raises(bands, M, mask, n, "hypothesis", "point", "definitely outside")


def test_checker_rejects_dropped_set_and_miscounted_points(evaluated):
    bands, (M, mask, n) = evaluated("g700")[0]
    h = R.check_ransac_output(bands, M, mask, n)["h"]
    k = int(bands.valid[np.nonzero(bands.hyp[h].e < 1.0)[0][0]])           # a definite inlier
    drop = mask.copy()
    drop[k] = 0
    _raises(bands, M, drop, n - 1, f"point {k}", "definitely inside")
    free = int(np.nonzero(BATCHES["g700"].cases[0][2] < 0)[0][1])          # an unmatched row
    stray = mask.copy()
    stray[free] = 1
    _raises(bands, M, stray, n + 1, f"point {free}", "unmatched")
    _raises(bands, M, mask, n + 1, "n_inliers")
    _raises(bands, M, mask, n - 1, "n_inliers")


def test_checker_rejects_a_fit_without_its_last_inlier(evaluated):
    for name in ("g1024", "g300"):
        bands, (M, mask, n) = evaluated(name)[0]
        rows = np.nonzero(mask[bands.valid] == 1)[0][:-1]
        _raises(bands, R.fit_similarity(bands.src[rows], bands.dst[rows]), mask, n, "least-squares", "point")


def test_checker_rejects_a_later_hypothesis_when_an_earlier_one_is_definitely_better(evaluated):
    """the winner replaced by the best hypothesis of the later half of the sequence, where an earlier one definitely has more inliers"""
    hits = 0
    for name in ("g1024", "g700", "g300", "g6000"):
        bands, (M, mask, n) = evaluated(name)[0]
        win = R.check_ransac_output(bands, M, mask, n)["h"]
        later = [q for q in bands.live if q.h >= len(bands.hyp) // 2 and q.h > win]
        q = max(later, key=lambda q: q.nU)
        if max(p.nL for p in bands.live if p.h < q.h) > q.nU:
            _raises(bands, *R.output_of_hypothesis(bands, q.h), "hypothesis", "point", "more than the mask")
            hits += 1
    assert hits >= 2


def test_degenerate_cases_accept_only_what_they_must():
    all_same, some_same = R.degenerate_cases()
    bands = R.hypothesis_bands(*all_same, 0, 7.0, 64, 3)
    assert bands.n >= 4 and not bands.live
    zM, zmask = np.zeros((2, 3), np.float32), np.zeros(len(all_same[2]), np.uint8)
    R.check_ransac_output(bands, zM, zmask, 0)
    M, mask, n = R.ransac_ref.estimate_affine_partial(*all_same, b=0, thresh=7.0, hypotheses=64, seed=3)
    R.check_ransac_output(bands, M, mask, n)
    one = zmask.copy()
    one[1] = one[2] = 1
    _raises(bands, zM, one, 2, "must be all zero")
    bands = R.hypothesis_bands(*some_same, 0, 7.0, 64, 3)
    assert any(q is None for q in bands.hyp) and bands.live
    M, mask, n = R.ransac_ref.estimate_affine_partial(*some_same, b=0, thresh=7.0, hypotheses=64, seed=3)
    assert R.check_ransac_output(bands, M, mask, n)["h"] is not None and n >= 2
    _raises(bands, zM, zmask, 0, "empty mask", "hypothesis", "point")
    few = (some_same[0], some_same[1], np.where(np.arange(12) < 5, some_same[2], -1))       # three matches: no fit
    bands = R.hypothesis_bands(*few, 0, 7.0, 64, 3)
    assert bands.n == 3
    R.check_ransac_output(bands, zM, zmask, 0)


def test_a_case_with_a_wide_band_is_rejected_not_passed():
    """every residual at the threshold: the band holds far more than 1 % of the points"""
    K = 40
    k0 = np.stack([np.arange(K) * 10.0 + 0.3, (np.arange(K) % 7) * 30.0 + 0.7], 1).astype(np.float32)
    k1 = k0.copy()
    k1[2:, 1] += 7.0                                                        # e = 7 exactly under the model through points 0 and 1
    m = np.arange(K, dtype=np.int64)
    seed = next(s for s in range(100000) if set(R.ransac_ref._pair(s, 0, 0, K)) == {0, 1})
    bands = R.hypothesis_bands(k0, k1, m, 0, 7.0, 1, seed)
    M, mask, n = R.ransac_ref.estimate_affine_partial(k0, k1, m, b=0, thresh=7.0, hypotheses=1, seed=seed)
    with pytest.raises(R.BadCase, match="undecided"):
        R.check_ransac_output(bands, M, mask, n)


# ---------------------------------------------------------------------------------------------- 2-NN
def test_brute_force_2nn_orders_ties_lowest_index_first():
    a, b = R.tie_case()
    nn1, nn2, d1sq, d2sq = R.knn2_ref(a, b)
    for g, grp in enumerate(R.TIE_GROUPS):
        assert (nn1[g], nn2[g]) == grp[:2] and d1sq[g] == d2sq[g] and 0 < d1sq[g] < 0.5
    bar1, bar2 = R.knn_sq_bar(a, b, nn1), R.knn_sq_bar(a, b, nn2)
    for ratio, want in ((0.7, False), (1.5, True)):
        accept, decided = R.knn_decided(d1sq, d2sq, bar1, bar2, ratio)
        assert (accept == want).all() and decided.all()
    accept, decided = R.knn_decided(d1sq, d2sq, bar1, bar2, 1.0)            # dist1 < dist2 on a tie: false in float64, but not decided
    assert not accept.any() and not decided.any()
    m, d1, d2 = R.knn_fp32_restatement(a, b, 1.5)
    R.check_knn_output(a, b, 1.5, m, d1, d2, "ties")


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("s", R.NEAR_DUPLICATE_S)
def test_near_duplicates_fp32_restatement_is_inside_the_squared_distance_bar(d, s):
    """the host's fp32 evaluation of |a|^2 + |b|^2 - 2ab passes the check the GPU is held to; at most 2 % of the rows are undecided"""
    a, b = R.near_duplicate_case(d, s)
    m, d1, d2 = R.knn_fp32_restatement(a, b, 0.7)
    worst, undecided = R.check_knn_output(a, b, 0.7, m, d1, d2, f"d={d} s={s}")
    print(f"[registration-host] near-duplicates d={d} s={s}: fp32 restatement uses {worst:.3f} of the squared-distance bar, {undecided} of {len(a)} rows undecided, "
          f"nearest distance {np.sqrt(R.knn2_ref(a, b)[2]).max():.2e} at most")
    if s >= 1e-4:
        assert undecided <= 0.02 * len(a)
    wrong = d1.astype(np.float64) + 1e-2                                   # what the present 2e-4 bar on the distance cannot see at s = 0 ...
    with pytest.raises(AssertionError, match="of the bar"):
        R.check_knn_output(a, b, 0.7, m, wrong, d2, "shifted")


@pytest.mark.parametrize("N1", R.EDGE_N1)
def test_edge_counts_fp32_restatement_passes(N1):
    for N0 in R.EDGE_N0:
        a, b = R.planted_case(N0, N1, 64, 0)
        m, d1, d2 = R.knn_fp32_restatement(a, b, 0.95)
        R.check_knn_output(a, b, 0.95, m, d1, d2, f"{N0}x{N1}")
