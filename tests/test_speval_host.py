"""The fixtures of tests/test_gpu_speval.py are fair: by the float64 reference alone (tests/speval_ref.py), every matcher case leaves at
most max(2, 1 %) of a side's rows inside the similarity band, numpy's own fp32 product sits well inside the bound the band is built
from, planted duplicates are decided rows whose answer is the lowest index, and the metric cases leave no decision within 1e-9 px of
eps, of the image border or of w = 0 -- except the points planted exactly on the border, which are exact and visible.  No GPU."""
import numpy as np
import pytest

from tests import speval_ref as R


@pytest.mark.parametrize("name", sorted(R.MATCH_CASES))
def test_matcher_cases_are_fair(name):
    a, b = R.descriptor_case(*R.MATCH_CASES[name])
    m = R.Match(a, b)
    print(f"{name}: {m.s0.band_rows()} of {m.s0.n} rows and {m.s1.band_rows()} of {m.s1.n} columns in the band")
    assert m.fair()
    # the bound is not vacuous and not tight: an fp32 product computed by other code (numpy's) stays far inside it
    err = np.abs((a @ b.T).astype(np.float64) - m.S) / R.gamma(a, b)
    print(f"{name}: numpy's fp32 product at {err.max():.3f} gamma")
    assert err.max() < 0.5
    # the planted copies are what the search finds: most rows of the first half of side 1 have a mutual neighbour
    mutual = sum(1 for j in range(m.s1.n) if m.s1.nn[j] >= 0 and m.s0.nn[m.s1.nn[j]] == j)
    assert R.MATCH_CASES[name][1] == 1 or mutual >= m.s1.n // 4


def test_ragged_counts_are_fair():
    a, b = R.descriptor_case(*R.MATCH_CASES["d128"])
    for n0, n1 in R.RAGGED:
        m = R.Match(a, b, n0, n1)
        assert m.fair()
        if n0 == 0:
            assert all(len(c) == 0 for c in m.s1.cand) and m.s0.n == 0
        if n0 == 1:
            assert np.all(m.s1.nn == 0) and 0 <= m.s0.nn[0] < n1


def test_duplicates_are_decided_rows_with_the_lowest_index():
    a, b, src, copies = R.duplicate_case()
    m = R.Match(a, b)
    assert m.fair()
    assert m.s0.decided[src] and list(m.s0.cand[src]) == [3, 7, 200] and m.s0.nn[src] == 3
    for j in (3, 7, 200):
        assert m.s1.decided[j] and m.s1.nn[j] == src
    for i in copies:                               # three copies of one query: the same key, which answers with the lowest of them
        assert m.s0.decided[i] and m.s0.nn[i] == 10
    assert list(m.s1.cand[10]) == copies and m.s1.decided[10] and m.s1.nn[10] == copies[0]


def test_d1_is_all_exact_ties():
    a, b = R.descriptor_case(*R.MATCH_CASES["d1"])
    assert set(np.unique(a)) == {-1.0, 1.0} == set(np.unique(b))
    m = R.Match(a, b)
    assert m.s0.decided.all() and m.s1.decided.all()
    assert all(m.s0.nn[i] == np.nonzero(b[:, 0] == a[i, 0])[0][0] for i in range(len(a)))


def test_nan_rows_have_no_neighbour_and_never_win():
    a, b = R.descriptor_case(*R.MATCH_CASES["d33"])
    b[11, 5] = np.nan
    m = R.Match(a, b)
    assert len(m.s1.cand[11]) == 0 and m.s1.nn[11] == -1 and not np.any(m.s0.nn == 11) and m.fair()


@pytest.mark.parametrize("with_matches", [True, False])
def test_metric_case_leaves_no_decision_in_the_band(with_matches):
    case = R.metric_case(21, 3, 257, 300, *R.METRIC_COUNTS)
    counts, sums, margin = R.case_metrics(case, 3.0, with_matches)
    print(counts, sums, margin)
    assert margin > R.EPS_BAND
    v0, v1, r0, r1, m, c = counts[0, :6]
    assert 0 < r0 < v0 < 257 and 0 < r1 < v1 < 300 and sums[0].min() > 0      # the warp takes points out of view; not every point repeats
    assert (0 < c < m < 257) if with_matches else (m == c == 0)
    assert not counts[2, [0, 2, 3, 4, 5]].any() and counts[2, 1] > 0 and counts[1, 1] <= 1     # an empty side 0; a single point on side 1


def test_border_points_under_the_identity_are_exact_and_visible():
    w, h = 640, 480
    k = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1], [17, 0], [w - 1, 33.5], [w - 0.5, 10], [5, -0.25]], np.float32)
    counts, sums, _ = R.pair_metrics(k, len(k), k, len(k), np.eye(3), w, h, 3.0, np.arange(len(k)))
    assert list(counts) == [6, 6, 6, 6, 8, 8, 0, 0] and not sums.any()


def test_singular_warp_is_bad():
    k = np.ones((4, 2), np.float32)
    counts, sums, _ = R.pair_metrics(k, 4, k, 4, np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1.0]]), 64, 64, 3.0, None)
    assert list(counts) == [0, 0, 0, 0, 0, 0, 1, 0] and not sums.any()
