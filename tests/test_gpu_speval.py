"""The mutual nearest-neighbour matcher and the pair metrics on the GPU (libimx_speval.so: imx_mutual_nn_match,
imx_keypoint_pair_metrics; Engine.mutual_nn_match, Engine.keypoint_pair_metrics) against tests/speval_ref.py.

The rules, all derived from the reference alone (speval_ref's docstring; tests/test_speval_host.py shows the cases to be fair):
  the matcher  sim is within gamma = 2 (D + 2) 2^-24 |a| |b| of the float64 maximum; a decided row (one candidate within 2 gamma of the
               best, or bit-identical copies of one) reports the lowest candidate exactly, a row in the band one of its candidates;
               matches0[i] == j exactly where matches1[j] == i
  the metrics  no decision of the cases lies within 1e-9 px of its boundary, so the eight integers are equal; the sums agree to 1e-9 px
               per point
  invariances  bit for bit
Needs an MI355X; each test takes a few seconds at the most."""
import functools

import numpy as np
import pytest
import torch

from tests import speval_ref as R
from tests import util

pytestmark = pytest.mark.gpu
EPS = 3.0


@pytest.fixture(scope="module")
def eng():
    from image_matching_amd.engine import Engine
    return Engine(util.sp_config(128, 256), util.sg_config(128), "cuda")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(x, y):
    return all(np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8)) for p, q in zip(x, y))


@functools.lru_cache(maxsize=None)
def case(name):
    return R.descriptor_case(*R.MATCH_CASES[name])


def match(eng, a, b, n0=None, n1=None, layout="bkd"):
    """a (B,N0,D), b (B,N1,D) numpy -> the four outputs as numpy.  layout: how the device tensor is stored -- (B,K,D) read through a
    transposed view, or (B,D,N) contiguous"""
    if layout == "bkd":
        d0, d1 = cuda(a).transpose(1, 2), cuda(b).transpose(1, 2)
    else:
        d0, d1 = cuda(a.transpose(0, 2, 1)), cuda(b.transpose(0, 2, 1))
    out = eng.mutual_nn_match(d0, d1, None if n0 is None else cuda(np.asarray(n0, np.int32)), None if n1 is None else cuda(np.asarray(n1, np.int32)))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def padded(a, n, N):
    """rows [0, n) of a in a frame of N rows; the rest NaN"""
    out = np.full((N, a.shape[1]), np.nan, np.float32)
    out[:n] = a[:n]
    return out


# ------------------------------------------------------------------------------------------------------------ the matcher
def test_ragged_batch_against_the_reference(eng):
    """B = 3, D = 128, 257 x 300, counts (257, 300), (0, 150), (1, 200); NaN past the counts"""
    a, b = case("d128")
    A = np.stack([padded(a, n0, 257) for n0, _ in R.RAGGED])
    Bm = np.stack([padded(b, n1, 300) for _, n1 in R.RAGGED])
    out = match(eng, A, Bm, [n for n, _ in R.RAGGED], [n for _, n in R.RAGGED])
    for k, (n0, n1) in enumerate(R.RAGGED):
        worst = R.Match(a, b, n0, n1).check(*(o[k] for o in out))
        print(f"pair {k} ({n0} x {n1}): sim at {worst:.3f} of gamma")
    assert not (out[0][1] != -1).any() and not out[2][1].any() and not (out[1][1] != -1).any() and not out[3][1].any()    # the empty side
    assert out[0][2][0] >= 0 and out[1][2][out[0][2][0]] == 0             # a single row is every key's neighbour: it has a mutual one


@pytest.mark.parametrize("name", ["d256", "d33", "d1", "d64_two_row_blocks"])
def test_case_against_the_reference(eng, name):
    a, b = case(name)
    out = match(eng, a[None], b[None])
    worst = R.Match(a, b).check(*(o[0] for o in out))
    print(f"{name}: sim at {worst:.3f} of gamma; {(out[0][0] >= 0).sum()} mutual matches")
    assert (out[0][0] >= 0).sum() >= min(len(a), len(b)) // 4 or name == "d1"


def test_one_count_on_the_key_side(eng):
    a, b = case("d33")
    out = match(eng, a[None], b[None], [70], [1])
    R.Match(a, b, 70, 1).check(*(o[0] for o in out))
    assert out[1][0][0] >= 0 and (out[0][0] >= 0).sum() == 1


def test_both_layouts_give_equal_bits(eng):
    a, b = case("d33")
    x, y = case("d128")
    for p, q in ((a, b), (x, y)):
        assert same_bits(match(eng, p[None], q[None], layout="bkd"), match(eng, p[None], q[None], layout="bdn"))


def test_duplicate_rows_answer_with_the_lowest_index(eng):
    a, b, src, copies = R.duplicate_case()
    m0, m1, s0, s1 = (o[0] for o in match(eng, a[None], b[None]))
    R.Match(a, b).check(m0, m1, s0, s1)
    assert m0[src] == 3 and m1[3] == src and m1[7] == -1 and m1[200] == -1
    assert m1[10] == copies[0] and m0[copies[0]] == 10 and m0[copies[1]] == -1 and m0[copies[2]] == -1
    assert s1[3] == s1[7] == s1[200] == s0[src] and s0[copies[0]] == s0[copies[1]] == s0[copies[2]] == s1[10]    # one similarity, one bit pattern


def test_a_similarity_has_the_same_bits_in_both_directions(eng):
    """every mutual pair's sim0[i] and sim1[j] are the same number computed by the two launches"""
    for name in ("d128", "d256", "d33"):
        a, b = case(name)
        m0, m1, s0, s1 = (o[0] for o in match(eng, a[None], b[None]))
        i = np.nonzero(m0 >= 0)[0]
        assert len(i) and np.array_equal(s0[i].view(np.uint32), s1[m0[i]].view(np.uint32))


def test_nan_inside_a_valid_row(eng):
    a, b = case("d33")
    b = b.copy()
    b[11, 5] = np.nan
    m0, m1, s0, s1 = (o[0] for o in match(eng, a[None], b[None]))
    R.Match(a, b).check(m0, m1, s0, s1)
    assert m1[11] == -1 and s1[11] == 0.0 and not (m0 == 11).any() and np.isfinite(s0).all()


def test_match_invariances(eng):
    """a pair alone, inside a batch, at another position, in a larger frame, after a poisoned workspace and on a second handle"""
    from image_matching_amd.engine import Engine
    a, b = case("d128")
    x, y = case("d256")
    n0, n1 = 200, 257
    want = tuple(o[0] for o in match(eng, padded(a, n0, 257)[None], padded(b, n1, 300)[None], [n0], [n1]))
    other = (padded(a[::-1], 257, 257), padded(b[::-1], 300, 300))
    A = np.stack([other[0], padded(a, n0, 257), other[0]])
    Bm = np.stack([other[1], padded(b, n1, 300), other[1]])
    got = match(eng, A, Bm, [257, n0, 100], [300, n1, 0])
    assert same_bits(want, tuple(o[1] for o in got)), "inside a batch"
    got = match(eng, np.stack([A[1], A[0]]), np.stack([Bm[1], Bm[0]]), [n0, 100], [n1, 0])
    assert same_bits(want, tuple(o[0] for o in got)), "at another position"
    got = match(eng, padded(a, n0, 411)[None], padded(b, n1, 389)[None], [n0], [n1])
    assert same_bits(want, (got[0][0][:257], got[1][0][:300], got[2][0][:257], got[3][0][:300])), "in a larger frame"
    assert (got[0][0][257:] == -1).all() and (got[1][0][300:] == -1).all()
    for p in ("nan", "huge", "zero"):
        match(eng, x[None], y[None])                       # another shape in between
        eng.set_option("debug_poison", p)
        assert same_bits(want, tuple(o[0] for o in match(eng, padded(a, n0, 257)[None], padded(b, n1, 300)[None], [n0], [n1]))), p
    eng.set_option("debug_poison", "off")
    cold = Engine(util.sp_config(256, 64), util.sg_config(256), "cuda")          # another descriptor_dim: D is the call's
    cold.set_option("debug_poison", "nan")
    assert same_bits(want, tuple(o[0] for o in match(cold, padded(a, n0, 257)[None], padded(b, n1, 300)[None], [n0], [n1]))), "a second handle"


def test_the_matcher_refuses_what_it_cannot_read(eng):
    from image_matching_amd.engine import ImxError
    a, b = (torch.from_numpy(v).t()[None] for v in case("d33"))
    for bad in ((a, b.cuda()), (a.cuda(), b), (a.cuda().double(), b.cuda().double()), (a.cuda()[0], b.cuda()[0]), (a.cuda(), b.cuda()[:, :20])):
        with pytest.raises(ImxError):
            eng.mutual_nn_match(*bad)
    with pytest.raises(ImxError):
        eng.mutual_nn_match(a.cuda(), b.cuda(), torch.tensor([70], dtype=torch.int64).cuda(), None)
    big = torch.zeros(1, 1025, 4, device="cuda")
    with pytest.raises(ImxError):
        eng.mutual_nn_match(big, big)


# ------------------------------------------------------------------------------------------------------------ the pair metrics
@functools.lru_cache(maxsize=None)
def metric_case():
    return R.metric_case(21, 3, 257, 300, *R.METRIC_COUNTS)


def metrics(eng, c, eps=EPS, with_matches=True, counts=True, size=None):
    w, h = size or c["size"]
    out = eng.keypoint_pair_metrics(cuda(c["kpts0"]), cuda(c["n0"]) if counts else None, cuda(c["kpts1"]), cuda(c["n1"]) if counts else None,
                                    cuda(c["H"]), (h, w), eps, cuda(c["matches0"]) if with_matches else None)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check_metrics(got, want):
    counts, sums = got
    wc, ws, margin = want
    assert margin > R.EPS_BAND, "a bad case: a decision inside the band"
    assert counts.dtype == np.int32 and np.array_equal(counts, wc), (counts, wc)
    err = np.abs(sums - ws) / np.maximum(wc[:, 2:4], 1)
    print(f"sums at {err.max() / R.SUM_BAR:.2e} of the bar ({R.SUM_BAR} px per point)")
    assert err.max() <= R.SUM_BAR


@pytest.mark.parametrize("with_matches", [True, False])
def test_planted_warps_against_the_reference(eng, with_matches):
    c = metric_case()
    check_metrics(metrics(eng, c, with_matches=with_matches), R.case_metrics(c, EPS, with_matches))


def test_identity_warp_with_identical_point_sets(eng):
    w, h = 640, 480
    rng = np.random.default_rng(8)
    k = rng.uniform([0, 0], [w - 1, h - 1], (3, 300, 2)).astype(np.float32)
    k[0, :6] = [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1], [17, 0], [w - 1, 33.5]]       # on the border: visible
    n = np.array([300, 131, 1], np.int32)
    c = {"kpts0": k, "kpts1": k, "n0": n, "n1": n, "H": np.stack([np.eye(3)] * 3), "size": (w, h),
         "matches0": np.tile(np.arange(300, dtype=np.int64), (3, 1))}
    counts, sums = metrics(eng, c)
    for b in range(3):
        assert list(counts[b]) == [n[b]] * 6 + [0, 0], counts[b]
    assert not sums.any() and not np.signbit(sums).any()
    k2 = k.copy()
    k2[0, 6:8] = [[w - 0.5, 10], [5, -0.25]]                       # outside the image: not visible, still matched and correct
    c2 = dict(c, kpts0=k2, kpts1=k2)
    counts, sums = metrics(eng, c2)
    assert list(counts[0]) == [298, 298, 298, 298, 300, 300, 0, 0] and not sums.any()


def test_singular_and_non_finite_warps_are_bad(eng):
    c = dict(metric_case())
    H = c["H"].copy()
    H[0] = [[1, 2, 3], [2, 4, 6], [0, 0, 1]]
    H[2, 1, 1] = np.inf
    c["H"] = H
    counts, sums = metrics(eng, c)
    want = R.case_metrics(metric_case(), EPS)
    for b in (0, 2):
        assert list(counts[b]) == [0, 0, 0, 0, 0, 0, 1, 0] and not sums[b].any()
    assert np.array_equal(counts[1], want[0][1]) and counts[1, 6] == 0


def test_the_largest_size_is_served_and_the_next_refused(eng):
    from image_matching_amd.engine import ImxError
    c = R.metric_case(33, 1, 4096, 4096, (4096,), (4096,))
    check_metrics(metrics(eng, c, counts=False), R.case_metrics(c, EPS))
    k = torch.zeros(1, 4097, 2, device="cuda")
    for k0, k1 in ((k, k[:, :8]), (k[:, :8], k)):
        with pytest.raises(ImxError, match="4096"):
            eng.keypoint_pair_metrics(k0, None, k1, None, torch.eye(3, dtype=torch.float64, device="cuda")[None], (480, 640))


def test_metric_invariances(eng):
    from image_matching_amd.engine import Engine
    c = metric_case()
    want = metrics(eng, c)

    def sub(idx, K0=257, K1=300):
        out = {"size": c["size"]}
        for key, K, fill in (("kpts0", K0, np.nan), ("kpts1", K1, np.nan), ("matches0", K0, 5)):
            v = c[key][idx]
            big = np.full((len(idx), K) + v.shape[2:], fill, v.dtype)
            big[:, :v.shape[1]] = v
            out[key] = big
        for key in ("n0", "n1", "H"):
            out[key] = c[key][idx]
        return out

    for b in range(3):
        assert same_bits(tuple(o[b:b + 1] for o in want), metrics(eng, sub([b]))), f"pair {b} alone"
    assert same_bits(tuple(o[[2, 0, 1]] for o in want), metrics(eng, sub([2, 0, 1]))), "at other positions"
    assert same_bits(want, metrics(eng, sub([0, 1, 2], 400, 311))), "in a larger frame"
    cold = Engine(util.sp_config(256, 64), util.sg_config(256), "cuda")
    cold.set_option("debug_poison", "nan")
    assert same_bits(want, metrics(cold, c)) and same_bits(want, metrics(eng, c)), "a second handle, a second call"


def test_the_metrics_refuse_what_they_cannot_read(eng):
    from image_matching_amd.engine import ImxError
    c = metric_case()
    k0, k1, H, m = cuda(c["kpts0"]), cuda(c["kpts1"]), cuda(c["H"]), cuda(c["matches0"])
    n0, n1 = cuda(c["n0"]), cuda(c["n1"])
    for args, kw in (((k0.cpu(), n0, k1, n1, H, (480, 640)), {}), ((k0.double(), n0, k1, n1, H, (480, 640)), {}),
                     ((k0, n0, k1, n1, H.float(), (480, 640)), {}), ((k0, n0, k1, n1, H[:2], (480, 640)), {}),
                     ((k0, n0.long(), k1, n1, H, (480, 640)), {}), ((k0, n0, k1, n1, H, (480, 640)), {"matches0": m.int()}),
                     ((k0, n0, k1, n1, H, (480, 640)), {"matches0": m[:, :100]}), ((k0, n0, k1, n1, H, (480, 640)), {"eps": float("nan")}),
                     ((k0, n0, k1, n1, H.cpu(), (480, 640)), {})):
        with pytest.raises(ImxError):
            eng.keypoint_pair_metrics(*args, **kw)
