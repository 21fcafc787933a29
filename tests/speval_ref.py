"""numpy float64 reference of libimx_speval.so (include/imx_speval.h): the mutual nearest-neighbour matcher and the pair metrics under a
known warp.  It shares no arithmetic with the kernels: a plain `a @ b.T`, np.linalg.inv and dense distance matrices.

What a kernel may decide either way, and nothing else:
  the matcher  an fp32 dot product of D terms differs from the exact one by at most (D + 2) 2^-24 |a| |b| (the standard bound with a
               first-order constant, two terms of slack); GAMMA is twice that.  The kernel's row maximum is within GAMMA of the float64
               one, and the index it reports has a float64 similarity within 2 GAMMA of the best: the CANDIDATES of the row.  A row whose
               candidates are one descriptor (one row, or bit-identical copies of it) is DECIDED: the answer is the lowest candidate,
               exactly.  Any other row is in the band; more than max(2, 1 %) of a side's rows there reject the case.
  the metrics  every decision (w > 0, inside the image border, d <= eps) whose float64 margin is above 1e-9 px is certain: float64
               arithmetic of a dozen operations on coordinates below 2^13 errs by 1e-12 at the most.  The fixtures leave no decision
               inside that band (asserted by tests/test_speval_host.py), so the integer outputs must be equal.
"""
import numpy as np

EPS_BAND = 1e-9          # px: the band round eps, round the image border and round w = 0
SUM_BAR = 1e-9           # px per point: what the sums of nearest distances may differ by


# ------------------------------------------------------------------------------------------------------------ the matcher
def unit_rows(rng, n, d):
    a = rng.standard_normal((n, d))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def descriptor_case(seed, D, N0, N1):
    """unit Gaussian rows; the first half of side 1 are noisy copies (0.3 / sqrt D per channel, renormalised) of distinct rows of side 0,
    in a shuffled order.  fp32, as the kernel reads them."""
    rng = np.random.default_rng(seed)
    a = unit_rows(rng, N0, D)
    b = unit_rows(rng, N1, D)
    h = min(N1 // 2, N0)
    src = rng.permutation(N0)[:h]
    c = a[src] + rng.standard_normal((h, D)) * (0.3 / np.sqrt(D))
    b[:h] = c / np.linalg.norm(c, axis=1, keepdims=True)
    return a.astype(np.float32), b.astype(np.float32)


def gamma(a, b):
    """(N0, N1): twice the bound of an fp32 dot product of D terms"""
    D = a.shape[1]
    na, nb = np.linalg.norm(a.astype(np.float64), axis=1), np.linalg.norm(b.astype(np.float64), axis=1)
    return 2.0 * (D + 2) * 2.0 ** -24 * na[:, None] * nb[None, :]


class Side:
    """one direction of the search over float64 similarities S (Nq, Nk) with bounds G: per row the float64 best, the candidate
    sets and whether the row is decided"""

    def __init__(self, S, G, keys):
        self.n = S.shape[0]
        self.best = np.zeros(self.n)                      # the float64 row maximum over comparable entries (0: none)
        self.g = np.zeros(self.n)                         # the row's bound
        self.nn = np.full(self.n, -1, np.int64)           # the decided answer (lowest candidate), -1: no neighbour; meaningless in the band
        self.cand = []
        self.decided = np.ones(self.n, bool)
        for i in range(self.n):
            ok = ~np.isnan(S[i]) if S.shape[1] else np.zeros(0, bool)
            if not ok.any():
                self.cand.append(np.zeros(0, np.int64))
                continue
            s = np.where(ok, S[i], -np.inf)
            self.best[i] = s.max()
            self.g[i] = np.nanmax(np.where(ok, G[i], 0.0))
            c = np.nonzero(ok & (s >= self.best[i] - 2.0 * self.g[i]))[0]
            self.cand.append(c)
            self.nn[i] = c[0]
            self.decided[i] = all(np.array_equal(keys[c[0]].view(np.uint32), keys[j].view(np.uint32)) for j in c[1:])

    def band_rows(self):
        return int((~self.decided).sum())


class Match:
    """the reference's view of one pair: a (N0, D), b (N1, D) fp32, counts n0, n1"""

    def __init__(self, a, b, n0=None, n1=None):
        self.n0 = a.shape[0] if n0 is None else int(n0)
        self.n1 = b.shape[0] if n1 is None else int(n1)
        self.N0, self.N1 = a.shape[0], b.shape[0]
        a, b = a[:self.n0], b[:self.n1]
        with np.errstate(invalid="ignore"):
            S = a.astype(np.float64) @ b.astype(np.float64).T
            G = gamma(a, b)
        self.S = S
        self.s0, self.s1 = Side(S, G, b), Side(S.T, G.T, a)

    def fair(self):
        """the case leaves at most max(2, 1 %) of each side's rows undecided"""
        return all(s.band_rows() <= max(2, s.n // 100) for s in (self.s0, self.s1))

    def check(self, m0, m1, sim0, sim1):
        """the kernel's outputs of this pair (full frames) against the rules; returns the largest |sim - best| / gamma seen"""
        assert self.fair(), "a bad case: too many rows inside the band"
        worst = 0.0
        for s, o, m, mo, sim, n, N in ((self.s0, self.s1, m0, m1, sim0, self.n0, self.N0), (self.s1, self.s0, m1, m0, sim1, self.n1, self.N1)):
            assert m.shape == (N,) and sim.shape == (N,)
            assert np.all(m[n:] == -1) and not sim[n:].any(), "rows past the count hold -1 / 0"
            for i in range(n):
                c = s.cand[i]
                if len(c) == 0:                            # no comparable similarity (or no key at all)
                    assert m[i] == -1 and sim[i] == 0.0, i
                    continue
                err = abs(float(sim[i]) - s.best[i])
                assert err <= s.g[i], (i, err, s.g[i])
                if s.g[i] > 0:
                    worst = max(worst, err / s.g[i])
                j = int(m[i])
                assert j == -1 or j in c, (i, j, c)
                if j >= 0:
                    assert mo[j] == i, "matches0[i] == j exactly where matches1[j] == i"
                if s.decided[i] and o.decided[c[0]]:       # both searches are certain: so is the mutual test
                    want = c[0] if o.nn[c[0]] == i else -1
                    assert j == want, (i, j, want)
        return worst


# ------------------------------------------------------------------------------------------------------------ the pair metrics
def project(H, p):
    """p (n, 2) float64 -> ((n, 2) positions, (n) w)"""
    q = np.concatenate([p, np.ones((len(p), 1))], axis=1) @ H.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return q[:, :2] / q[:, 2:3], q[:, 2]


def _visible(xy, w, width, height, margins):
    x, y = xy[:, 0], xy[:, 1]
    with np.errstate(invalid="ignore"):
        vis = (w > 0) & (x >= 0) & (x <= width - 1) & (y >= 0) & (y <= height - 1)
    pos = w > 0
    # a point exactly ON the border is exact in float64 under an identity warp and counts as visible: its margin is 0 by construction, so
    # only non-zero margins are reported
    for v in (w, x[pos], (width - 1) - x[pos], y[pos], (height - 1) - y[pos]):
        margins.extend(np.abs(v[np.isfinite(v) & (v != 0)]).tolist())
    return vis


def pair_metrics(k0, n0, k1, n1, H, width, height, eps, matches0=None):
    """one pair.  Returns (counts (8) int64, sums (2) float64, margin): margin is the smallest distance of any decision from its
    boundary (eps, the border, w = 0), decisions that sit exactly on the border excepted"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    det = np.linalg.det(H)
    if not (np.isfinite(det) and det != 0 and np.all(np.isfinite(H))):
        return np.array([0, 0, 0, 0, 0, 0, 1, 0]), np.zeros(2), np.inf
    margins = []
    p0, p1 = k0[:n0].astype(np.float64), k1[:n1].astype(np.float64)
    w0, ww0 = project(H, p0)
    w1, ww1 = project(np.linalg.inv(H), p1)
    vis0, vis1 = _visible(w0, ww0, width, height, margins), _visible(w1, ww1, width, height, margins)
    a, b = w0[vis0], p1[vis1]                                    # both in image 1
    counts, sums = np.zeros(8, np.int64), np.zeros(2)
    counts[0], counts[1] = vis0.sum(), vis1.sum()
    if len(a) and len(b):
        dist = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
        for k, d in enumerate((dist.min(axis=1), dist.min(axis=0))):
            counts[2 + k] = (d <= eps).sum()
            sums[k] = d[d <= eps].sum()
            margins.extend(np.abs(d - eps).tolist())
    if matches0 is not None:
        m = np.asarray(matches0[:n0])
        ok = (m >= 0) & (m < n1)
        counts[4] = ok.sum()
        i = np.nonzero(ok)[0]
        with np.errstate(invalid="ignore"):
            d = np.sqrt(((w0[i] - p1[m[i]]) ** 2).sum(-1))
            counts[5] = ((ww0[i] > 0) & (d <= eps)).sum()
        margins.extend(np.abs(d[np.isfinite(d)] - eps).tolist())
    return counts, sums, (min(margins) if margins else np.inf)


def random_homography(rng, width, height, strength=1.0):
    """a warp of pixel coordinates near the identity: a rotation, a scale, a shift and a little perspective, so that a part of either
    image leaves the other's view"""
    t = rng.uniform(-0.25, 0.25) * strength
    s = 1.0 + rng.uniform(-0.15, 0.15) * strength
    c = np.array([[1, 0, width / 2], [0, 1, height / 2], [0, 0, 1.0]])
    A = np.array([[s * np.cos(t), -s * np.sin(t), rng.uniform(-40, 40) * strength], [s * np.sin(t), s * np.cos(t), rng.uniform(-30, 30) * strength],
                  [rng.uniform(-2e-4, 2e-4) * strength, rng.uniform(-2e-4, 2e-4) * strength, 1.0]])
    H = c @ A @ np.linalg.inv(c)
    return H / H[2, 2]


def metric_case(seed, B, K0, K1, counts0, counts1, size=(640, 480)):
    """B pairs: kpts0 uniform over a frame somewhat larger than the image's interior, the first part of kpts1 the warped kpts0 (shuffled)
    moved by 0 to 6 px, the rest uniform; matches0 the planted correspondence with a fifth unmatched, a tenth wrong and a few indices
    past the count.  Slots past the counts hold NaN / a wild index."""
    width, height = size
    rng = np.random.default_rng(seed)
    k0 = np.full((B, K0, 2), np.nan, np.float32)
    k1 = np.full((B, K1, 2), np.nan, np.float32)
    m0 = np.full((B, K0), 1 << 40, np.int64)
    Hs = np.stack([random_homography(rng, width, height) for _ in range(B)])
    for b in range(B):
        n0, n1 = counts0[b], counts1[b]
        p = rng.uniform([-10, -10], [width + 10, height + 10], (n0, 2)).astype(np.float32)
        k0[b, :n0] = p
        q = rng.uniform([0, 0], [width - 1, height - 1], (n1, 2))
        h = min(n0, (2 * n1) // 3)
        src = rng.permutation(n0)[:h]
        slot = rng.permutation(n1)[:h]
        w, _ = project(Hs[b], p[src].astype(np.float64))
        ang, rad = rng.uniform(0, 2 * np.pi, h), rng.uniform(0, 6, h)
        q[slot] = w + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
        k1[b, :n1] = q.astype(np.float32)
        m = np.full(n0, -1, np.int64)
        m[src] = slot
        r = rng.uniform(size=n0)
        m[r < 0.2] = -1
        wrong = (r > 0.9) & (n1 > 0)
        m[wrong] = rng.integers(0, max(n1, 1), int(wrong.sum()))
        m[(r > 0.2) & (r < 0.23)] = n1 + 3                       # inside the frame or not, past the count: unmatched
        m0[b, :n0] = m
    return {"kpts0": k0, "kpts1": k1, "matches0": m0, "H": Hs, "n0": np.asarray(counts0, np.int32), "n1": np.asarray(counts1, np.int32),
            "size": size}


def case_metrics(case, eps, with_matches=True):
    """the reference over a whole case: counts (B,8), sums (B,2), the smallest margin"""
    out = [pair_metrics(case["kpts0"][b], int(case["n0"][b]), case["kpts1"][b], int(case["n1"][b]), case["H"][b], case["size"][0],
                        case["size"][1], eps, case["matches0"][b] if with_matches else None) for b in range(len(case["H"]))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), min(o[2] for o in out)


# ------------------------------------------------------------------------------------------------------------ the shared cases
# name -> (seed, D, N0, N1): what tests/test_speval_host.py shows to be fair and tests/test_gpu_speval.py runs
MATCH_CASES = {"d128": (1, 128, 257, 300), "d64_two_row_blocks": (3, 64, 1000, 1023), "d256": (2, 256, 130, 65), "d33": (4, 33, 70, 90),
               "d1": (5, 1, 40, 50)}
RAGGED = ((257, 300), (0, 150), (1, 200))          # the counts of the B = 3 case at D = 128: a full pair, an empty side, a single row
METRIC_COUNTS = ((257, 100, 0), (300, 1, 37))      # counts0, counts1 of the B = 3 metric case at K = 257 / 300


def duplicate_case():
    """the d128 case with bit-identical duplicate rows planted on both sides: key 3 of side 1 (a noisy copy of some row `src` of side
    0) again at 7 and 200, and the row `q` of side 0 that key 10 copies again at two other rows.  Returns a, b, src and the three copies
    of q in ascending order."""
    a, b = descriptor_case(*MATCH_CASES["d128"])
    b[7] = b[3]
    b[200] = b[3]
    S = a.astype(np.float64) @ b.astype(np.float64).T
    src, q = int(np.argmax(S[:, 3])), int(np.argmax(S[:, 10]))
    spots = [i for i in (5, 256, 131) if i not in (src, q)][:2]
    for i in spots:
        a[i] = a[q]
    return a, b, src, sorted(spots + [q])
