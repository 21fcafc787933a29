"""Reference for the RANSAC homography fit of include/imx_homog.h, in numpy float64 -- test infrastructure, independent of the kernel's
arithmetic: the integer index draw is restated (being integer it must agree exactly), every four-point system is np.linalg.solve on
the 8 x 8 system, the refit is np.linalg.lstsq and its Gauss-Newton steps are lstsq on J.

What the kernel may decide either way is derived here from the reference alone.  Every hypothesis' residuals are evaluated a second
time -- in np.longdouble with a hand-written elimination where its epsilon is below 1e-18, elsewhere by a second float64 method (the
null vector of the 8 x 9 system by SVD) -- and gamma_h = 1e-9 px + 64 x the largest disagreement is the half-width of the band round
the threshold inside which a point is left to the evaluation.  A hypothesis whose smallest triple area lies in [0.5e-6, 2e-6] may be
ruled degenerate either way."""
import numpy as np

M32 = 0xFFFFFFFF
AREA_MIN = 1e-6
EXTENDED = np.finfo(np.longdouble).eps < 1e-18


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def draw4(seed, h, n):
    """the four distinct indices of hypothesis h among n >= 4 points: an integer hash of (seed, h, n) only; draw k takes one of the
    n - k indices still free, counted in ascending order"""
    s = mix32((seed + 0x9E3779B9 * (h + 1)) & M32)
    s = mix32(s ^ ((0x85EBCA6B * n) & M32))
    picked = []
    for k in range(4):
        if k:
            s = mix32((s + 0x27D4EB2F) & M32)
        i = s % (n - k)
        for t in sorted(picked):
            if i >= t:
                i += 1
        picked.append(i)
    return tuple(picked)


def compact(kpts0, kpts1, matches0, count0=None):
    """the matched pairs in index order: (src (n,2), dst (n,2)) float64 of the fp32 values, and their keypoint0 indices"""
    kpts0, kpts1, matches0 = np.asarray(kpts0), np.asarray(kpts1), np.asarray(matches0)
    K0 = matches0.shape[0]
    c = K0 if count0 is None else min(max(int(count0), 0), K0)
    m = matches0[:c]
    idx = np.nonzero((m >= 0) & (m < kpts1.shape[0]))[0]
    return kpts0[idx].astype(np.float64), kpts1[m[idx]].astype(np.float64), idx


def hartley(p):
    """(cx, cy, s): x_n = (x - c) s takes the centroid to 0 and the mean distance to sqrt 2; s is None where that distance is 0"""
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    return c[0], c[1], (np.sqrt(p.dtype.type(2)) / d if d > 0 and np.isfinite(d) else None)


def normalise(p, nrm):
    return (p - np.array([nrm[0], nrm[1]], p.dtype)) * nrm[2]


def t_matrix(nrm, dtype=np.float64):
    cx, cy, s = nrm
    return np.array([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]], dtype)


def denormalise(Hn, n0, n1):
    return np.linalg.inv(t_matrix(n1)) @ Hn @ t_matrix(n0)


def dlt_rows(x, y, u, v):
    """the two standard DLT rows per point for the unknowns h11 .. h32 with h33 = 1, and their right-hand sides"""
    z, o = np.zeros_like(x), np.ones_like(x)
    A = np.stack([np.stack([x, y, o, z, z, z, -u * x, -u * y], -1), np.stack([z, z, z, x, y, o, -v * x, -v * y], -1)], 1).reshape(-1, 8)
    return A, np.stack([u, v], 1).reshape(-1)


def triple_areas(p4):
    """twice the signed areas of the triples (0,1,2), (0,1,3), (0,2,3), (1,2,3)"""
    out = []
    for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        out.append((p4[j, 0] - p4[i, 0]) * (p4[k, 1] - p4[i, 1]) - (p4[j, 1] - p4[i, 1]) * (p4[k, 0] - p4[i, 0]))
    return np.array(out)


def project(H, p):
    w = H[2, 0] * p[:, 0] + H[2, 1] * p[:, 1] + H[2, 2]
    with np.errstate(all="ignore"):
        q = np.stack([(H[0, 0] * p[:, 0] + H[0, 1] * p[:, 1] + H[0, 2]) / w, (H[1, 0] * p[:, 0] + H[1, 1] * p[:, 1] + H[1, 2]) / w], 1)
    return q, w


def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting, written out so that it runs in np.longdouble (LAPACK has no such type)"""
    A, b = A.copy(), b.copy()
    n = len(b)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]], b[[c, p]] = A[[p, c]], b[[p, c]]
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:] -= f[:, None] * A[c]
        b[c + 1:] -= f * b[c]
    x = np.zeros(n, A.dtype)
    for c in range(n - 1, -1, -1):
        x[c] = (b[c] - A[c, c + 1:] @ x[c + 1:]) / A[c, c]
    return x


def _second_residuals(src, dst, idx4):
    """the residuals and w of the four-point map through idx4, by the second evaluation"""
    if EXTENDED:
        ld = np.longdouble
        s, d = src.astype(ld), dst.astype(ld)
        n0, n1 = hartley(s), hartley(d)
        a, b = normalise(s, n0), normalise(d, n1)
        A, rhs = dlt_rows(a[idx4, 0], a[idx4, 1], b[idx4, 0], b[idx4, 1])
        Hn = np.append(_solve_ld(A, rhs), ld(1)).reshape(3, 3)
        q, w = project(Hn, a)
        return np.sqrt((((q - b) / n1[2]) ** 2).sum(1)).astype(np.float64), w.astype(np.float64)
    n0, n1 = hartley(src), hartley(dst)
    a, b = normalise(src, n0), normalise(dst, n1)
    A, rhs = dlt_rows(a[idx4, 0], a[idx4, 1], b[idx4, 0], b[idx4, 1])
    v = np.linalg.svd(np.concatenate([A, -rhs[:, None]], 1))[2][-1]
    H = denormalise((v / v[8]).reshape(3, 3), n0, n1)
    q, w = project(H, src)
    return np.sqrt(((q - dst) ** 2).sum(1)), w            # (the third row of T1^-1 is (0, 0, 1): w is the normalised problem's, h33 = 1 there)


class Hypothesis:
    """One hypothesis of a pair, as the reference sees it.  degenerate: True, False, or None where it may be ruled either way.  sure_in /
    sure_out: the matched points that must / must not be in its mask at threshold thr; nL, nU: the bounds of its inlier count (-1 for a
    degenerate one)."""

    def __init__(self, src, dst, n0, n1, seed, h, thr):
        n = len(src)
        self.h, self.idx = h, np.array(draw4(seed, h, n))
        a, b = normalise(src, n0)[self.idx], normalise(dst, n1)[self.idx]
        ta, tb = triple_areas(a), triple_areas(b)
        small = min(np.abs(ta).min(), np.abs(tb).min())
        flipped = bool(np.any((ta > 0) != (tb > 0)))
        self.own_degenerate = bool(small < AREA_MIN or flipped)          # the reference's own float64 ruling
        self.sure_in = self.sure_out = np.zeros(n, bool)
        self.undecided = np.zeros(n, bool)
        if small < 0.5 * AREA_MIN or (flipped and small > 2 * AREA_MIN):
            self.degenerate, self.nL, self.nU = True, -1, -1
            return
        self.degenerate = None if small <= 2 * AREA_MIN else False
        A, rhs = dlt_rows(a[:, 0], a[:, 1], b[:, 0], b[:, 1])
        try:
            self.Hn = np.append(np.linalg.solve(A, rhs), 1.0).reshape(3, 3)
        except np.linalg.LinAlgError:           # the horizon through the centroid: h33 = 1 has no solution; anything goes
            self.degenerate, self.own_degenerate, self.nL, self.nU, self.undecided = None, True, -1, n, np.ones(n, bool)
            return
        self.H = denormalise(self.Hn, n0, n1)
        q, w = project(self.H, src)
        e = np.sqrt(((q - dst) ** 2).sum(1))
        e2, w2 = _second_residuals(src, dst, self.idx)
        with np.errstate(all="ignore"):
            dis = np.abs(e - e2)
        dis = np.where(np.isfinite(dis), dis, np.inf)
        self.gamma = 1e-9 + 64.0 * float(dis.max())
        w_pos, w_neg = (w > 1e-9) & (w2 > 1e-9), (w < -1e-9) & (w2 < -1e-9)
        self.e = e
        self.sure_in = w_pos & (e < thr - self.gamma)
        self.sure_out = w_neg | (w_pos & (e > thr + self.gamma))
        self.undecided = ~(self.sure_in | self.sure_out)
        self.nL = -1 if self.degenerate is None else int(self.sure_in.sum())
        self.nU = n - int(self.sure_out.sum())


class Pair:
    """The reference's view of one pair: the compaction, the normalisation, and every hypothesis on demand"""

    def __init__(self, kpts0, kpts1, matches0, count0, thr, hypotheses, seed):
        self.src, self.dst, self.index0 = compact(kpts0, kpts1, matches0, count0)
        self.K0, self.n, self.thr, self.hypotheses, self.seed = len(matches0), len(self.src), float(thr), int(hypotheses), int(seed) & M32
        self.ok = self.n >= 4
        if self.ok:
            self.n0, self.n1 = hartley(self.src), hartley(self.dst)
            self.ok = self.n0[2] is not None and self.n1[2] is not None
        self._hyp = {}

    def hyp(self, h):
        if h not in self._hyp:
            self._hyp[h] = Hypothesis(self.src, self.dst, self.n0, self.n1, self.seed, h, self.thr)
        return self._hyp[h]

    def check_winner(self, best_h):
        """the reported best_h must not be certainly beaten: no h' with nL(h') > nU(best_h), and no h' < best_h with nL(h') >= nU(best_h)"""
        assert 0 <= best_h < self.hypotheses, best_h
        w = self.hyp(best_h)
        assert w.degenerate is not True, f"hypothesis {best_h} is degenerate"
        for h in range(self.hypotheses):
            o = self.hyp(h)
            assert not o.nL > w.nU, (h, o.nL, best_h, w.nU)
            assert not (h < best_h and o.nL >= w.nU), (h, o.nL, best_h, w.nU)

    def check_mask(self, best_h, mask):
        """the band rule for the reported winner's mask (keypoint0 index space); more than 1 % undecided points is a bad CASE"""
        w = self.hyp(best_h)
        assert w.undecided.sum() <= 0.01 * self.n, f"bad case: {int(w.undecided.sum())} of {self.n} points undecided (gamma {w.gamma:g})"
        mask = np.asarray(mask).astype(bool)
        compacted = mask[self.index0]
        assert mask.sum() == compacted.sum(), "the mask marks an unmatched slot"
        assert np.all(compacted[w.sure_in]), "a certain inlier is missing from the mask"
        assert not np.any(compacted[w.sure_out]), "a certain outlier is in the mask"
        return compacted

    def refit(self, compacted_mask, refine_iters=3):
        """the refit on a given inlier set (a mask over the compacted points): lstsq on the DLT rows in normalised coordinates (h33 = 1),
        then refine_iters Gauss-Newton steps, lstsq on J; back to pixels with H[2,2] = 1.  None where the result is not finite"""
        a, b = normalise(self.src, self.n0)[compacted_mask], normalise(self.dst, self.n1)[compacted_mask]
        A, rhs = dlt_rows(a[:, 0], a[:, 1], b[:, 0], b[:, 1])
        g = np.linalg.lstsq(A, rhs, rcond=None)[0]
        for _ in range(int(refine_iters)):
            x, y = a[:, 0], a[:, 1]
            iw = 1.0 / (g[6] * x + g[7] * y + 1.0)
            qx, qy = (g[0] * x + g[1] * y + g[2]) * iw, (g[3] * x + g[4] * y + g[5]) * iw
            J, r = dlt_rows(x * iw, y * iw, qx, qy)          # [x/w y/w 1/w 0 0 0 -qx x/w -qx y/w] and its partner
            J[0::2, 2], J[1::2, 5] = iw, iw
            res = np.stack([qx - b[:, 0], qy - b[:, 1]], 1).reshape(-1)
            g = g + np.linalg.lstsq(J, -res, rcond=None)[0]
        H = denormalise(np.append(g, 1.0).reshape(3, 3), self.n0, self.n1)
        if not np.all(np.isfinite(H)) or abs(H[2, 2]) < 1e-12 * np.linalg.norm(H):
            return None
        return H / H[2, 2]

    def estimate(self, refine_iters=3):
        """the whole fit by the reference's own float64 decisions: (H or None, mask (K0) bool, n_inliers, best_h)"""
        fail = (None, np.zeros(self.K0, bool), 0, -1)
        if not self.ok:
            return fail
        best, best_n = -1, -1
        for h in range(self.hypotheses):
            o = self.hyp(h)
            if o.own_degenerate:
                continue
            q, w = project(o.H, self.src)
            c = int(((w > 0) & (((q - self.dst) ** 2).sum(1) < self.thr ** 2)).sum())
            if c > best_n:
                best, best_n = h, c
        if best_n < 4:
            return fail
        o = self.hyp(best)
        q, w = project(o.H, self.src)
        inl = (w > 0) & (((q - self.dst) ** 2).sum(1) < self.thr ** 2)
        H = self.refit(inl, refine_iters)
        if H is None:
            return fail
        mask = np.zeros(self.K0, bool)
        mask[self.index0[inl]] = True
        return H, mask, best_n, best


def corners(width, height):
    return np.array([[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]], np.float64)


def corner_distances(H_a, H_b, width, height):
    """the distances of the four image corners under two homographies"""
    c = corners(width, height)
    return np.sqrt(((project(np.asarray(H_a, np.float64).reshape(3, 3), c)[0] - project(np.asarray(H_b, np.float64).reshape(3, 3), c)[0]) ** 2).sum(1))


def corner_error(H_est, H_gt, width, height):
    """imx_homography_corner_error for one pair: the mean corner distance, +inf for an all-zero H_est or a value that is not finite"""
    H_est = np.asarray(H_est, np.float64)
    if not H_est.any():
        return np.inf
    with np.errstate(all="ignore"):
        v = corner_distances(H_est, H_gt, width, height).mean()
    return float(v) if np.isfinite(v) else np.inf


REFIT_BAR = 1e-7      # px at the four image corners, kernel's H against refit() on the kernel's own inlier set (the issue derives it: two
                      # float64 solutions of one normalised problem differ by at most 4.2e-12 px there; an fp32 accumulation sits at 1e-4)


def planted_case(seed, B, K0, K1, counts0, size=(640, 480), noise=0.0, outlier_every=7, unmatched_every=3):
    """B pairs of K0 / K1 keypoint slots related by random perspective warps of a (width, height) image: every `unmatched_every`-th slot
    unmatched, every `outlier_every`-th match moved 30 to 130 px off, optional Gaussian noise on the rest.  Continuous random
    coordinates.  Returns dict of numpy arrays: kpts0, kpts1 fp32, matches0 int64, counts0 int32, H_gt (B,3,3), planted (B,K0) bool (the
    matched, unmoved slots below counts0)."""
    rng = np.random.default_rng(seed)
    W, Hh = size
    kpts0 = np.stack([rng.uniform(0, W - 1, (B, K0)), rng.uniform(0, Hh - 1, (B, K0))], -1)
    kpts1 = np.stack([rng.uniform(0, W - 1, (B, K1)), rng.uniform(0, Hh - 1, (B, K1))], -1)
    matches0 = np.full((B, K0), -1, np.int64)
    planted = np.zeros((B, K0), bool)
    H_gt = np.zeros((B, 3, 3))
    for b in range(B):
        c = corners(W, Hh)
        A, rhs = dlt_rows(c[:, 0], c[:, 1], *(c + rng.uniform(-0.12, 0.12, (4, 2)) * [W, Hh]).T)
        H_gt[b] = np.append(np.linalg.solve(A, rhs), 1.0).reshape(3, 3)
        perm = rng.permutation(K1)
        for i in range(min(K0, K1)):
            if i % unmatched_every == unmatched_every - 1:
                continue
            j = perm[i]
            matches0[b, i] = j
            q = project(H_gt[b], kpts0[b, i:i + 1])[0][0]
            if i % outlier_every == outlier_every - 1:
                ang, r = rng.uniform(0, 2 * np.pi), rng.uniform(30, 130)
                q = q + r * np.array([np.cos(ang), np.sin(ang)])
            else:
                q = q + noise * rng.standard_normal(2)
                planted[b, i] = i < counts0[b]
            kpts1[b, j] = q
    return {"kpts0": kpts0.astype(np.float32), "kpts1": kpts1.astype(np.float32), "matches0": matches0,
            "counts0": np.asarray(counts0, np.int32), "H_gt": H_gt, "planted": planted, "size": size}
