"""TEST INFRASTRUCTURE (checker only) -- an exact-arithmetic reference of the registration post-step (csrc/registration.hip):
what ANY correct fp32 evaluation of the RANSAC partial-affine fit may return, and a float64 brute-force 2-NN search.

oracle/ransac_ref.py is an unfused fp32 restatement of the kernel; the device contracts products and sums to FMAs, so the two agree
bit for bit only where no residual comes near the threshold.  This helper does not restate the kernel's arithmetic: it evaluates
every hypothesis of the shared counter-based sequence (oracle.ransac_ref._pair) in float64 and puts a derived error band round the
threshold, so that a point is required in the mask, forbidden, or -- inside the band -- left to the evaluation.  Pure numpy, float64,
no GPU and no torch."""
import numpy as np

from oracle import ransac_ref

U24 = 2.0 ** -24                     # half a spacing of an fp32 number in [1, 2): the largest relative error of one fp32 rounding
RANSAC_ATOL, RANSAC_RTOL = 2e-4, 1e-5   # the project's bar on the fitted matrix (tests/test_gpu_registration.py)
UNDECIDED_CAP = 0.01                 # the band of the winning hypothesis may hold at most this share of the matched points


class RansacCheckError(AssertionError):
    """the output is not one a correct evaluation of the RANSAC fit can give"""


class BadCase(AssertionError):
    """the case leaves too much undecided (or breaks its own premise) to test anything: rejected, not passed"""


# ---------------------------------------------------------------------------------------------- bands
class Hypothesis:
    __slots__ = ("h", "i", "j", "model", "e", "gamma", "exact", "L", "U", "nL", "nU")


class Bands:
    """hypothesis_bands' result: `valid` (the keypoint0 rows of the matched points, in index order), `src` / `dst` (n,2) float64,
    `hyp` (one Hypothesis or None per hypothesis index), and the call's parameters."""
    __slots__ = ("K", "valid", "src", "dst", "hyp", "thresh", "b", "seed")

    @property
    def n(self):
        return len(self.valid)

    @property
    def live(self):
        return [q for q in self.hyp if q is not None]


def hypothesis_bands(kpts0, kpts1, matches0, b, thresh, hypotheses, seed, counts0=None):
    """For every hypothesis h of oracle.ransac_ref._pair(seed, b, h, n): the similarity (ca, cb, tx, ty) through the two sampled
    matches and the residual length e_k of every matched point, in float64 from the fp32 coordinates, and the two inlier sets
        L(h) = {k : e_k < thresh - gamma_h}   (inliers of every correct fp32 evaluation)
        U(h) = {k : e_k < thresh + gamma_h}   (nothing outside may be an inlier)
    with their sizes; None for a degenerate pair (den <= 1e-12).  Fewer than four matches: no hypothesis at all (`hyp` is empty).

    gamma_h = 16 * 2^-24 * ((|ca| + |cb|) * 2 X + |tx| + |ty| + U),   X = max_k (|x_k| + |y_k|),   U = max |kpts1|
    is the a-priori forward error bound of an fp32 evaluation of the model and of one residual vector, fused or not.  It is DERIVED,
    not measured: from the coordinates to a residual component the kernel's expressions take at most about 13 roundings (the two
    coordinate differences, the products and sums of the numerator, the quotient, the products and sums of the translation, and again
    those of the residual; an FMA only removes some).  Each is at most half a spacing, i.e. 2^-24, of a partial result, and no partial
    is larger than the bracket: |ca x|, |cb y| <= (|ca| + |cb|) X, the translation, a destination coordinate.  The relative error of
    ca and cb themselves stays a few 2^-24 of |ca| + |cb| however short the sampled baseline is, because numerator and denominator
    shrink together.  The two components of the residual give a factor sqrt 2 on its length; 16 covers 13 sqrt 2 with the slack that
    most partials sit far below the bracket.  The squaring, the sum of squares and the comparison with thresh^2 add two more
    roundings RELATIVE to e^2 (about 1e-7 of e): below a thousandth of the band.  Measured on the host: the unfused fp32
    restatement uses at most 0.061 of gamma; gamma is 0.002 to 0.02 px on the suite's cases.

    One exception, also derived: where the coordinates, the model and every partial result are integers below 2^24 (_all_exact: a
    lattice case under a model with integer coefficients), no fp32 operation rounds at all, fused or not -- a correctly rounded
    quotient with a representable value is that value -- so gamma_h = 0 and e^2 < thresh^2 is decided exactly, e == thresh included."""
    k0 = np.asarray(kpts0, np.float32).astype(np.float64)
    k1 = np.asarray(kpts1, np.float32).astype(np.float64)
    m = np.asarray(matches0).astype(np.int64)
    K = len(m)
    ok = m >= 0
    if counts0 is not None:
        ok &= np.arange(K) < int(counts0)
    out = Bands()
    out.K, out.valid, out.thresh, out.b, out.seed = K, np.nonzero(ok)[0], float(thresh), int(b), int(seed)
    out.src, out.dst = k0[out.valid], k1[m[out.valid]]
    out.hyp = []
    n = out.n
    if n <= 3:
        return out
    s, d = out.src, out.dst
    X = float((np.abs(s[:, 0]) + np.abs(s[:, 1])).max())
    U = float(np.abs(k1).max())
    lattice = bool((s == np.rint(s)).all() and (d == np.rint(d)).all())
    for h in range(int(hypotheses)):
        i, j = ransac_ref._pair(seed, b, h, n)
        px, py = s[j] - s[i]
        qx, qy = d[j] - d[i]
        den = px * px + py * py
        if den <= 1e-12:
            out.hyp.append(None)
            continue
        ca, cb = (qx * px + qy * py) / den, (qy * px - qx * py) / den
        tx = d[i, 0] - (ca * s[i, 0] - cb * s[i, 1])
        ty = d[i, 1] - (cb * s[i, 0] + ca * s[i, 1])
        ex = ca * s[:, 0] - cb * s[:, 1] + tx - d[:, 0]
        ey = cb * s[:, 0] + ca * s[:, 1] + ty - d[:, 1]
        q = Hypothesis()
        q.h, q.i, q.j, q.model = h, i, j, (ca, cb, tx, ty)
        q.e = np.hypot(ex, ey)
        q.exact = lattice and _all_exact(px, py, qx, qy, den, q.model, X, U, ex, ey)
        q.gamma = 0.0 if q.exact else 16 * U24 * ((abs(ca) + abs(cb)) * 2 * X + abs(tx) + abs(ty) + U)
        q.L, q.U = q.e < thresh - q.gamma, q.e < thresh + q.gamma
        q.nL, q.nU = int(q.L.sum()), int(q.U.sum())
        out.hyp.append(q)
    return out


def _all_exact(px, py, qx, qy, den, model, X, U, ex, ey):
    """Integer coordinates (checked by the caller), integer model, and every partial of the kernel's expressions below 2^24 in
    magnitude: all of them are representable, so no fp32 operation, contracted or not, rounds."""
    ca, cb, tx, ty = model
    if any(v != np.rint(v) for v in model):
        return False
    lim = 2.0 ** 24
    numer = 2 * max(abs(px), abs(py)) * max(abs(qx), abs(qy))
    resid = (abs(ca) + abs(cb)) * X + abs(tx) + abs(ty) + U
    return bool(den < lim and numer < lim and resid < lim and 2 * max(np.abs(ex).max(), np.abs(ey).max()) ** 2 < lim)


def fit_similarity(p, q):
    """The least-squares similarity q ~ [a -b; b a] p + t by np.linalg.lstsq on the stacked 2n x 4 system [x -y 1 0; y x 0 1] --
    NOT the centred closed form that the kernel and oracle/ransac_ref.py share.  Returns the (2,3) float64 matrix."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    n = len(p)
    A = np.zeros((2 * n, 4))
    A[:n, 0], A[:n, 1], A[:n, 2] = p[:, 0], -p[:, 1], 1.0
    A[n:, 0], A[n:, 1], A[n:, 3] = p[:, 1], p[:, 0], 1.0
    (a, b, tx, ty), *_ = np.linalg.lstsq(A, np.concatenate([q[:, 0], q[:, 1]]), rcond=None)
    return np.array([[a, -b, tx], [b, a, ty]])


def output_of_hypothesis(bands, h):
    """(M, mask, n_inliers) as the fit would return them had hypothesis h won, decided in float64 at the threshold itself."""
    q = bands.hyp[h]
    inl = q.e < bands.thresh
    mask = np.zeros(bands.K, np.uint8)
    mask[bands.valid[inl]] = 1
    return fit_similarity(bands.src[inl], bands.dst[inl]).astype(np.float32), mask, int(inl.sum())


def check_ransac_output(bands, M, mask, n_inliers, pair=None):
    """Raises RansacCheckError unless (M (2,3), mask (K,), n_inliers) is an output a correct fp32 evaluation can give for `bands`:
      (a) n_inliers == mask.sum(), and mask is 0 on unmatched rows and on rows past counts0;
      (b) mask.sum() >= max_h |L(h)|: no hypothesis has definitely more inliers than the winner;
      (c) some h has L(h) <= mask <= U(h) and |L(h')| < mask.sum() for every h' < h (the first best wins: `cnt > best_cnt`);
      (d) M is the least-squares similarity over exactly the rows of mask (fit_similarity), at atol 2e-4, rtol 1e-5.
    With fewer than four matches, only degenerate hypotheses, or a best |U| below 2, only the all-zero output passes.  The undecided
    set U(h) minus L(h) of the hypothesis found in (c) may hold at most 1 % of the matched points: beyond that BadCase is raised --
    such a case is rejected, not passed.  Every message names the pair, the hypothesis and the point.  Returns a dict of what was
    found: h, undecided, second (the largest |L| of another hypothesis), n."""
    pair = bands.b if pair is None else pair
    M = np.asarray(M, np.float64).reshape(2, 3)
    mask = np.asarray(mask).astype(np.int64).reshape(-1)
    n_inliers = int(n_inliers)
    who = f"pair {pair}"
    if len(mask) != bands.K:
        raise RansacCheckError(f"{who}: mask of {len(mask)} rows for {bands.K} keypoints")
    if set(np.unique(mask)) - {0, 1}:
        raise RansacCheckError(f"{who}: the mask holds values other than 0 and 1: {np.unique(mask)[:6]}")
    total = int(mask.sum())
    if n_inliers != total:
        raise RansacCheckError(f"{who}: n_inliers {n_inliers} but the mask holds {total}")
    allowed = np.zeros(bands.K, bool)
    allowed[bands.valid] = True
    stray = np.nonzero((mask == 1) & ~allowed)[0]
    if len(stray):
        raise RansacCheckError(f"{who}: point {int(stray[0])} is unmatched (or past counts0) and set in the mask ({len(stray)} such rows)")
    live = bands.live
    best_U = max((q.nU for q in live), default=0)
    best_L = max((q.nL for q in live), default=0)
    zeros = total == 0 and not M.any()
    if best_U < 2:
        if not zeros:
            raise RansacCheckError(f"{who}: no hypothesis can reach two inliers ({bands.n} matches, {len(live)} non-degenerate hypotheses): "
                                   f"the output must be all zero, got {total} inliers, M {M.ravel()}")
        return {"h": None, "undecided": 0, "second": 0, "n": bands.n}
    if total == 0:
        if best_L >= 2 or not zeros:
            q = max(live, key=lambda q: q.nL)
            raise RansacCheckError(f"{who}: empty mask, but hypothesis {q.h} has {q.nL} definite inliers, first of them point {int(bands.valid[np.nonzero(q.L)[0][0]])}"
                                   if best_L >= 2 else f"{who}: empty mask with a non-zero M {M.ravel()}")
        return {"h": None, "undecided": 0, "second": best_L, "n": bands.n}
    # (b)
    for q in live:
        if q.nL > total:
            miss = np.nonzero(q.L & (mask[bands.valid] == 0))[0]
            raise RansacCheckError(f"{who}: hypothesis {q.h} has {q.nL} definite inliers (e < {bands.thresh} - {q.gamma:.2e}), more than the mask's {total}; "
                                   f"point {int(bands.valid[miss[0]])} (e = {q.e[miss[0]]:.6f}) is one the mask lacks")
    # (c)
    mk = mask[bands.valid] == 1
    found, nearest, prefix_L, blocked = None, None, 0, None
    for q in bands.hyp:
        if q is None:
            continue
        viol = (q.L & ~mk) | (mk & ~q.U)
        nv = int(viol.sum())
        if nv == 0:
            if prefix_L < total:
                found = q
                break
            blocked = blocked or (q, prefix_h)
        elif nearest is None or nv < nearest[1]:
            nearest = (q, nv, int(np.nonzero(viol)[0][0]))
        if q.nL > prefix_L:
            prefix_L, prefix_h = q.nL, q.h
    if found is None:
        if blocked is not None:
            q, first = blocked
            k = int(np.nonzero(bands.hyp[first].L)[0][0])
            raise RansacCheckError(f"{who}: the mask is that of hypothesis {q.h}, but the earlier hypothesis {first} has {bands.hyp[first].nL} definite inliers "
                                   f"(e.g. point {int(bands.valid[k])}), no fewer than the mask's {total}: the first best must win")
        q, nv, k = nearest
        side = "definitely inside" if q.L[k] else "definitely outside"
        raise RansacCheckError(f"{who}: the mask fits no hypothesis; nearest is hypothesis {q.h} with {nv} violations, first at point {int(bands.valid[k])}: "
                               f"e = {q.e[k]:.6f} is {side} {bands.thresh} +- {q.gamma:.2e} and the mask says {int(mk[k])}")
    undecided = int((found.U & ~found.L).sum())
    if undecided > UNDECIDED_CAP * bands.n:
        k = int(np.nonzero(found.U & ~found.L)[0][0])
        raise BadCase(f"{who}: hypothesis {found.h} leaves {undecided} of {bands.n} matched points undecided (first: point {int(bands.valid[k])}): "
                      f"more than {UNDECIDED_CAP:.0%}, the case is badly chosen")
    # (d)
    want = fit_similarity(bands.src[mk], bands.dst[mk])
    bad = np.abs(M - want) > RANSAC_ATOL + RANSAC_RTOL * np.abs(want)
    if bad.any():
        r, c = (int(v) for v in np.argwhere(bad)[0])
        raise RansacCheckError(f"{who}: M[{r},{c}] = {M[r, c]:.7f} is not the least-squares fit {want[r, c]:.7f} over the mask's {total} rows "
                               f"(hypothesis {found.h}, last of them point {int(bands.valid[np.nonzero(mk)[0][-1]])}); |diff| max {np.abs(M - want).max():.2e}")
    second = max((q.nL for q in live if q.h != found.h), default=0)
    return {"h": found.h, "undecided": undecided, "second": second, "n": bands.n}


def fp32_band_usage(bands):
    """Largest |e_fp32 - e_f64| / gamma_h over all hypotheses and points, e_fp32 from the unfused fp32 expressions of
    oracle/ransac_ref.py (model and residual; the length by a float64 square root of the fp32 sum of squares)."""
    f = np.float32
    s, d = bands.src.astype(f), bands.dst.astype(f)
    worst = 0.0
    for q in bands.live:
        i, j = q.i, q.j
        px, py = s[j, 0] - s[i, 0], s[j, 1] - s[i, 1]
        qx, qy = d[j, 0] - d[i, 0], d[j, 1] - d[i, 1]
        den = px * px + py * py
        ca, cb = (qx * px + qy * py) / den, (qy * px - qx * py) / den
        tx = d[i, 0] - (ca * s[i, 0] - cb * s[i, 1])
        ty = d[i, 1] - (cb * s[i, 0] + ca * s[i, 1])
        ex = ca * s[:, 0] - cb * s[:, 1] + tx - d[:, 0]
        ey = cb * s[:, 0] + ca * s[:, 1] + ty - d[:, 1]
        e2 = ex * ex + ey * ey
        assert e2.dtype == f
        err = float(np.abs(np.sqrt(e2.astype(np.float64)) - q.e).max())
        if q.exact:                   # no band: the fp32 evaluation must be the float64 one
            assert err < 1e-12, f"hypothesis {q.h} is exact by _all_exact, its fp32 residuals differ by {err:.2e}"
        else:
            worst = max(worst, err / q.gamma)
    return worst


# ---------------------------------------------------------------------------------------------- cases
def graded_case(seed, K, theta, scale, t, sigma=3.0, unmatched=3, out_every=5, out_max=40.0):
    """Residuals spread continuously across any threshold: Gaussian noise of `sigma` px on every correspondence, every
    `out_every`-th one displaced further by a uniform 0..`out_max` px in a random direction; every `unmatched`-th row unmatched.
    Returns (kpts0 (K,2) f32, kpts1 (K,2) f32, matches0 (K,) int64, the true (2,3) transform)."""
    rng = np.random.RandomState(seed)
    k0 = (rng.rand(K, 2) * 600).astype(np.float32)
    R = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]]) * scale
    perm = rng.permutation(K)
    pts = k0 @ R.T + np.asarray(t, float) + rng.randn(K, 2) * sigma
    far = np.arange(1, K, out_every)
    r, phi = rng.rand(len(far)) * out_max, rng.rand(len(far)) * 2 * np.pi
    pts[far] += np.stack([r * np.cos(phi), r * np.sin(phi)], 1)
    k1 = np.zeros((K, 2), np.float32)
    k1[perm] = pts.astype(np.float32)
    m = perm.astype(np.int64).copy()
    m[::unmatched] = -1
    return k0, k1, m, np.concatenate([R, np.asarray(t, float)[:, None]], 1)


LATTICE_MOVES = np.array([(x, y) for x in range(-7, 8) for y in range(-7, 8) if x * x + y * y in (41, 45, 49, 50, 52, 53)], np.int64)
assert len(LATTICE_MOVES) == 48 and int(((LATTICE_MOVES ** 2).sum(1) == 49).sum()) == 4


def lattice_case(seed, K, kind):
    """Integer kpts0 in [0, 500); kpts1 an exact similarity of it -- kind "trans": k0 + (13, -40); kind "rot2": (-2y + 30, 2x - 11),
    i.e. ca = 0, cb = 2 -- with every fifth correspondence moved by one of the 48 integer vectors of squared length 41, 45, 49, 50,
    52 or 53 (four of them exactly on the 7-px circle) and every fourth row unmatched.  On a clean hypothesis (both sampled points
    unmoved) every product, quotient and sum of the kernel is an exact small integer in fp32: contraction cannot change a bit, and
    e^2 < 49 is decided exactly, e^2 == 49 included.  Returns (kpts0, kpts1, matches0, M true, moved (K,) bool)."""
    if kind not in ("trans", "rot2"):
        raise ValueError(kind)
    rng = np.random.RandomState(seed)
    k0 = rng.randint(0, 500, size=(K, 2)).astype(np.int64)
    perm = rng.permutation(K)
    if kind == "trans":
        pts, M = k0 + np.array([13, -40]), np.array([[1., 0., 13.], [0., 1., -40.]])
    else:
        pts, M = np.stack([-2 * k0[:, 1] + 30, 2 * k0[:, 0] - 11], 1), np.array([[0., -2., 30.], [2., 0., -11.]])
    moved = np.zeros(K, bool)
    moved[1::5] = True
    pts = pts.copy()
    pts[moved] += LATTICE_MOVES[rng.randint(0, len(LATTICE_MOVES), size=int(moved.sum()))]
    k1 = np.zeros((K, 2), np.float32)
    k1[perm] = pts.astype(np.float32)
    m = perm.astype(np.int64).copy()
    m[::4] = -1
    return k0.astype(np.float32), k1, m, M, moved


def lattice_expected_mask(case, counts0=None):
    """The inlier mask of the true transform with e^2 < 49 evaluated in integers (exact; points on the circle are out)."""
    k0, k1, m, M, _ = case
    K = len(m)
    ok = m >= 0
    if counts0 is not None:
        ok &= np.arange(K) < int(counts0)
    a = k0.astype(np.int64)
    Mi = np.rint(M).astype(np.int64)
    assert (Mi == M).all()
    proj = a @ Mi[:, :2].T + Mi[:, 2]
    r = proj - k1[np.where(ok, m, 0)].astype(np.int64)
    return (ok & ((r * r).sum(1) < 49)).astype(np.uint8)


def lattice_premise(case, bands):
    """The premise of a lattice case, from the data alone: there is a clean hypothesis, and the smallest |L| of a clean hypothesis
    exceeds the largest |U| of any other -- so every correct evaluation lets a clean hypothesis win, with the exact mask.
    Returns (holds, text)."""
    moved = case[4][bands.valid]
    clean = [q for q in bands.live if not (moved[q.i] or moved[q.j])]
    other = [q for q in bands.live if moved[q.i] or moved[q.j]]
    if not clean:
        return False, "no clean hypothesis"
    lo, hi = min(q.nL for q in clean), max((q.nU for q in other), default=0)
    return lo > hi, f"{len(clean)} clean hypotheses with |L| >= {lo}, {len(other)} others with |U| <= {hi}"


# ---------------------------------------------------------------------------------------------- 2-NN
def knn2_ref(a, b):
    """Float64 brute force: a (N0,d), b (N1,d), N1 >= 2 -> (nn1, nn2, d1sq, d2sq), the two nearest rows of b for every row of a by
    the sum of squared differences (no |a|^2 + |b|^2 - 2ab cancellation), lowest index first among equal distances."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    D = np.empty((len(a), len(b)))
    for i in range(len(a)):
        D[i] = ((b - a[i]) ** 2).sum(1)
    order = np.argsort(D, axis=1, kind="stable")
    nn1, nn2 = order[:, 0], order[:, 1]
    rows = np.arange(len(a))
    return nn1, nn2, D[rows, nn1], D[rows, nn2]


def knn_sq_bar(a, b, nn):
    """(d + 4) * 2^-24 * (|a_i|^2 + |b_nn(i)|^2): the a-priori bound of an fp32 evaluation of |a|^2 + |b|^2 - 2ab in any summation
    order (d products and d - 1 sums per term, the three terms' sums, the clamp), per query row.  Derived, not measured."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a.shape[1] + 4) * U24 * ((a * a).sum(1) + (b[nn] * b[nn]).sum(1))


def knn_decided(d1sq, d2sq, bar1, bar2, ratio):
    """The ratio decision dist1 < ratio * dist2 in float64, and where it survives moving both squared distances by their bars
    (each way): (accept (N0,) bool, decided (N0,) bool).  Only decided rows bind an fp32 evaluation."""
    lo = lambda x, bar: np.sqrt(np.maximum(x - bar, 0.0))
    hi = lambda x, bar: np.sqrt(x + bar)
    accept = np.sqrt(d1sq) < ratio * np.sqrt(d2sq)
    sure_yes = hi(d1sq, bar1) < ratio * lo(d2sq, bar2)
    sure_no = lo(d1sq, bar1) >= ratio * hi(d2sq, bar2)
    return accept, np.where(accept, sure_yes, sure_no)


# ---------------------------------------------------------------------------------------------- the suite's cases
class Batch:
    """One call of estimate_affine_partial: B cases of equal K, the call's parameters, optional counts0 (one per pair)."""

    def __init__(self, name, cases, thresh, hypotheses, seed, counts0=None, lattice=False):
        self.name, self.cases, self.thresh, self.hypotheses, self.seed, self.counts0, self.lattice = name, cases, thresh, hypotheses, seed, counts0, lattice

    def bands(self, b):
        c = self.cases[b]
        return hypothesis_bands(c[0], c[1], c[2], b, self.thresh, self.hypotheses, self.seed, None if self.counts0 is None else self.counts0[b])

    def oracle(self, b):
        c = self.cases[b]
        m = c[2] if self.counts0 is None else np.where(np.arange(len(c[2])) < self.counts0[b], c[2], -1)
        return ransac_ref.estimate_affine_partial(c[0], c[1], m, b=b, thresh=self.thresh, hypotheses=self.hypotheses, seed=self.seed)


def _g300():
    return graded_case(13, 300, 1.0, 2.0, (300, 10))


def graded_batches():
    """Graded cases: the three single pairs, B = 3 with a transform per pair (the b + 1 term of the hash), counts0 cutting two pairs,
    and K = 6000 (96 KB of dynamic LDS)."""
    return [Batch("g1024", [graded_case(11, 1024, 0.05, 0.95, (12, -7))], 7.0, 256, 5),
            Batch("g700", [graded_case(12, 700, -0.3, 1.2, (-40, 25))], 3.0, 512, 6),
            Batch("g300", [_g300()], 7.0, 100, 7),
            Batch("g512x3", [graded_case(21, 512, 0.4, 0.7, (5, 60)), graded_case(22, 512, -1.2, 1.5, (200, -30)), graded_case(23, 512, 0.0, 1.0, (-9, 9))], 7.0, 128, 8),
            Batch("g600_counts", [graded_case(31, 600, 0.2, 1.1, (3, 4)), graded_case(32, 600, -0.1, 0.9, (-20, 14)), graded_case(33, 600, 0.7, 1.3, (50, 50))],
                  7.0, 128, 9, counts0=[600, 350, 251]),
            Batch("g6000", [graded_case(41, 6000, 0.15, 1.05, (20, -11))], 7.0, 64, 10)]


HYPOTHESIS_COUNTS = (1, 255, 256, 257, 700)       # the hypothesis loop strides by the 256 threads of the workgroup


def hypothesis_count_batches():
    return [Batch(f"g300_h{h}", [_g300()], 7.0, h, 7) for h in HYPOTHESIS_COUNTS]


def lattice_batches():
    """Lattice cases: K = 257 and 400, then the sizes round the two steps of the coordinate staging -- 4096 / 4097 (64 KB of dynamic
    LDS, the default limit, and the first launch above it), 8191 / 8192 (the last LDS sizes, 128 KB) and 8193 (HBM scratch) with two
    pairs, so that the second pair's scratch offset counts.  Data and RANSAC seeds are chosen so that lattice_premise holds."""
    L = lambda name, cases, hyp, seed: Batch(name, cases, 7.0, hyp, seed, lattice=True)
    return [L("l257", [lattice_case(1, 257, "trans")], 32, 2),
            L("l400", [lattice_case(1, 400, "rot2")], 32, 1),
            L("l4096", [lattice_case(1, 4096, "rot2")], 64, 1),
            L("l4097", [lattice_case(1, 4097, "trans")], 64, 3),
            L("l8191", [lattice_case(2, 8191, "rot2")], 64, 1),
            L("l8192", [lattice_case(1, 8192, "trans")], 64, 4),
            L("l8193x2", [lattice_case(3, 8193, "trans"), lattice_case(1, 8193, "rot2")], 64, 1)]


def degenerate_cases():
    """(all_same, some_same): K = 12 rows; in the first every matched kpts0 row is the same point (den = 0 for every hypothesis), in
    the second only the first five are (some hypotheses degenerate; the rest follow an exact translation with one point off)."""
    K = 12
    k0 = np.tile(np.array([[37., 91.]], np.float32), (K, 1))
    k1 = (np.arange(2 * K, dtype=np.float32).reshape(K, 2) * 3 + 5)
    m = np.arange(K, dtype=np.int64)
    m[::4] = -1
    all_same = (k0, k1, m)
    k0b = k0.copy()
    k0b[5:] = np.array([[10, 20], [200, 40], [33, 300], [150, 150], [400, 10], [90, 260], [310, 220]], np.float32)
    k1b = k0b + np.array([13, -40], np.float32)
    k1b[7] += np.array([3, 60], np.float32)
    return all_same, (k0b, k1b, m.copy())


# ---------------------------------------------------------------------------------------------- 2-NN checks and cases
def check_knn_output(a, b, ratio, matches, dist1, dist2, what=""):
    """One pair of knn_ratio_match against the float64 brute force: a (N0,d), b (N1,d) with N1 >= 2, the outputs (N0,).
      * the bar is on the SQUARED distance: |dist^2 - ref^2| <= (d + 4) 2^-24 (|a|^2 + |b|^2) (knn_sq_bar) for both neighbours;
      * the ratio decision is required wherever the float64 decision survives moving both squared distances by their bars
        (knn_decided), and an accepted row must then name the nearest neighbour wherever that is nearest by more than the bars.
    An exact duplicate need NOT come back at distance 0: |a|^2 + |b|^2 - 2ab cancels to within the bar, not to zero (the kernel
    clamps at 0 before the root), so the distance of a duplicate may be anything up to sqrt(bar), about 3e-3 at d = 64.
    Returns (worst fraction of the bar used, number of undecided rows)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    matches, dist1, dist2 = np.asarray(matches), np.asarray(dist1, np.float64), np.asarray(dist2, np.float64)
    nn1, nn2, d1sq, d2sq = knn2_ref(a, b)
    bar1, bar2 = knn_sq_bar(a, b, nn1), knn_sq_bar(a, b, nn2)
    use1, use2 = np.abs(dist1 ** 2 - d1sq) / bar1, np.abs(dist2 ** 2 - d2sq) / bar2
    worst = float(max(use1.max(), use2.max()))
    i = int(np.argmax(np.maximum(use1, use2)))
    assert worst <= 1.0, (f"{what}: row {i}: squared distances {dist1[i] ** 2:.9e} / {dist2[i] ** 2:.9e} against {d1sq[i]:.9e} / {d2sq[i]:.9e}: "
                          f"{worst:.2f} of the bar {bar1[i]:.3e}")
    accept, decided = knn_decided(d1sq, d2sq, bar1, bar2, ratio)
    got_accept = matches >= 0
    bad = np.nonzero(decided & (got_accept != accept))[0]
    assert not len(bad), f"{what}: row {int(bad[0])}: ratio decision {bool(got_accept[bad[0]])}, float64 says {bool(accept[bad[0]])} beyond the bars ({len(bad)} rows)"
    clear = d2sq - d1sq > bar1 + bar2
    bad = np.nonzero(got_accept & clear & (matches != nn1))[0]
    assert not len(bad), f"{what}: row {int(bad[0])}: matched to {int(matches[bad[0]])}, the nearest is {int(nn1[bad[0]])} ({len(bad)} rows)"
    bad = np.nonzero(got_accept & ((matches >= len(b)) | ((matches != nn1) & (matches != nn2))))[0]
    assert not len(bad), f"{what}: row {int(bad[0])}: matched to {int(matches[bad[0]])}, neither of the two nearest ({int(nn1[bad[0]])}, {int(nn2[bad[0]])})"
    return worst, int((~decided).sum())


def knn_fp32_restatement(a, b, ratio):
    """An fp32 evaluation of the kernel's expression on the host (numpy sums, another order than the device's): (matches, d1, d2)."""
    f = np.float32
    a, b = np.asarray(a, f), np.asarray(b, f)
    k = (b * b).sum(1, dtype=f)[None] - f(2) * (a @ b.T)
    order = np.argsort(k, axis=1, kind="stable")
    rows = np.arange(len(a))
    na = (a * a).sum(1, dtype=f)
    d1 = np.sqrt(np.maximum(na + k[rows, order[:, 0]], f(0)))
    d2 = np.sqrt(np.maximum(na + k[rows, order[:, 1]], f(0)))
    return np.where(d1 < f(ratio) * d2, order[:, 0], -1), d1, d2


def _unit(x):
    x = np.asarray(x, np.float32)
    return (x / np.sqrt((x * x).sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)


NEAR_DUPLICATE_S = (0.0, 1e-6, 1e-4, 1e-2)


def near_duplicate_case(d, s, N=150, seed=0):
    """desc0 (N,d) unit rows, desc1 = normalize(desc0 + s * noise): the nearest neighbour of row i is row i at distance about
    s sqrt(d), where |a|^2 + |b|^2 - 2ab cancels."""
    rng = np.random.RandomState(1000 * d + seed)
    a = _unit(rng.randn(N, d))
    return a, _unit(a + np.float32(s) * rng.randn(N, d).astype(np.float32))


# tied columns of desc1: the copies of column j sit 64 further (the same lane of the wave: the in-lane rule of the scan), 1 and 37
# further (other lanes: the cross-lane merge), for j in the first 64-block and with the copy in the last, partial one; two triples
TIE_N1 = 233
TIE_GROUPS = ((3, 67), (10, 11), (20, 57), (150, 214), (200, 201), (193, 230), (40, 77, 104), (133, 170, 197), (232 - 64, 232))


def tie_case(d=64, seed=0):
    """(desc0 (len(TIE_GROUPS),d), desc1 (TIE_N1,d)): the columns of every group of TIE_GROUPS are bit-equal, query g is a noisy copy
    of group g's column, every other column a random unit vector (at distance about 1.4)."""
    rng = np.random.RandomState(77 + seed)
    b = _unit(rng.randn(TIE_N1, d))
    for grp in TIE_GROUPS:
        b[list(grp[1:])] = b[grp[0]]
    a = _unit(b[[grp[0] for grp in TIE_GROUPS]] + np.float32(0.05) * rng.randn(len(TIE_GROUPS), d).astype(np.float32))
    return a, b


def planted_case(N0, N1, d, seed):
    """Random unit rows on both sides; every third query (as far as side 1 reaches) has a noisy copy planted at its own index, so
    that the ratio test accepts some rows."""
    rng = np.random.RandomState(31 * N0 + 7 * N1 + d + seed)
    a, b = _unit(rng.randn(N0, d)), _unit(rng.randn(N1, d))
    k = min(N0, N1)
    b[:k:3] = _unit(a[:k:3] + np.float32(0.05) * rng.randn(*a[:k:3].shape).astype(np.float32))
    return a, b


EDGE_N1 = (2, 3, 63, 64, 65, 129)      # 64 = one lane stride of the scan
EDGE_N0 = (1, 3, 4, 5)                 # four query rows per workgroup
