"""The three stages of a SuperGlue training sample restated in numpy / float64, for the parity tests of
imx_warp_perspective_u8, imx_gt_matches and imx_match_loss (include/imx.h).  The project's own text: every function names the
reference lines (datasets/GlueSparse.py, superglue/models/superglue_train.py) or the published OpenCV algorithm it restates.
tests/golden/make_golden_trainpairs.py hands the OpenCV restatements to the reference as its `cv2`; the fixtures it writes are the
reference's own outputs, and tests/test_trainpairs_host.py holds this file against them."""
import numpy as np

RADIUS = 3.0          # GlueSparse.py:71


# ---------------------------------------------------------------------------------------------- OpenCV stand-ins
def four_point_matrix(src, dst):
    """cv2.getPerspectiveTransform (GlueSparse.py:31): the 3x3 matrix taking four points onto four points, m8 = 1; the 8x8 system
    solved in float64 (OpenCV's own solver is unpinned)."""
    A, b = np.zeros((8, 8)), np.zeros(8)
    for k, ((x, y), (u, v)) in enumerate(zip(np.asarray(src, np.float64), np.asarray(dst, np.float64))):
        A[k] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[k + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[k], b[k + 4] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def invert3(M):
    """the double-precision inversion cv2.warpPerspective applies to a forward matrix (the caller's job in imx_warp_perspective_u8)"""
    return np.linalg.inv(np.asarray(M, np.float64).reshape(3, 3))


def _sat_int(v):
    return np.rint(np.clip(v, -2147483648.0, 2147483647.0)).astype(np.int64)


def warp_coords(minv, H, W):
    """Fixed-point source coordinates of every destination pixel (5 fractional bits), and the unrounded 32 x coordinate they were
    rounded from: w = m6 x + m7 y + m8, s = w ? 32 / w : 0, X = sat_int(rint((m0 x + m1 y + m2) s))."""
    m = np.asarray(minv, np.float64).reshape(9)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    w = m[6] * x + m[7] * y + m[8]
    with np.errstate(divide="ignore"):
        s = np.where(w != 0, 32.0 / w, 0.0)
    fX, fY = (m[0] * x + m[1] * y + m[2]) * s, (m[3] * x + m[4] * y + m[5]) * s
    return _sat_int(fX), _sat_int(fY), fX, fY


def _taps(img, X, Y):
    H, W = img.shape
    ix, iy = X >> 5, Y >> 5
    out = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = ix + dx, iy + dy
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        t = np.zeros(X.shape, np.int64)
        t[ok] = img[yy[ok], xx[ok]]
        out.append(t)
    return out


def warp_perspective_u8(img, minv):
    """cv2.warpPerspective(img, M, (W, H)) for a uint8 image (GlueSparse.py:32), INTER_LINEAR, constant border 0, given inv(M):
    four taps (0 outside the image) with the integer weights (32 - a)(32 - b) 32, ... of 15 fractional bits, rounded shift."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    X, Y, _, _ = warp_coords(minv, H, W)
    a, b = X & 31, Y & 31
    t00, t01, t10, t11 = _taps(img, X, Y)
    acc = t00 * ((32 - b) * (32 - a) * 32) + t01 * ((32 - b) * a * 32) + t10 * (b * (32 - a) * 32) + t11 * (b * a * 32)
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def warp_bilinear_f64(img, minv):
    """the exact float64 bilinear value at the SAME fixed-point coordinates (unrounded): what the integer form may be one grey level from"""
    img = np.asarray(img, np.uint8)
    X, Y, _, _ = warp_coords(minv, *img.shape)
    a, b = (X & 31) / 32.0, (Y & 31) / 32.0
    t00, t01, t10, t11 = _taps(img, X, Y)
    return t00 * (1 - b) * (1 - a) + t01 * (1 - b) * a + t10 * b * (1 - a) + t11 * b * a


def warp_boundary_pixels(minv, H, W, eps=1e-6):
    """(y, x) of the pixels whose 32 x coordinate lies within eps of a rounding boundary (k + 1/2): the only ones where two correct
    evaluations of the coordinate may round apart"""
    _, _, fX, fY = warp_coords(minv, H, W)
    near = lambda f: np.abs(np.abs(f - np.floor(f)) - 0.5) < eps
    return np.argwhere(near(fX) | near(fY)).astype(np.int32)


def project(kpts, M):
    """cv2.perspectiveTransform(kpts[None], M)[0] for float32 points and a double matrix (GlueSparse.py:64): homogeneous product in
    double, w = 1 / w where |w| exceeds double epsilon (else 0), rounded to float32."""
    k = np.asarray(kpts, np.float32).reshape(-1, 2).astype(np.float64)
    m = np.asarray(M, np.float64).reshape(9)
    x, y = k[:, 0], k[:, 1]
    w = x * m[6] + y * m[7] + m[8]
    with np.errstate(divide="ignore"):
        w = np.where(np.abs(w) > np.finfo(np.float64).eps, 1.0 / w, 0.0)
    return np.stack([(x * m[0] + y * m[1] + m[2]) * w, (x * m[3] + y * m[4] + m[5]) * w], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------- GlueSparse.py:64-82
def distances(proj, kpts1):
    """cdist(proj, kpts1) (:65): sqrt(dx dx + dy dy) in double from float32 points"""
    p, q = np.asarray(proj, np.float32).astype(np.float64), np.asarray(kpts1, np.float32).astype(np.float64)
    dx, dy = p[:, None, 0] - q[None, :, 0], p[:, None, 1] - q[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def gt_matches(proj, kpts1, radius=RADIUS):
    """The ground-truth assignment of :67-82 from the projected keypoints of side 0 and the keypoints of side 1.

    The reference takes min1[j] (nearest i of column j), min2[i] (nearest j of row i), the set min1f of the j that are nearest to
    some row whose smallest distance is below the radius, the set xx of the j with min2[min1[j]] == j, and intersects them (:70-74).
    That set is {j : i = min1[j], min2[i] == j, D[i, j] < radius}: for j in xx the pair (i, j) is mutual, so D[i, j] is both row
    i's minimum and column j's; if some row i' with min2[i'] == j has its minimum D[i', j] below the radius then D[i, j] <=
    D[i', j] is below it too, and the converse holds with i' = i.  So: a pair is a match when each point is the other's nearest
    (numpy's argmin: the lowest index among equal distances) and their distance is below the radius.

    Returns dict(gt0 (n0), gt1 (n1), matches (2, n) rows (i, j) ascending in j, all_matches (2, n0 + n1 - n): the matches, then
    every unmatched i ascending against column n1, then every unmatched j ascending against row n0)."""
    D = distances(proj, kpts1)
    n0, n1 = D.shape
    gt0, gt1 = np.full(n0, -1, np.int64), np.full(n1, -1, np.int64)
    if n0 and n1:
        near_i, near_j = D.argmin(0), D.argmin(1)          # per column / per row
        for j in range(n1):
            i = near_i[j]
            if near_j[i] == j and D[i, j] < radius:
                gt0[i], gt1[j] = j, i
    js = np.nonzero(gt1 >= 0)[0]
    un0, un1 = np.nonzero(gt0 < 0)[0], np.nonzero(gt1 < 0)[0]
    matches = np.stack([gt1[js], js]).astype(np.int64)
    cols = [matches, np.stack([un0, np.full(len(un0), n1)]), np.stack([np.full(len(un1), n0), un1])]
    return {"gt0": gt0, "gt1": gt1, "matches": matches, "all_matches": np.concatenate(cols, 1).astype(np.int64), "dists": D}


def margins(D, radius=RADIUS):
    """How far the decisions of gt_matches are from flipping: the gap between the smallest and second smallest distance of every row
    and of every column (inf for a line of one entry), and |row minimum - radius|."""
    def gap(A):
        if A.shape[1] < 2:
            return np.full(A.shape[0], np.inf)
        s = np.sort(A, 1)
        return s[:, 1] - s[:, 0]
    return {"row_gap": gap(D), "col_gap": gap(D.T), "radius_gap": np.abs(D.min(1) - radius)}


# ---------------------------------------------------------------------------------------------- superglue_train.py:289-299
def match_loss(Z, all_matches, dtype=np.float32):
    """mean over the columns (x, y) of -log(exp(Z[x][y])) (:289-298) in `dtype`; Z is log_optimal_transport's (n0+1, n1+1) output"""
    am = np.asarray(all_matches, np.int64)
    if am.shape[1] == 0:
        return dtype(0)
    z = np.asarray(Z)[am[0], am[1]].astype(dtype)
    with np.errstate(divide="ignore"):
        return (-np.log(np.exp(z))).astype(dtype).mean(dtype=dtype)


def match_stats(matches0, gt0):
    """[ground-truth matches, predicted matches, correct ones]: what precision and recall of a validation pass are made of"""
    m, g = np.asarray(matches0, np.int64), np.asarray(gt0, np.int64)
    return np.array([(g >= 0).sum(), (m > -1).sum(), ((m == g) & (g >= 0)).sum()], np.int32)
