"""A restatement, in text of our own, of the four stages of SuperPoint descriptor training that libimx serves
(csrc/sptrain.hip): numpy / torch on the CPU, every step with the line of the reference it restates.  It is held to the
fixtures the reference wrote (tests/golden/make_golden_sptrain.py) by tests/test_sptrain_host.py, and the kernels are held to
it and to those fixtures by tests/test_gpu_sptrain.py.

The erosion follows OpenCV's PUBLISHED algorithm (getStructuringElement(MORPH_ELLIPSE), erode): OpenCV is on no machine of
this project, so parity with cv2 itself is unpinned and the kernel is held to this restatement."""
import numpy as np
import torch

F32 = np.float32
WARPED_PAIR_PARAMS = dict(translation=True, rotation=True, scaling=True, perspective=True, scaling_amplitude=0.2, perspective_amplitude_x=0.2,
                          perspective_amplitude_y=0.2, patch_ratio=0.85, max_angle=1.57, allow_artifacts=True)   # the shipped yaml's warped_pair.params


# ---------------------------------------------------------------------------------------------- matrices
def _conjugate(Hn, width, height):
    """inverse(trans) @ H @ trans in fp32, the reference's torch expression"""
    trans = torch.tensor([[2. / width, 0., -1.], [0., 2. / height, -1.], [0., 0., 1.]], dtype=torch.float32)
    Hn = torch.as_tensor(np.asarray(Hn, F32)).reshape(-1, 3, 3)
    return torch.stack([torch.inverse(trans) @ m @ trans for m in Hn]).numpy()      # one 2-D product chain per matrix, as the reference


def scale_pixels(Hn, H, W):
    """homography_scaling_torch (utils/utils.py:586-589): [-1,1]^2 matrices -> pixel coordinates"""
    return _conjugate(Hn, float(W), float(H))


def scale_cells(Hn, Hc, Wc):
    """scale_homography_torch(H, (Hc, Wc), shift=(-1,-1)) (utils/homographies.py:121-125)"""
    return _conjugate(Hn, float(Wc), float(Hc))


def _fma(a, b, c):
    """round32(a b + c): the product of two fp32 values is exact in float64"""
    return (np.float64(a) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def warp_points(m, x, y):
    """warp_points (utils/utils.py:561-584) in fp32, its matrix product H @ (x, y, 1) as torch's CPU product evaluates it where the
    processor has fused multiply-add: k ascending, the first product rounded, every later term fused into the running sum; then
    the division.  The fixtures' warped points agree with this bit for bit."""
    m = np.asarray(m, F32).reshape(9)
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    with np.errstate(all="ignore"):
        u, v, w = (_fma(m[r + 2], F32(1), _fma(m[r + 1], y, (m[r] * x).astype(F32))) for r in (0, 3, 6))
        return (u / w).astype(F32), (v / w).astype(F32)


# ---------------------------------------------------------------------------------------------- labels
def points_to_2d(pts, H, W):
    """ALLSS.points_to_2D (datasets/ALLSS.py:129-133): truncation, no warp, no filter.  Returns (labels, flag): a point outside the
    image is written nowhere and raises the flag (the reference would index out of bounds)."""
    labels, flag = np.zeros((H, W), F32), 0
    p = np.trunc(np.asarray(pts, F32).reshape(-1, 2))
    for x, y in p:
        if 0 <= x <= W - 1 and 0 <= y <= H - 1:
            labels[int(y), int(x)] = 1
        else:
            flag = 1
    return labels, flag


def warp_labels(pts, mat_px, H, W):
    """warpLabels (datasets/data_tools.py:36-54) with the residual in ALLSS's (2,H,W) layout (datasets/ALLSS.py:226): .long(),
    warp_points, filter_points on the unrounded point, round() half to even.  Two points on one pixel: the HIGHER index writes
    the residual (the documented rule of imx_warp_labels).  Returns (labels, res, warped points kept (n,2))."""
    labels, res = np.zeros((H, W), F32), np.zeros((2, H, W), F32)
    p = np.trunc(np.asarray(pts, F32).reshape(-1, 2))
    wx, wy = warp_points(mat_px, p[:, 0], p[:, 1])
    keep = (wx >= 0) & (wx <= W - 1) & (wy >= 0) & (wy <= H - 1)
    wx, wy = wx[keep], wy[keep]
    rx, ry = np.rint(wx), np.rint(wy)
    for i in range(len(wx)):                                           # ascending: the last writer is the highest index
        labels[int(ry[i]), int(rx[i])] = 1
        res[0, int(ry[i]), int(rx[i])] = wx[i] - rx[i]
        res[1, int(ry[i]), int(rx[i])] = wy[i] - ry[i]
    return labels, res, np.stack([wx, wy], 1)


# ---------------------------------------------------------------------------------------------- erosion
def ellipse(r):
    """cv2.getStructuringElement(MORPH_ELLIPSE, (2r, 2r)) as OpenCV publishes it: row i has dy = i - r and, where |dy| <= r,
    dx = (int)rint(r sqrt((r^2 - dy^2) / r^2)) in double and ones in columns [max(r - dx, 0), min(r + dx + 1, 2r))"""
    k = np.zeros((2 * r, 2 * r), np.uint8)
    for i in range(2 * r):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(r * np.sqrt((r * r - dy * dy) / float(r * r))))
            k[i, max(r - dx, 0):min(r + dx + 1, 2 * r)] = 1
    return k


def erode(mask, r):
    """cv2.erode(mask, ellipse(r)), anchor (r, r), one iteration: out(y,x) = min over the set (i,j) of in(y+i-r, x+j-r), pixels
    outside the image taking no part (the margin of compute_valid_mask, utils/utils.py:449-452)"""
    mask = np.asarray(mask, F32)
    if r == 0:
        return mask.copy()
    H, W = mask.shape[-2:]
    pad = np.full(mask.shape[:-2] + (H + 2 * r, W + 2 * r), np.inf, F32)
    pad[..., r:r + H, r:r + W] = mask
    out = np.full(mask.shape, np.inf, F32)
    for i, j in np.argwhere(ellipse(r)):
        out = np.minimum(out, pad[..., i:i + H, j:j + W])
    return out


# ---------------------------------------------------------------------------------------------- detector loss
def cell_targets(labels, dtype=torch.float64):
    """labels2Dto3D(add_dustbin=True) (utils/utils.py:456-468): (B,H,W) -> (B,65,Hc,Wc); c = dy 8 + dx (SpaceToDepth)"""
    lab = torch.as_tensor(np.asarray(labels)).to(dtype)
    B, H, W = lab.shape
    t = lab.reshape(B, H // 8, 8, W // 8, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, H // 8, W // 8)
    dust = 1 - t.sum(1)
    dust[dust < 1.] = 0
    t = torch.cat([t, dust[:, None]], 1)
    return t / t.sum(1, keepdim=True)


def cell_masks(mask, dtype=torch.float64):
    """getMasks (Train_model_frontend.py:362-377): the product of the 64 mask values of a cell"""
    m = torch.as_tensor(np.asarray(mask)).to(dtype)
    B, H, W = m.shape
    return m.reshape(B, H // 8, 8, W // 8, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, H // 8, W // 8).prod(1)


def detector_loss(semi, labels, mask, dtype=torch.float64, conditioned=True):
    """detector_loss(loss_type='softmax') (Train_model_heatmap.py:72-81) -> (loss, sum of cell masks).
    conditioned=False: as written, softmax then BCELoss with its clamps at -100, in `dtype`.
    conditioned=True: the same value evaluated well: -log p_c = min(100, lse - x_c) and 1 - p_c from the sum of the OTHER
    exponentials.  The two agree (in float64) while no probability rounds to 1 or underflows: logit gaps below ~36; beyond, the
    written form leaves the exact value -- in float64 too -- and the conditioned one is the arithmetic rule of imx_detector_loss."""
    x = torch.as_tensor(np.asarray(semi)).to(dtype)
    t, m = cell_targets(labels, dtype), cell_masks(mask, dtype)
    if conditioned:
        mx = x.max(1, keepdim=True).values
        e = torch.exp(x - mx)
        S = e.sum(1, keepdim=True)
        nlp = torch.clamp((mx - x) + torch.log(S), max=100)
        others = torch.stack([e[:, [k for k in range(65) if k != c]].sum(1) for c in range(65)], 1)
        nl1p = torch.clamp(torch.log(S) - torch.log(others), min=0, max=100)
    else:
        p = torch.softmax(x, 1)
        nlp, nl1p = -torch.clamp(torch.log(p), min=-100), -torch.clamp(torch.log(1 - p), min=-100)
    cell = (t * nlp + (1 - t) * nl1p).sum(1)
    return float((cell * m).sum() / (m.sum() + 1e-10)), float(m.sum())


# ---------------------------------------------------------------------------------------------- sparse descriptor loss
def desc_pairs(hcell, Hc, Wc):
    """sparse_loss.py:118-124: cells in row-major order as (x, y), warp_points in fp32, round_() half to even, filter_points against
    (Wc, Hc).  Returns the surviving flat cell indices (a, b), in row-major order of a."""
    ys, xs = np.divmod(np.arange(Hc * Wc), Wc)
    wx, wy = warp_points(hcell, xs, ys)
    rx, ry = np.rint(wx), np.rint(wy)
    keep = (rx >= 0) & (rx <= Wc - 1) & (ry >= 0) & (ry <= Hc - 1)
    return np.flatnonzero(keep).astype(np.int32), (ry[keep].astype(np.int64) * Wc + rx[keep].astype(np.int64)).astype(np.int32)


def _sample(desc, cells, Hc, Wc):
    """sampleDescriptors (pixelwise_contrastive_loss.py:160-174): grid_sample(align_corners=True) at normPts(p, (Wc, Hc))"""
    uv = torch.stack([torch.as_tensor(cells % Wc), torch.as_tensor(cells // Wc)], 1).to(desc.dtype)
    g = uv / torch.tensor([Wc, Hc], dtype=desc.dtype) * 2 - 1
    out = torch.nn.functional.grid_sample(desc[None], g[None, :, None], mode="bilinear", align_corners=True)
    return out[0, :, :, 0].t()


def desc_loss(desc_a, desc_b, pair_a, pair_b, choice, nonmatch_b, lamda_d=250., margin=0.2, method="1d", dtype=torch.float64):
    """descriptor_loss_sparse (sparse_loss.py:98-174, dist='cos') for one image, given the draws: desc_{a,b} (d,Hc,Wc), the
    compacted pair list, choice (M) into it, nonmatch_b (M,R) flat cell indices.  Returns (loss, lamda_d match, non_match,
    num_hard_negatives, the (M,R) non-match products)."""
    da, db = torch.as_tensor(np.asarray(desc_a)).to(dtype), torch.as_tensor(np.asarray(desc_b)).to(dtype)
    d, Hc, Wc = da.shape
    ia, ib = np.asarray(pair_a, np.int64)[choice], np.asarray(pair_b, np.int64)[choice]
    fa, fb = da.reshape(d, -1).t(), db.reshape(d, -1).t()
    a1 = fa[ia]
    if method == "2d":
        ma, mb = _sample(da, ia, Hc, Wc), _sample(db, ib, Hc, Wc)
    else:
        ma, mb = a1, fb[ib]
    match = torch.clamp(1 - (ma * mb).sum(-1), min=0).sum() / len(ia)                       # pixelwise_contrastive_loss.py:193-195
    prod = (a1[:, None, :] * fb[torch.as_tensor(np.asarray(nonmatch_b, np.int64))]).sum(-1)  # :220-233, a_m the 1d descriptor
    v = torch.clamp(prod - margin, min=0)
    hard = int((v != 0).sum())
    non = v.sum() / (hard + 1)                                                              # sparse_loss.py:88-96
    return float(lamda_d * match + non), float(lamda_d * match), float(non), hard, prod.numpy()


# ---------------------------------------------------------------------------------------------- workload-size cases
# (tests/test_gpu_sp_workload_paths.py runs them, for imx_warp_labels and -- through tests/sploop_ref.py -- imx_warp_labels_bi;
# tests/test_sp_workload_paths_host.py checks what they promise)
def workload_mats(B):
    """mild pixel-space homographies, one per image: a shrink of about 3 %, a small shear, a shift of a few pixels and a perspective
    term of 1e-5 -- every pixel of an image of up to 900 x 900 stays inside it, and neighbouring integer points now and then round to
    the same pixel"""
    return np.stack([np.array([[0.97 - 0.004 * b, 0.012, 4.25 + b], [-0.009, 0.968 + 0.003 * b, 8.5], [1.5e-5, -1e-5, 1.0]], F32) for b in range(B)])


def warped_pixels(m, x, y):
    """the pixel (px, py) warpLabels writes for the integer points (x, y): warp_points, then round() half to even"""
    wx, wy = warp_points(m, np.asarray(x, F32), np.asarray(y, F32))
    return np.rint(wx).astype(np.int64), np.rint(wy).astype(np.int64)


CLUSTER = ((10, 200, -1), (5, 100))      # the point indices of a case's triple (the last is the image's last point) and of its pair


def workload_points(H, W, counts, row0, seed, avoid=None, low=150):
    """(pts_rows, mats): counts[b] points (x, y) with fractional parts for image b under workload_mats.  Per image: the points
    CLUSTER[0] are the integer points (x, y), (x + 1, y), (x, y + 1) of a place where all three round to ONE pixel of a row >= row0, the
    points CLUSTER[1] are (x, y), (x + 1, y) of another such place; the first `low` of the others have y so large that they land in
    rows >= row0; the rest lie anywhere.  `avoid` (B,H,W) bool: no point lands within two pixels of a pixel set there."""
    rng = np.random.default_rng(seed)
    B = len(counts)
    mats = workload_mats(B)
    near = np.zeros((B, H + 4, W + 4), bool)
    if avoid is not None:
        for dy in range(5):
            for dx in range(5):
                near[:, dy:dy + H, dx:dx + W] |= avoid
    near = near[:, 2:-2, 2:-2]
    ys, xs = (g.reshape(-1) for g in np.mgrid[0:H - 1, 0:W - 1])
    out = []
    for b, n in enumerate(counts):
        m = mats[b]
        (px0, py0), (px1, py1), (px2, py2) = warped_pixels(m, xs, ys), warped_pixels(m, xs + 1, ys), warped_pixels(m, xs, ys + 1)
        assert px0.min() >= 0 and px0.max() < W and py0.min() >= 0 and py0.max() < H
        same_x, same_y = (px0 == px1) & (py0 == py1), (px0 == px2) & (py0 == py2)
        ok = (py0 >= row0 + 8) & ~near[b, py0, px0]
        t = rng.choice(np.flatnonzero(same_x & same_y & ok))
        p = rng.choice(np.flatnonzero(same_x & ~same_y & ok & (np.abs(ys - ys[t]) > 8)))
        pts = np.zeros((n, 2), np.int64)
        i3, i2 = [i % n for i in CLUSTER[0]], list(CLUSTER[1])
        pts[i3] = [(xs[t], ys[t]), (xs[t] + 1, ys[t]), (xs[t], ys[t] + 1)]
        pts[i2] = [(xs[p], ys[p]), (xs[p] + 1, ys[p])]
        taken = {tuple(q) for q in pts[i3 + i2]}
        y_low = int(row0 / 0.95) + 12
        for k, i in enumerate(j for j in range(n) if j not in i3 + i2):
            while True:
                q = (int(rng.integers(0, W)), int(rng.integers(y_low if k < low else 0, H)))
                qx, qy = warped_pixels(m, [q[0]], [q[1]])
                if q not in taken and not near[b, qy[0], qx[0]]:
                    break
            taken.add(q)
            pts[i] = q
        out.append((pts + rng.uniform(0.05, 0.95, (n, 2))).astype(F32))
    return out, mats


def det_case(B, H, W, seed):
    """(semi (B,65,H/8,W/8) of N(0, 3^2) logits, labels (B,H,W) of density 0.01)"""
    rng = np.random.default_rng(seed)
    semi = rng.standard_normal((B, 65, H // 8, W // 8), dtype=F32) * F32(3)
    return semi, (rng.random((B, H, W), dtype=F32) < 0.01).astype(F32)


def last_cells_mask(B, H, W, n):
    """(B,H,W): 1 on the pixels of the last n 8x8 cells in (image, cell row, cell column) order, 0 elsewhere"""
    cm = np.zeros(B * (H // 8) * (W // 8), F32)
    cm[-n:] = 1
    return np.ascontiguousarray(np.broadcast_to(cm.reshape(B, H // 8, 1, W // 8, 1), (B, H // 8, 8, W // 8, 8))).reshape(B, H, W)
