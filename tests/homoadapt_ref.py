"""CPU restatement of the homographic-adaptation stages (torch / numpy, float32 or float64) for the tests that cannot
carry the reference to where they run.  Written from the semantics of the reference, cited by line:
  warp / valid mask      utils/utils.py:358-454   (warp_points, inv_warp_image_batch, compute_valid_mask)
  heatmap from semi      utils/utils.py:491-505, utils/d2s.py:8-25   (flattenDetection)
  combine                utils/utils.py:507-518   (combine_heatmap)
  points                 utils/utils.py:250-332   (getPtsFromHeatmap, nms_fast)
  sub-pixel              superpoint/models/model_wrap.py:146-176, utils/losses.py:48-83,111-129
tests/test_homoadapt_host.py pins it to fixtures the reference itself wrote (tests/golden/make_golden_homoadapt.py)."""
import numpy as np
import torch
import torch.nn.functional as F

BORDER = 4


def source_grid(mats, H, W, dtype=torch.float32):
    """(N,H,W,2) normalised source coordinates: M_b applied to (linspace(-1,1,W)[x], linspace(-1,1,H)[y], 1), divided by
    the third component.  float32: the reference's arithmetic; float64: the same formula in double."""
    mats = torch.as_tensor(np.asarray(mats)).to(dtype)
    xs, ys = torch.linspace(-1, 1, W, dtype=dtype), torch.linspace(-1, 1, H, dtype=dtype)
    pts = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W), torch.ones(H, W, dtype=dtype)], -1).reshape(-1, 3)
    N = mats.shape[0]
    w = (mats.reshape(N * 3, 3) @ pts.t()).reshape(N, 3, -1).transpose(2, 1)
    return (w[:, :, :2] / w[:, :, 2:]).reshape(N, H, W, 2)


def warp(img, mats, mode="bilinear", dtype=torch.float32):
    """img (N,H,W), or (H,W) shared by all matrices -> (N,H,W)."""
    img = torch.as_tensor(np.asarray(img)).to(dtype)
    N = len(mats)
    if img.dim() == 2:
        img = img[None].expand(N, -1, -1)
    H, W = img.shape[-2:]
    return F.grid_sample(img[:, None], source_grid(mats, H, W, dtype), mode=mode, align_corners=True)[:, 0]


def valid_mask(mats, H, W, dtype=torch.float32):
    return warp(torch.ones(len(mats), H, W), mats, "nearest", dtype)


def source_pixels(mats, H, W, dtype=torch.float64):
    """un-normalised source pixel coordinates (N,H,W,2) (x, y): ((g + 1) / 2) (size - 1)"""
    g = source_grid(mats, H, W, dtype)
    return torch.stack([(g[..., 0] + 1) / 2 * (W - 1), (g[..., 1] + 1) / 2 * (H - 1)], -1)


def flatten_detection(semi):
    """semi (N,65,Hc,Wc) -> heatmaps (N,8Hc,8Wc): softmax over the 65 channels, dustbin dropped, channel dy*8+dx -> (dy, dx)."""
    semi = torch.as_tensor(np.asarray(semi)) if not isinstance(semi, torch.Tensor) else semi
    return F.pixel_shuffle(torch.softmax(semi, 1)[:, :-1], 8)[:, 0]


def combine(heat, mask, unwarp, dtype=torch.float32):
    """-> (combined (H,W), count (H,W)); 0 / 0 = NaN where no map covers a pixel."""
    heat = torch.as_tensor(np.asarray(heat)).to(dtype)
    mask = torch.as_tensor(np.asarray(mask)).to(dtype)
    num = warp(heat * mask, unwarp, "bilinear", dtype).sum(0)
    den = warp(mask, unwarp, "bilinear", dtype).sum(0)
    return num / den, den


def points(heatmap, conf_thresh, nms_dist, border=BORDER):
    """(3,K) float64 rows x, y, conf by descending conf.  Greedy NMS in descending score, equal scores by the lower
    row-major index first (the reference's argsort leaves that order open); border removed after the NMS."""
    h = np.asarray(heatmap)
    H, W = h.shape
    ys, xs = np.where(h >= conf_thresh)
    if len(ys) == 0:
        return np.zeros((3, 0))
    sc = h[ys, xs].astype(np.float64)
    order = np.lexsort((ys * W + xs, -sc))
    taken = np.zeros((H + 2 * nms_dist, W + 2 * nms_dist), bool)      # True: inside the window of a kept point
    keep = []
    for i in order:
        y, x = ys[i], xs[i]
        if taken[y + nms_dist, x + nms_dist]:
            continue
        taken[y:y + 2 * nms_dist + 1, x:x + 2 * nms_dist + 1] = True
        keep.append(i)
    keep = np.asarray(keep, int)
    x, y, s = xs[keep], ys[keep], sc[keep]
    ok = ~((x < border) | (x >= W - border) | (y < border) | (y >= H - border))
    return np.stack([x[ok].astype(np.float64), y[ok].astype(np.float64), s[ok]])


def subpixel(heatmap, pts, patch=5):
    """pts (3,K) -> (3,K) float64: x, y moved to the centroid of the patch x patch window of the zero-padded map
    (softmax(log(p / (sum p + 1e-6))) = p / sum p), minus patch // 2."""
    h = np.pad(np.asarray(heatmap, np.float64), patch // 2)
    out = np.array(pts, np.float64, copy=True)
    ax = np.arange(patch, dtype=np.float64)
    for k in range(out.shape[1]):
        x, y = int(out[0, k]), int(out[1, k])
        p = h[y:y + patch, x:x + patch]
        out[0, k] += (p * ax[None, :]).sum() / p.sum() - patch // 2
        out[1, k] += (p * ax[:, None]).sum() / p.sum() - patch // 2
    return out


def rows_equal_up_to_ties(a, b):
    """Two (K,3) point lists are the same list, where rows of equal score may come in any order."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    if not np.array_equal(a[:, 2], b[:, 2]):
        return False
    key = lambda r: sorted(map(tuple, r))
    for s in np.unique(a[:, 2]):
        if key(a[a[:, 2] == s]) != key(b[b[:, 2] == s]):
            return False
    return True
