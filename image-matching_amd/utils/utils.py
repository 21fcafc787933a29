"""Drop-ins for the reference's utils/utils.py helpers that homographic adaptation uses (utils/utils.py:250-332,388-454,
507-518): same names, signatures, argument shapes and return types; the arithmetic runs in libimx (csrc/homoadapt.hip).
GPU only: `device` must be a 'cuda' device (the reference's default 'cpu' has no meaning here and selects the current GPU)."""
import numpy as np
import torch

from ..engine import Engine

_engines = {}


def _engine(device=None):
    """One weight-less handle per device for the stages that need no network."""
    dev = torch.device(device) if device is not None and torch.device(device).type == "cuda" else torch.device("cuda")
    dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
    if dev not in _engines:
        _engines[dev] = Engine(None, None, dev)
    return _engines[dev]


def inv_warp_image_batch(img, mat_homo_inv, device='cpu', mode='bilinear'):
    """img [batch, 1, H, W] (or [H, W] / [1, H, W] with one matrix), mat_homo_inv [batch, 3, 3] -> [batch, 1, H, W]."""
    if img.dim() in (2, 3):
        img = img.reshape(1, 1, img.shape[-2], img.shape[-1])
    if mat_homo_inv.dim() == 2:
        mat_homo_inv = mat_homo_inv.reshape(1, 3, 3)
    B, C, H, W = img.shape
    if C != 1:
        raise ValueError(f"inv_warp_image_batch: one channel per image expected, got {C}")
    return _engine(device).warp_homography(img.reshape(B, H, W), mat_homo_inv, mode).reshape(B, 1, H, W)


def inv_warp_image(img, mat_homo_inv, device='cpu', mode='bilinear'):
    return inv_warp_image_batch(img, mat_homo_inv, device, mode).squeeze()


def compute_valid_mask(image_shape, inv_homography, device='cpu', erosion_radius=0):
    """-> [batch, H, W] float mask of the pixels whose (nearest) source lies inside the image."""
    if erosion_radius > 0:
        raise NotImplementedError("compute_valid_mask: erosion_radius > 0 is an OpenCV erosion in the reference; only 0 is provided")
    if inv_homography.dim() == 2:
        inv_homography = inv_homography.reshape(-1, 3, 3)
    return _engine(device).warp_homography((int(image_shape[0]), int(image_shape[1])), inv_homography, "nearest")


def combine_heatmap(heatmap, inv_homographies, mask_2D, device="cpu"):
    """heatmap, mask_2D [N, 1, H, W], inv_homographies [1, N, 3, 3] -> [1, H, W] (NaN where no map covers a pixel)."""
    N, _, H, W = heatmap.shape
    out = _engine(device).combine_heatmap(heatmap.reshape(N, H, W), mask_2D.reshape(N, H, W), inv_homographies[0, :, :, :])
    return out.reshape(1, H, W)


def getPtsFromHeatmap(heatmap, conf_thresh, nms_dist):
    """heatmap np (H, W) -> np float64 (3, K): rows x, y, conf by descending conf."""
    rows = _engine().heatmap_points_host(torch.as_tensor(np.ascontiguousarray(heatmap, dtype=np.float32)), conf_thresh, nms_dist)
    return np.ascontiguousarray(rows.T, dtype=np.float64)
