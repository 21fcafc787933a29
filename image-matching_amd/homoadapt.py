"""Homographic adaptation (the reference's superpoint_export_pseudo.py): the host-side homography sampler and the
fused per-image export call.  All arithmetic on images and heatmaps runs in libimx (csrc/homoadapt.hip)."""
import math

import numpy as np

# the `homographies.params` block of superpoint/configs/magicpoint_allss_export.yaml over the defaults of
# utils/homographies.py:12-16
SAMPLER_DEFAULTS = dict(perspective=True, scaling=True, rotation=True, translation=True, n_scales=5, n_angles=25,
                        scaling_amplitude=0.1, perspective_amplitude_x=0.1, perspective_amplitude_y=0.1, patch_ratio=0.5,
                        max_angle=math.pi / 2, allow_artifacts=False, translation_overflow=0.)
EXPORT_PARAMS = dict(translation=True, rotation=True, scaling=True, perspective=True, scaling_amplitude=0.2,
                     perspective_amplitude_x=0.2, perspective_amplitude_y=0.2, allow_artifacts=True, patch_ratio=0.85)


def _truncated_normal(rng, loc, scale, size, bound=2.0):
    """normal(loc, scale) restricted to loc +- bound * scale, by rejection"""
    out = np.empty(size)
    todo = np.arange(size)
    while todo.size:
        z = rng.standard_normal(todo.size)
        ok = np.abs(z) <= bound
        out[todo[ok]] = z[ok]
        todo = todo[~ok]
    return loc + scale * out


def four_point_transform(src, dst):
    """The 3x3 matrix (last entry 1) that maps the four points src -> dst: the 8x8 linear system of the projective
    relation, in float64."""
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A.append([x, y, 1, 0, 0, 0, -x * u, -y * u])
        A.append([0, 0, 0, x, y, 1, -x * v, -y * v])
        b += [u, v]
    return np.append(np.linalg.solve(np.asarray(A, np.float64), np.asarray(b, np.float64)), 1.0).reshape(3, 3)


def sample_patch_corners(rng, **params):
    """Corners (4,2) in the unit square of one random patch: a centred patch_ratio crop, then a perspective displacement,
    a scale, a translation and a rotation, each drawn as utils/homographies.py:57-106 describes.  Without
    allow_artifacts the scale and the rotation are drawn among those that keep the patch inside [0, 1)."""
    p = {**SAMPLER_DEFAULTS, **params}
    ratio = p["patch_ratio"]
    margin = (1 - ratio) / 2
    c = margin + np.array([[0, 0], [0, ratio], [ratio, ratio], [ratio, 0]], np.float64)
    if p["perspective"]:
        ax, ay = p["perspective_amplitude_x"], p["perspective_amplitude_y"]
        if not p["allow_artifacts"]:
            ax, ay = min(ax, margin), min(ay, margin)
        dy = _truncated_normal(rng, 0., ay / 2, 1)[0]
        dl = _truncated_normal(rng, 0., ax / 2, 1)[0]
        dr = _truncated_normal(rng, 0., ax / 2, 1)[0]
        c += np.array([[dl, dy], [dl, -dy], [dr, dy], [dr, -dy]])

    def inside(q):
        return np.nonzero(((q >= 0.) & (q < 1.)).all(axis=(1, 2)))[0]
    if p["scaling"]:
        s = np.concatenate([[1.], _truncated_normal(rng, 1., p["scaling_amplitude"] / 2, p["n_scales"])])
        mid = c.mean(0, keepdims=True)
        cand = (c - mid)[None] * s[:, None, None] + mid
        ok = np.arange(p["n_scales"]) if p["allow_artifacts"] else inside(cand)
        c = cand[ok[rng.integers(len(ok))]]
    if p["translation"]:
        lo, hi = c.min(0), (1 - c).min(0)
        if p["allow_artifacts"]:
            lo, hi = lo + p["translation_overflow"], hi + p["translation_overflow"]
        # (with artifacts allowed the patch may already stick out and an interval be reversed: u in [0,1) spans it either way)
        c = c + (-lo + (hi + lo) * rng.random(2))
    if p["rotation"]:
        ang = np.concatenate([np.linspace(-p["max_angle"], p["max_angle"], p["n_angles"]), [0.]])
        mid = c.mean(0, keepdims=True)
        rot = np.stack([np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)], 1).reshape(-1, 2, 2)
        cand = np.matmul((c - mid)[None], rot) + mid
        ok = np.arange(p["n_angles"]) if p["allow_artifacts"] else inside(cand)
        c = cand[ok[rng.integers(len(ok))]]
    return c


def sample_homographies(n, seed=0, **params):
    """The two matrix stacks of datasets/ALLSS.py:156-166 for n views, on [-1,1]^2 coordinates: (homographies,
    inv_homographies), float32 (n,3,3), homographies[0] the identity, inv_homographies their fp32 inverses.
    Parameters: the names and defaults of utils/homographies.py:12-16 (EXPORT_PARAMS holds the shipped yaml's values).
    Host plumbing with numpy's own random stream (the reference draws from scipy and solves with OpenCV): the
    matrices are valid samples of the same family but NOT the reference's stream -- unpinned."""
    rng = np.random.default_rng(seed)
    unit = np.array([[0., 0.], [0., 1.], [1., 1.], [1., 0.]])
    H = np.empty((n, 3, 3), np.float64)
    for i in range(n):
        # the unit square scaled to [-1,1]^2 (shape (2,2), shift -1), unit corners -> patch corners, then inverted (ALLSS.py:162)
        M = four_point_transform(unit * 2 - 1, sample_patch_corners(rng, **params) * 2 - 1)
        H[i] = np.linalg.inv(M)
    if n:
        H[0] = np.eye(3)
    H32 = H.astype(np.float32)
    inv32 = np.stack([np.linalg.inv(m) for m in H32]).astype(np.float32) if n else H32.copy()
    return H32, inv32


def export_image(engine, img, homographies, inv_homographies, conf_thresh=0.015, nms_dist=4, top_k=0, subpixel=False):
    """One image (H,W) through superpoint_export_pseudo.py:58-99 on the GPU: the image is warped by inv_homographies, the
    heatmaps come back by homographies (the script's names are swapped, :63-66), then points.  Two library calls on one
    stream, then ONE device-to-host copy of the rows.  Returns pts (K,3) float32 numpy rows (x, y, conf)."""
    heat = engine.homography_adapt(img, inv_homographies, homographies)
    return engine.heatmap_points_host(heat, conf_thresh, nms_dist, top_k=top_k, subpixel=subpixel)
