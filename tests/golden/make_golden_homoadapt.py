"""Writes the homographic-adaptation fixtures from the REFERENCE itself (imported unchanged; never runs where the
reference is absent):

    python tests/golden/make_golden_homoadapt.py --reference /path/to/reference

  homoadapt_small.npz    120 x 160, N = 8, first matrix the identity (every pixel has count >= 1)
  homoadapt_ragged.npz   136 x 200, N = 5, no identity: some pixels are covered by no warp (count 0, reference NaN)
each with its two stacks in files of their own (<name>_warped.npz, <name>_heat.npz) and the float64 evaluation of either stack as
float32 differences from it (<name>_warped_d64.npz, <name>_heat_d64.npz, the convention of the strict fixtures), so that every
committed file stays below 1 MiB, the project's limit for a committed file.  The float64 evaluation is the same pipeline through
tests/homoadapt_ref.py with the reference network in double; the combined map's sits in the main file.  The matrices come from
the sampler BELOW (the generator's own, seeded; a frozen copy of the algorithm, so that a later change of the product's sampler
cannot make these fixtures unreproducible).  The reference's utils/utils.py imports OpenCV at module level and calls
it in none of the functions used here: an empty module stands in for it."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

NMS = 4
THR_E2E, THR_INJ = 0.05, 0.015      # end-to-end comparisons need a threshold the reference is stable at (condition 3)


def load_reference(path):
    sys.path.insert(0, path)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    import utils.utils as U                                            # noqa: E402  (the reference's)
    from superpoint.models.superpoint_train import SuperPoint         # noqa: E402
    return U, SuperPoint


# ---------------------------------------------------------------------------------------------- the generator's own sampler
EXPORT_PARAMS = dict(scaling_amplitude=0.2, perspective_amplitude_x=0.2, perspective_amplitude_y=0.2, patch_ratio=0.85, n_scales=5, n_angles=25)


def _tnormal(rng, loc, scale, size):
    out, todo = np.empty(size), np.arange(size)
    while todo.size:
        z = rng.standard_normal(todo.size)
        ok = np.abs(z) <= 2.0
        out[todo[ok]] = z[ok]
        todo = todo[~ok]
    return loc + scale * out


def _four_points(src, dst):
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A += [[x, y, 1, 0, 0, 0, -x * u, -y * u], [0, 0, 0, x, y, 1, -x * v, -y * v]]
        b += [u, v]
    return np.append(np.linalg.solve(np.asarray(A, np.float64), np.asarray(b, np.float64)), 1.0).reshape(3, 3)


def sample_matrices(n, seed, scaling_amplitude, perspective_amplitude_x, perspective_amplitude_y, patch_ratio, n_scales, n_angles):
    """(homographies, inv_homographies) float32 (n,3,3) on [-1,1]^2, artifacts allowed, first matrix the identity: perspective, scale,
    translation and rotation of a centred patch, the four-point transform, inverted; fp32 inverses as datasets/ALLSS.py:162-166."""
    rng = np.random.default_rng(seed)
    unit = np.array([[0., 0.], [0., 1.], [1., 1.], [1., 0.]])
    H = np.empty((n, 3, 3))
    for i in range(n):
        c = (1 - patch_ratio) / 2 + unit * patch_ratio
        dy = _tnormal(rng, 0., perspective_amplitude_y / 2, 1)[0]
        dl = _tnormal(rng, 0., perspective_amplitude_x / 2, 1)[0]
        dr = _tnormal(rng, 0., perspective_amplitude_x / 2, 1)[0]
        c = c + np.array([[dl, dy], [dl, -dy], [dr, dy], [dr, -dy]])
        s = np.concatenate([[1.], _tnormal(rng, 1., scaling_amplitude / 2, n_scales)])
        mid = c.mean(0, keepdims=True)
        c = ((c - mid)[None] * s[:, None, None] + mid)[rng.integers(n_scales)]
        lo, hi = c.min(0), (1 - c).min(0)
        c = c + (-lo + (hi + lo) * rng.random(2))
        ang = np.concatenate([np.linspace(-np.pi / 2, np.pi / 2, n_angles), [0.]])
        mid = c.mean(0, keepdims=True)
        rot = np.stack([np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)], 1).reshape(-1, 2, 2)
        c = (np.matmul((c - mid)[None], rot) + mid)[rng.integers(n_angles)]
        H[i] = np.linalg.inv(_four_points(unit * 2 - 1, c * 2 - 1))
    H[0] = np.eye(3)
    H32 = H.astype(np.float32)
    return H32, np.stack([np.linalg.inv(m) for m in H32]).astype(np.float32)


def stress_maps():
    """Maps that stress the NMS, values distinct wherever two candidates are within reach of each other."""
    rng = np.random.default_rng(7)
    out = {}
    H, W = 40, 56
    ramp = (0.02 + 0.9 * (np.arange(H * W, dtype=np.float64).reshape(H, W) / (H * W))).astype(np.float32)
    out["ramp"] = ramp                                                 # plateau-free: every pixel a candidate
    out["ramp_rev"] = ramp[::-1, ::-1].copy()
    chain = np.zeros((120, 160), np.float32)                           # suppression chains far longer than the bounded rounds:
    for k in range(38):                                                # each point within nms_dist of the next, strictly decreasing
        chain[4 + 3 * k, 4 + 3 * k] = 0.9 - 0.01 * k                   # ... from the top-left down
        chain[4 + 3 * k, 155 - 3 * k] = 0.5 + 0.01 * k + 0.001         # ... and from the bottom-left up (decided last to first)
    out["chain"] = chain
    border = np.zeros((H, W), np.float32)
    for i, (y, x) in enumerate([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (3, 20), (4, 20), (H - 4, 30), (H - 5, 31), (20, 3),
                                (20, 4), (21, W - 4), (22, W - 5), (2, 2), (5, 5), (10, 10), (12, 13)]):
        border[y, x] = 0.3 + 0.01 * i                                  # border points suppress their neighbours before they are removed
    out["border"] = border
    out["empty"] = np.full((H, W), 0.001, np.float32)
    one = np.full((H, W), 0.001, np.float32)
    one[17, 23] = 0.7
    out["one"] = one
    noise = rng.random((H, W)).astype(np.float32) * 0.2
    noise[5:9, 7:30] = np.nan                                          # NaN is never a candidate
    out["nan"] = noise
    return out


def no_close_ties(h, thr, nms):
    """condition 1: no two candidates of equal fp32 value within nms of each other"""
    ys, xs = np.where(h >= thr)
    v = h[ys, xs]
    for val in np.unique(v)[np.unique(v, return_counts=True)[1] > 1]:
        y, x = ys[v == val], xs[v == val]
        d = np.maximum(np.abs(y[:, None] - y[None]), np.abs(x[:, None] - x[None]))
        if (d[np.triu_indices(len(y), 1)] <= nms).any():
            return False
    return True


def build(U, SuperPoint, name, H, W, N, identity, seed):
    from tests import homoadapt_ref as R
    from tests import util
    img = util.pair(seed, H, W)[0][0, 0]                               # (H,W) float32
    hom, inv = sample_matrices(N + 1, seed, **EXPORT_PARAMS)
    hom, inv = (hom[:N], inv[:N]) if identity else (hom[1:], inv[1:])
    hom_t, inv_t = torch.from_numpy(hom), torch.from_numpy(inv)
    net = SuperPoint(128).eval()
    net.load_state_dict(util.sp_sd(128))
    with torch.no_grad():
        # datasets/ALLSS.py:168-175 and superpoint_export_pseudo.py:58-80, the reference's own functions
        warped = U.inv_warp_image_batch(img.repeat(N, 1, 1, 1), inv_t, mode="bilinear")          # (N,1,H,W)
        mask = U.compute_valid_mask(torch.tensor([H, W]), inv_homography=inv_t, erosion_radius=0)  # (N,H,W)
        heat = U.flattenDetection(net(warped)["semi"], tensor=True)                               # (N,1,H,W)
        den = U.inv_warp_image_batch(mask[:, None], hom_t, mode="bilinear").sum(0)[0]
        comb = U.combine_heatmap(heat, hom_t[None], mask[:, None])[0]                             # (H,W)
        # float64: the same pipeline through the restatement, the reference network in double
        w64 = R.warp(img.double(), inv, "bilinear", torch.float64)
        h64 = R.flatten_detection(net.double()(w64[:, None])["semi"])
        c64, _ = R.combine(h64, R.valid_mask(inv, H, W, torch.float64), hom, torch.float64)
        net.float()
    comb_np, den_np = comb.numpy(), den.numpy()
    fx = {"seed": np.int64(seed), "size": np.array([H, W], np.int64), "homographies": hom, "inv_homographies": inv,
          "mask": mask.numpy().astype(np.uint8), "combined": comb_np, "count": den_np, "combined_f64": c64.numpy()}
    # condition 2: pixels whose float64 source coordinate is within 1e-3 px of a mask edge are the only ones a mask test may skip
    px = R.source_pixels(inv, H, W).numpy()
    edge = np.zeros((N, H, W), bool)
    for coord, size in ((px[..., 0], W), (px[..., 1], H)):
        edge |= (np.abs(coord + 0.5) < 1e-3) | (np.abs(coord - (size - 0.5)) < 1e-3)
    assert edge.mean() <= 1e-4, f"{name}: {edge.sum()} pixels on a mask edge"
    m64 = R.valid_mask(inv, H, W, torch.float64).numpy()
    assert ((m64 != mask.numpy()) & ~edge).sum() == 0, f"{name}: fp32 and float64 masks differ away from the edges"
    fx["mask_edge_pixels"] = np.argwhere(edge).astype(np.int32).reshape(-1, 3)
    # points: the reference's getPtsFromHeatmap on its own map
    ref_map = comb_np.astype(np.float32)
    for thr in (THR_INJ, THR_E2E):
        for nms in (NMS, 1):
            assert no_close_ties(ref_map, thr, nms), f"{name}: equal candidates within nms_dist {nms} at {thr}"      # condition 1
            fx[f"pts_{thr}_{nms}"] = U.getPtsFromHeatmap(ref_map, thr, nms)
    # condition 3: the end-to-end threshold is one the reference itself is stable at under the project tolerance
    base = set(map(tuple, fx[f"pts_{THR_E2E}_{NMS}"][:2].T.astype(int)))
    rng = np.random.default_rng(seed)
    finite = np.nan_to_num(ref_map, nan=0.0)
    for _ in range(8):
        noisy = (ref_map + (rng.random(ref_map.shape) * 2 - 1) * (1e-4 + 1e-4 * np.abs(finite))).astype(np.float32)
        got = set(map(tuple, U.getPtsFromHeatmap(noisy, THR_E2E, NMS)[:2].T.astype(int)))
        assert len(got ^ base) <= 0.02 * max(len(base), 1), f"{name}: threshold {THR_E2E} is not stable ({len(got ^ base)} of {len(base)})"
    assert len(base) >= 10, f"{name}: only {len(base)} points at {THR_E2E}"
    if identity:
        assert (den_np >= 1 - 1e-6).all()
    else:
        keep = (den_np >= 0.5).mean()
        assert keep >= 0.85 and (den_np == 0).any(), f"{name}: count >= 0.5 on {keep:.3f} of the pixels, {(den_np == 0).sum()} of count 0"
        assert np.isnan(comb_np[den_np == 0]).all() and not np.isinf(comb_np).any()
    print(f"{name}: {len(base)} points at {THR_E2E}, {fx[f'pts_{THR_INJ}_{NMS}'].shape[1]} at {THR_INJ}; count 0 on {(den_np == 0).sum()} pixels, "
          f">= 0.5 on {(den_np >= 0.5).mean():.3f}; {edge.sum()} mask-edge pixels; |ref32 - f64| max {np.nanmax(np.abs(comb_np - c64.numpy())):.2e}")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **fx)
    np.savez_compressed(os.path.join(HERE, name + "_warped.npz"), warped=warped[:, 0].numpy())
    np.savez_compressed(os.path.join(HERE, name + "_heat.npz"), heat=heat[:, 0].numpy())
    np.savez_compressed(os.path.join(HERE, name + "_warped_d64.npz"), warped_d64=(w64 - warped[:, 0].double()).float().numpy())
    np.savez_compressed(os.path.join(HERE, name + "_heat_d64.npz"), heat_d64=(h64 - heat[:, 0].double()).float().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    U, SuperPoint = load_reference(a.reference)
    build(U, SuperPoint, "homoadapt_small", 120, 160, 8, True, 12)
    build(U, SuperPoint, "homoadapt_ragged", 136, 200, 5, False, 12)
    st = {}
    for key, m in stress_maps().items():
        st["map_" + key] = m
        for nms in (NMS, 1):
            assert no_close_ties(m, THR_INJ, nms), key
            st[f"pts_{key}_{nms}"] = U.getPtsFromHeatmap(m, THR_INJ, nms)
    np.savez_compressed(os.path.join(HERE, "homoadapt_stress.npz"), **st)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("homoadapt_"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < (1 << 20), f"{f}: {size} bytes"
            print(f, size)


if __name__ == "__main__":
    main()
