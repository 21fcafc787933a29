"""A restatement, in text of our own, of what libimx_sploop.so computes (csrc/sploop.hip, include/imx_sploop.h): the bilinear label splat
of the reference's gaussian_label with its 8-bit round trip, and one Adam step -- numpy on the CPU, every step with the line of the
reference it restates.  It is held to the fixtures the reference wrote (tests/golden/make_golden_sploop.py) and to torch.optim.Adam
by tests/test_sploop_host.py, and the kernels are held to it and to those fixtures by tests/test_gpu_sploop.py."""
import math

import numpy as np

from tests import sptrain_ref as R

F32 = np.float32


# ---------------------------------------------------------------------------------------------- labels
def quantise(img, levels=255):
    """The two lines of ImgAugTransform.__call__ round the augmenter (utils/photometric.py:74, :76): (img * 255).astype(np.uint8), then
    .astype(np.float32) / 255.  A value outside [0, 255] is clamped (the reference's cast is undefined there; imx_warp_labels_bi's choice).
    levels = 0: the map as it is."""
    img = np.asarray(img, F32)
    if levels == 0:
        return img
    q = np.clip(np.trunc((img * F32(255)).astype(F32)), 0, 255).astype(np.uint8)
    return q.astype(F32) / F32(255)


def labels_bi(pts, mat_px, H, W, levels=0):
    """get_labels_bi (datasets/data_tools.py:9-34) as warpLabels(..., bilinear=True) calls it (:36-47), in fp32: .long(), warp_points by the
    pixel-space matrix, NO filter on the warped point; extrapolate_points: p_int = trunc(p), r = p - p_int, the four corners in the
    order (x, y), (x, y+1), (x+1, y), (x+1, y+1) with weights (1-rx)(1-ry), (1-rx)ry, rx(1-ry), rx ry; filter_points on the corners;
    scatter_points as a SEQUENTIAL assignment in concatenation order (k-major, then the point index): the last writer of a pixel wins.
    A non-finite warped point is dropped (flag bit 1); a kept weight outside [0,1] raises flag bit 0.  Returns (map (H,W) fp32, flag)."""
    out, flag = np.zeros((H, W), F32), 0
    p = np.trunc(np.asarray(pts, F32).reshape(-1, 2))
    if len(p) == 0:
        return out, flag
    wx, wy = R.warp_points(mat_px, p[:, 0], p[:, 1])
    with np.errstate(all="ignore"):
        qx, qy = np.trunc(wx), np.trunc(wy)
        rx, ry = (wx - qx).astype(F32), (wy - qy).astype(F32)
        ex, ey = (F32(1) - rx).astype(F32), (F32(1) - ry).astype(F32)
        corners = ((qx, qy, ex * ey), (qx, qy + F32(1), ex * ry), (qx + F32(1), qy, rx * ey), (qx + F32(1), qy + F32(1), rx * ry))
    finite = np.isfinite(wx) & np.isfinite(wy)
    if not finite.all():
        flag |= 2
    for cx, cy, w in corners:                                          # k ascending ...
        w = w.astype(F32)
        for i in range(len(p)):                                        # ... then the point index: the reference's concatenation
            if not finite[i]:
                continue
            if 0 <= cx[i] <= W - 1 and 0 <= cy[i] <= H - 1:            # filter_points (utils/utils.py:551-559)
                if not 0 <= w[i] <= 1:
                    flag |= 1
                out[int(cy[i]), int(cx[i])] = w[i]
    return quantise(out, levels) if levels else out, flag


# ---------------------------------------------------------------------------------------------- Adam
def bias_terms(lr, betas, step):
    """(step_size, inv_sqrt_bc2) in double: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)"""
    return lr / (1.0 - betas[0] ** step), 1.0 / math.sqrt(1.0 - betas[1] ** step)


def adam_step(p, g, m, v, lr, betas, eps, weight_decay, step, dtype=np.float64):
    """One step of torch.optim.Adam (amsgrad=False, maximize=False) in include/imx_sploop.h's order of operations, every operation rounded
    to `dtype` on its own; the scalars are rounded to `dtype` once (1 - beta from the double difference).  Returns new (p, m, v)."""
    T = dtype
    p, g, m, v = (np.asarray(a, T) for a in (p, g, m, v))
    step_size, inv_sqrt_bc2 = bias_terms(lr, betas, step)
    b2, c1, c2 = T(betas[1]), T(1.0 - betas[0]), T(1.0 - betas[1])
    if weight_decay != 0:
        g = (g + (T(weight_decay) * p).astype(T)).astype(T)
    m = (m + (c1 * (g - m).astype(T)).astype(T)).astype(T)
    v = ((b2 * v).astype(T) + ((c2 * g).astype(T) * g).astype(T)).astype(T)
    d = ((np.sqrt(v).astype(T) * T(inv_sqrt_bc2)).astype(T) + T(eps)).astype(T)
    p = (p - (T(step_size) * (m / d).astype(T)).astype(T)).astype(T)
    return p, m, v


# ---------------------------------------------------------------------------------------------- the sigma gate
def blur_defect(sigma):
    """255 (1 - w0^2): an upper bound, in 8-bit levels, on what a normalised 7-tap Gaussian of this sigma moves any pixel of an 8-bit
    image (w0 its centre tap; the 2-D kernel's off-centre mass is 1 - w0^2)"""
    w0 = 1.0 / (1.0 + 2.0 * sum(math.exp(-x * x / (2.0 * sigma * sigma)) for x in (1, 2, 3)))
    return 255.0 * (1.0 - w0 * w0)


# ---------------------------------------------------------------------------------------------- Adam: shared cases and the bar
ADAM_HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
ADAM_STEPS = 5


def adam_case(n, seed, t0=0):
    """Seeded inputs of ADAM_STEPS steps on n floats, fp32: parameters, one gradient per step and -- for a run that starts after t0 steps --
    moments as t0 steps would have left them (exp_avg of the gradients' size, exp_avg_sq of their squares' size)."""
    rng = np.random.default_rng([seed, n, t0])
    p = rng.standard_normal(n).astype(F32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(F32) for _ in range(ADAM_STEPS)]
    m = (rng.standard_normal(n) * 0.1).astype(F32) if t0 else np.zeros(n, F32)
    v = (rng.random(n) * 0.01).astype(F32) if t0 else np.zeros(n, F32)
    return p, grads, m, v


def adam_run(case, weight_decay, t0, dtype):
    """ADAM_STEPS steps of adam_step from a case; the parameters after every step"""
    p, grads, m, v = case
    out = []
    for k, g in enumerate(grads):
        p, m, v = adam_step(p, g, m, v, weight_decay=weight_decay, step=t0 + k + 1, dtype=dtype, **ADAM_HYPER)
        out.append(p)
    return out


def adam_torch(case, weight_decay, t0, dtype, device="cpu"):
    """the same steps by torch.optim.Adam on the CPU (or on `device`) in `dtype` (torch.float32 / torch.float64); the parameters after
    every step"""
    import torch
    p0, grads, m0, v0 = case
    p = torch.nn.Parameter(torch.from_numpy(np.array(p0)).to(device, dtype))
    opt = torch.optim.Adam([p], weight_decay=weight_decay, **ADAM_HYPER)
    if t0:
        sd = opt.state_dict()
        sd["state"] = {0: {"step": torch.tensor(float(t0)), "exp_avg": torch.from_numpy(np.array(m0)).to(device, dtype),
                           "exp_avg_sq": torch.from_numpy(np.array(v0)).to(device, dtype)}}
        opt.load_state_dict(sd)
    out = []
    for g in grads:
        p.grad = torch.from_numpy(np.array(g)).to(device, dtype)
        opt.step()
        out.append(p.detach().cpu().clone().numpy())
    return out


def adam_bar(case, weight_decay, t0):
    """(p64 after the last step, the bar): the float64 restatement is the reference; the bar is twice what torch.optim.Adam in fp32 on the
    CPU shows against it on the same inputs -- the margin of 2 for a different but equally valid fp32 order"""
    import torch
    p64 = adam_run(case, weight_decay, t0, np.float64)[-1]
    t32 = adam_torch(case, weight_decay, t0, torch.float32)[-1]
    return p64, 2.0 * float(np.abs(t32.astype(np.float64) - p64).max())
