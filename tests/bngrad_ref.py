"""The project's own statement of what the kernels of csrc/bn_train.hip compute: nn.BatchNorm1d followed by nn.ReLU
(superglue/models/superglue_train.py:55-56, inside every MLP) and its derivative with respect to the input, the weight and the bias, as
the closed forms of DESIGN.md section 16 written out in torch on the CPU (float64 or fp32) -- no autograd in forward() / backward();
autograd() differentiates the same written forward with torch.autograd for the cross-check.  Held to the fixtures the reference's own
MLP and KeypointEncoder wrote under torch.autograd (tests/golden/make_golden_bngrad.py) by tests/test_bngrad_host.py; the kernels are
held to it and to those fixtures by tests/test_gpu_bngrad.py.  No bits are claimed between this file and the kernels.

Tensors are the reference's: x, y, dy, dx (B,C,N); gamma, beta, mean, rstd, dgamma, dbeta, running_mean, running_var (C).  n (B) counts or
None: columns past n[b] are never read (they may hold NaN), y and dx are 0 there, and they add nothing to any sum; the statistics are
those of the valid columns of all pairs, M = sum(n) of them."""
import numpy as np
import torch

from tests.mhagrad_ref import heavy
from tests.otgrad_ref import bar  # noqa: F401  (the default bar, element-wise: max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|))

EPS, MOMENTUM = 1e-5, 0.1           # nn.BatchNorm1d's defaults, which the reference's MLP() keeps
KINK = 1e-5                         # |z64| below this: the element may fall on either side of the ReLU in fp32


# ---------------------------------------------------------------------------------------------- seeded cases
def case(seed, B, C, N):
    """x (B,C,N), gamma (C) = 1 + 0.1 heavy, beta (C) = 0.1 heavy, dy (B,C,N): fp32, heavy-tailed"""
    gamma = (1.0 + 0.1 * heavy(seed, "bn.gamma", (C,)).astype(np.float64)).astype(np.float32)
    beta = (0.1 * heavy(seed, "bn.beta", (C,)).astype(np.float64)).astype(np.float32)
    return heavy(seed, "bn.x", (B, C, N)), gamma, beta, heavy(seed, "bn.dy", (B, C, N))


def running(seed, C):
    """seeded running statistics of a module that has seen data: mean 0.3 heavy, var 0.5 + heavy^2 (positive), fp32"""
    h = heavy(seed, "bn.rvar", (C,)).astype(np.float64)
    return (0.3 * heavy(seed, "bn.rmean", (C,)).astype(np.float64)).astype(np.float32), (0.5 + h * h).astype(np.float32)


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _counts(c, B, cap):
    return [cap] * B if c is None else [min(max(int(x), 0), cap) for x in np.asarray(c).reshape(-1)]


def _valid(x, counts):
    """the valid columns of all pairs, concatenated: (C, M)"""
    return torch.cat([x[b, :, :cnt] for b, cnt in enumerate(counts)], 1)


def ragged_pad(a, counts, frame, fill=np.nan):
    """(1,C,M) with M = sum(counts) -> (len(counts), C, frame): pair b holds its counts[b] columns, `fill` past them"""
    out = np.full((len(counts), a.shape[1], frame), fill, a.dtype)
    off = 0
    for b, cnt in enumerate(counts):
        out[b, :, :cnt] = a[0, :, off:off + cnt]
        off += cnt
    return out


def ragged_cat(a, counts):
    """the inverse: the valid columns of (B,C,frame) concatenated into (1,C,M)"""
    return np.concatenate([a[b, :, :cnt] for b, cnt in enumerate(counts)], 1)[None]


# ---------------------------------------------------------------------------------------------- the closed forms
def forward(x, gamma, beta, n=None, training=True, running_mean=None, running_var=None, eps=EPS, momentum=MOMENTUM, dtype=torch.float64):
    """-> dict of float64 arrays: y and z (B,C,N) (0 past the counts), mean, rstd (C) and, where given, running_mean / running_var after
    the step (unchanged in evaluation mode, with M = 0, and running_var with M = 1)"""
    x, gamma, beta = _t(x, dtype), _t(gamma, dtype), _t(beta, dtype)
    B, C, N = x.shape
    counts = _counts(n, B, N)
    M = sum(counts)
    rm = None if running_mean is None else _t(running_mean, dtype).clone()
    rv = None if running_var is None else _t(running_var, dtype).clone()
    z = torch.zeros(B, C, N, dtype=dtype)
    if M == 0:
        mean, rstd = torch.zeros(C, dtype=dtype), torch.zeros(C, dtype=dtype)
    else:
        if training:
            v = _valid(x, counts)
            mean = v.sum(1) / M
            var = ((v - mean[:, None]) ** 2).sum(1) / M
            if rm is not None:
                rm = (1 - momentum) * rm + momentum * mean
            if rv is not None and M > 1:
                rv = (1 - momentum) * rv + momentum * (var * M / (M - 1))
        else:
            mean, var = rm.clone(), rv.clone()
        rstd = 1 / torch.sqrt(var + eps)
        for b, cnt in enumerate(counts):
            z[b, :, :cnt] = (x[b, :, :cnt] - mean[:, None]) * rstd[:, None] * gamma[:, None] + beta[:, None]
    out = {"y": torch.clamp(z, min=0), "z": z, "mean": mean, "rstd": rstd}
    if rm is not None:
        out["running_mean"] = rm
    if rv is not None:
        out["running_var"] = rv
    return {k: v.double().numpy() for k, v in out.items()}


def backward(x, gamma, beta, mean, rstd, dy, n=None, training=True, mask=None, dtype=torch.float64):
    """-> dx (B,C,N), dgamma (C), dbeta (C) as float64 arrays; mean and rstd are the forward's.  mask (B,C,N) booleans replaces z > 0
    (only its valid columns are read)."""
    x, gamma, beta, mean, rstd = (_t(a, dtype) for a in (x, gamma, beta, mean, rstd))
    dy = _t(dy, dtype)
    B, C, N = x.shape
    counts = _counts(n, B, N)
    M = sum(counts)
    dx, dgamma, dbeta = torch.zeros(B, C, N, dtype=dtype), torch.zeros(C, dtype=dtype), torch.zeros(C, dtype=dtype)
    if M == 0:
        return dx.numpy().astype(np.float64), dgamma.numpy().astype(np.float64), dbeta.numpy().astype(np.float64)
    xhat, g = [], []
    for b, cnt in enumerate(counts):
        xh = (x[b, :, :cnt] - mean[:, None]) * rstd[:, None]
        on = (xh * gamma[:, None] + beta[:, None] > 0) if mask is None else torch.as_tensor(np.asarray(mask))[b, :, :cnt]
        xhat.append(xh)
        g.append(torch.where(on, dy[b, :, :cnt], torch.zeros((), dtype=dtype)))
    dbeta = torch.cat(g, 1).sum(1)
    dgamma = (torch.cat(g, 1) * torch.cat(xhat, 1)).sum(1)
    k = (gamma * rstd)[:, None]
    for b, cnt in enumerate(counts):
        dx[b, :, :cnt] = k * (g[b] - dbeta[:, None] / M - xhat[b] * dgamma[:, None] / M) if training else k * g[b]
    return dx.double().numpy(), dgamma.double().numpy(), dbeta.double().numpy()


def bn_relu_written(x, gamma, beta, training=True, running_mean=None, running_var=None, eps=EPS, mask=None):
    """the written forward on a full tensor, as the reference's modules have it (restated): relu(batch_norm(x)); with a mask, z * mask
    in place of the ReLU"""
    z = torch.nn.functional.batch_norm(x, None if training else running_mean, None if training else running_var, gamma, beta, training, 0.0, eps)
    return torch.relu(z) if mask is None else z * torch.as_tensor(np.asarray(mask)).to(z.dtype)


def autograd(x, gamma, beta, dy, training=True, running_mean=None, running_var=None, eps=EPS, mask=None, dtype=torch.float64):
    """the written forward differentiated by torch.autograd on full (unpadded) tensors -> dict of float64 arrays: y, dx, dgamma, dbeta"""
    with torch.enable_grad():
        leaves = [_t(a, dtype).requires_grad_(True) for a in (x, gamma, beta)]
        stats = [None if a is None else _t(a, dtype) for a in (running_mean, running_var)]
        y = bn_relu_written(*leaves, training, *stats, eps, mask)
        grads = torch.autograd.grad(y, leaves, _t(dy, dtype))
    return {"y": y.detach().double().numpy(), **{k: g.double().numpy() for k, g in zip(("dx", "dgamma", "dbeta"), grads)}}


def batch_reference(x, gamma, beta, dy, n=None, training=True, running_mean=None, running_var=None, eps=EPS, momentum=MOMENTUM, mask=None,
                    dtype=torch.float64):
    """everything the two entry points write, as a dict of float64 arrays (and z, the pre-activation)"""
    res = forward(x, gamma, beta, n, training, running_mean, running_var, eps, momentum, dtype)
    res["dx"], res["dgamma"], res["dbeta"] = backward(x, gamma, beta, res["mean"], res["rstd"], dy, n, training, mask, dtype)
    return res


def kink(z64, n=None):
    """the boolean map of valid elements whose float64 pre-activation lies within KINK of 0"""
    z64 = np.asarray(z64)
    near = np.abs(z64) < KINK
    for b, cnt in enumerate(_counts(n, z64.shape[0], z64.shape[2])):
        near[b, :, cnt:] = False
    return near


# ---------------------------------------------------------------------------------------------- the keypoint encoder, restated
class KeypointEncoder(torch.nn.Module):
    """superglue_train.py:70-79 restated: MLP([3] + layers + [feature_dim]) on cat([kpts^T, scores])"""

    def __init__(self, feature_dim, layers):
        super().__init__()
        ch = [3] + list(layers) + [feature_dim]
        mods = []
        for i in range(1, len(ch)):
            mods.append(torch.nn.Conv1d(ch[i - 1], ch[i], kernel_size=1, bias=True))
            if i < len(ch) - 1:
                mods += [torch.nn.BatchNorm1d(ch[i]), torch.nn.ReLU()]
        self.encoder = torch.nn.Sequential(*mods)

    def forward(self, kpts, scores):
        return self.encoder(torch.cat([kpts.transpose(1, 2), scores.unsqueeze(1)], dim=1))


def kenc_parameters(seed, module):
    """seeded values for every parameter of a KeypointEncoder (the reference's or the restated one: the names agree), name -> fp32 array:
    convolution weights heavy / sqrt(fan-in), biases 0.1 heavy, BatchNorm weights 1 + 0.1 heavy"""
    bn_weights = {f"encoder.{i}.weight" for i, m in enumerate(module.encoder) if isinstance(m, torch.nn.BatchNorm1d)}
    out = {}
    for name, p in module.named_parameters():
        h = heavy(seed, "kenc." + name, tuple(p.shape)).astype(np.float64)
        h = h / np.sqrt(p.shape[1]) if p.dim() == 3 else 0.1 * h + (1.0 if name in bn_weights else 0.0)
        out[name] = h.astype(np.float32)
    return out


def kenc_case(seed, N, d):
    """kpts (1,N,2) normalised keypoints, scores (1,N) in (0,1), dy (1,d,N) fp32"""
    s = heavy(seed, "kenc.scores", (1, N)).astype(np.float64)
    return ((0.5 * heavy(seed, "kenc.kpts", (1, N, 2)).astype(np.float64)).astype(np.float32), (1 / (1 + np.exp(-s))).astype(np.float32),
            heavy(seed, "kenc.dy", (1, d, N)))


def kenc_grads(module, forward, kpts, scores, dy):
    """out = forward(kpts, scores) on leaves, the gradients of sum(out * dy) -> dict name -> tensor: out, dkpts, dscores and one per
    parameter"""
    module.zero_grad()
    kpts, scores = kpts.clone().requires_grad_(True), scores.clone().requires_grad_(True)
    with torch.enable_grad():
        out = forward(kpts, scores)
        (out * dy).sum().backward()
    res = {"out": out.detach(), "dkpts": kpts.grad, "dscores": scores.grad}
    res.update({name: p.grad.clone() for name, p in module.named_parameters()})
    return res


def bn_outputs(module, run):
    """run() with a hook on every BatchNorm1d of module -> the list of their outputs (the pre-activations of the ReLUs), detached"""
    seen, hooks = [], []
    for m in module.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            hooks.append(m.register_forward_hook(lambda _m, _i, o: seen.append(o.detach())))
    try:
        run()
    finally:
        for h in hooks:
            h.remove()
    return seen
