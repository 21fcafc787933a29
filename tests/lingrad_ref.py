"""The project's own statement of what the kernels of csrc/lin_train.hip compute: nn.Conv1d(kernel_size=1) on torch.cat([x0, x1], 1)
(superglue/models/superglue_train.py:52, 96, 97, 111) and its derivative with respect to both inputs, the weight and the bias, as the
closed forms of DESIGN.md section 15 written out in torch on the CPU (float64 or fp32) -- no autograd in forward() / backward();
autograd() differentiates the same written forward with torch.autograd for the cross-check.  Held to the fixtures the reference's own
MLP wrote under torch.autograd (tests/golden/make_golden_lingrad.py) by tests/test_lingrad_host.py; the kernels are held to it and to
those fixtures by tests/test_gpu_lingrad.py.  No bits are claimed between this file and the kernels: the fp32 mode runs torch's
summation orders, the kernels their own (fixed) ones.

Tensors are the reference's: x0 (B,C0,N), x1 (B,C1,N) or None, w (Cout,C0+C1), bias (Cout) or None, y and dy (B,Cout,N).  n (B) counts or
None: columns past n[b] are never read (they may hold NaN), y and dx are 0 there, and they add nothing to dw and db."""
import numpy as np
import torch

from tests.mhagrad_ref import heavy
from tests.otgrad_ref import bar  # noqa: F401  (the default bar, element-wise: max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|))


# ---------------------------------------------------------------------------------------------- seeded cases
def case(seed, B, Cout, C0, C1, N, wseed=None):
    """x0 (B,C0,N), x1 (B,C1,N) or None, w (Cout,C0+C1), bias (Cout), dy (B,Cout,N) fp32: heavy-tailed activations and cotangent, weights
    heavy / sqrt(C0+C1), bias 0.1 heavy; wseed: another seed for w and bias (the items of one batch share their weights)"""
    x0 = heavy(seed, "lin.x0", (B, C0, N))
    x1 = heavy(seed, "lin.x1", (B, C1, N)) if C1 else None
    wseed = seed if wseed is None else wseed
    w = (heavy(wseed, "lin.w", (Cout, C0 + C1)).astype(np.float64) / np.sqrt(C0 + C1)).astype(np.float32)
    bias = (0.1 * heavy(wseed, "lin.bias", (Cout,)).astype(np.float64)).astype(np.float32)
    return x0, x1, w, bias, heavy(seed, "lin.dy", (B, Cout, N))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _counts(c, B, cap):
    return [cap] * B if c is None else [min(max(int(x), 0), cap) for x in np.asarray(c).reshape(-1)]


def _cat(x0, x1, dtype):
    return _t(x0, dtype) if x1 is None else torch.cat([_t(x0, dtype), _t(x1, dtype)], 1)


# ---------------------------------------------------------------------------------------------- the closed forms
def forward(x0, x1, w, bias=None, n=None, dtype=torch.float64):
    """-> y (B,Cout,N), a float64 array whatever the dtype of the arithmetic"""
    x, w = _cat(x0, x1, dtype), _t(w, dtype).reshape(np.shape(w)[0], -1)
    B, _, N = x.shape
    y = torch.zeros(B, w.shape[0], N, dtype=dtype)
    for b, cnt in enumerate(_counts(n, B, N)):
        if cnt:
            y[b, :, :cnt] = w @ x[b, :, :cnt]
            if bias is not None:
                y[b, :, :cnt] += _t(bias, dtype)[:, None]
    return y.double().numpy()


def backward(x0, x1, w, dy, n=None, dtype=torch.float64):
    """-> dx (B,C0+C1,N) (the caller splits it at C0), dw (Cout,C0+C1), db (Cout): dx = w^T dy, dw = sum_b dy x^T, db = sum_b sum_n dy,
    each pair's part formed on its valid columns only and the pairs added in ascending order"""
    x, w, g = _cat(x0, x1, dtype), _t(w, dtype).reshape(np.shape(w)[0], -1), _t(dy, dtype)
    B, _, N = x.shape
    dx, dw, db = torch.zeros_like(x), torch.zeros_like(w), torch.zeros(w.shape[0], dtype=dtype)
    for b, cnt in enumerate(_counts(n, B, N)):
        if cnt:
            dx[b, :, :cnt] = w.t() @ g[b, :, :cnt]
            dw += g[b, :, :cnt] @ x[b, :, :cnt].t()
            db += g[b, :, :cnt].sum(1)
    return dx.double().numpy(), dw.double().numpy(), db.double().numpy()


def conv1d_cat(x0, x1, w, bias):
    """the written forward, as the reference's modules have it (restated; tests and tools differentiate it with torch.autograd)"""
    x = x0 if x1 is None else torch.cat([x0, x1], 1)
    return torch.nn.functional.conv1d(x, w.reshape(w.shape[0], -1, 1), bias)


def autograd(x0, x1, w, bias, dy, dtype=torch.float64, fn=conv1d_cat):
    """the written forward differentiated by torch.autograd on full (unpadded) tensors -> dict of float64 arrays: y, dx (both sources,
    concatenated), dw, db"""
    with torch.enable_grad():
        leaves = [None if a is None else _t(a, dtype).requires_grad_(True) for a in (x0, x1, w, bias)]
        y = fn(*leaves)
        grads = torch.autograd.grad(y, [t for t in leaves if t is not None], _t(dy, dtype))
    it = iter(grads)
    g0, g1, gw, gb = (None if t is None else next(it).detach().double().numpy() for t in leaves)
    return {"y": y.detach().double().numpy(), "dx": g0 if g1 is None else np.concatenate([g0, g1], 1), "dw": gw, "db": gb}


def batch_reference(x0, x1, w, bias, dy, n=None, dtype=torch.float64):
    """everything the two entry points write, as a dict of float64 arrays (dx over the concatenated channels)"""
    dx, dw, db = backward(x0, x1, w, dy, n, dtype)
    return {"y": forward(x0, x1, w, bias, n, dtype), "dx": dx, "dw": dw, "db": db}


# ---------------------------------------------------------------------------------------------- one layer of the GNN, restated
class MultiHeadedAttention(torch.nn.Module):
    """superglue_train.py:89-104 restated (the three projections are modules of their own, as deepcopy leaves them)"""

    def __init__(self, num_heads, d_model):
        super().__init__()
        self.dim, self.num_heads = d_model // num_heads, num_heads
        self.merge = torch.nn.Conv1d(d_model, d_model, kernel_size=1)
        self.proj = torch.nn.ModuleList([torch.nn.Conv1d(d_model, d_model, kernel_size=1) for _ in range(3)])

    def forward(self, query, key, value):
        b = query.size(0)
        query, key, value = [l(x).view(b, self.dim, self.num_heads, -1) for l, x in zip(self.proj, (query, key, value))]
        scores = torch.einsum("bdhn,bdhm->bhnm", query, key) / self.dim ** .5
        x = torch.einsum("bhnm,bdhm->bdhn", torch.nn.functional.softmax(scores, dim=-1), value)
        return self.merge(x.contiguous().view(b, self.dim * self.num_heads, -1))


class AttentionalPropagation(torch.nn.Module):
    """superglue_train.py:107-116 restated: attention, then Conv1d, BatchNorm1d, ReLU, Conv1d on torch.cat([x, message], 1)"""

    def __init__(self, feature_dim, num_heads):
        super().__init__()
        self.attn = MultiHeadedAttention(num_heads, feature_dim)
        self.mlp = torch.nn.Sequential(torch.nn.Conv1d(2 * feature_dim, 2 * feature_dim, kernel_size=1), torch.nn.BatchNorm1d(2 * feature_dim),
                                       torch.nn.ReLU(), torch.nn.Conv1d(2 * feature_dim, feature_dim, kernel_size=1))

    def forward(self, x, source):
        return self.mlp(torch.cat([x, self.attn(x, source, source)], dim=1))


def layer_parameters(seed, module):
    """seeded values for the 14 parameters of an AttentionalPropagation (the reference's or the restated one: the names agree), name ->
    fp32 array: convolution weights heavy / sqrt(fan-in), biases 0.1 heavy, BatchNorm weight 1 + 0.1 heavy"""
    out = {}
    for name, p in module.named_parameters():
        h = heavy(seed, "layer." + name, tuple(p.shape)).astype(np.float64)
        if p.dim() == 3:
            h = h / np.sqrt(p.shape[1])
        else:
            h = 0.1 * h + (1.0 if name == "mlp.1.weight" else 0.0)
        out[name] = h.astype(np.float32)
    return out


def layer_case(seed, d, N, M):
    """x (1,d,N), source (1,d,M), dy (1,d,N) fp32"""
    return heavy(seed, "layer.x", (1, d, N)), heavy(seed, "layer.source", (1, d, M)), heavy(seed, "layer.dy", (1, d, N))


def layer_grads(module, forward, x, source, dy):
    """out = forward(x, source) on leaves, the gradients of sum(out * dy) -> dict name -> tensor: out, dx, dsource and one per parameter"""
    module.zero_grad()
    x, source = x.clone().requires_grad_(True), source.clone().requires_grad_(True)
    with torch.enable_grad():
        out = forward(x, source)
        (out * dy).sum().backward()
    res = {"out": out.detach(), "dx": x.grad, "dsource": source.grad}
    res.update({name: p.grad.clone() for name, p in module.named_parameters()})
    return res
