"""The project's own statement of what the kernels of csrc/mha_train.hip compute: the attention of SuperGlue's GNN
(superglue/models/superglue_train.py:82-86) and its derivative with respect to query, key and value, as the closed forms of DESIGN.md
section 14 written out in torch on the CPU (float64 or fp32) -- no autograd in forward() / backward(); autograd() differentiates the
same written forward with torch.autograd for the cross-check.  Held to the fixtures the reference's own autograd wrote
(tests/golden/make_golden_mhagrad.py) by tests/test_mhagrad_host.py; the kernels are held to it and to those fixtures by
tests/test_gpu_mhagrad.py.  No bits are claimed between this file and the kernels: the fp32 mode runs torch's summation orders, the
kernels their own (fixed) ones.

Tensors are the reference's: q (B,D,H,N), k and v (B,D,H,M); lse (B,H,N).  nq / nk (B) counts or None: queries past nq[b] and keys past
nk[b] are never read (they may hold NaN) and every output is 0 there."""
import numpy as np
import torch

from image_matching_amd import synth
from tests.otgrad_ref import bar  # noqa: F401  (the default bar, element-wise: max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|))


# ---------------------------------------------------------------------------------------------- seeded cases
def heavy(seed, name, shape):
    """a normal times exp(0.5 normal): heavy-tailed, fp32; integer hashing only (image_matching_amd.synth), the same bits everywhere"""
    n = int(np.prod(shape))
    g = synth.normal(seed, name, n).astype(np.float64)
    t = synth.normal(seed, name + ".tail", n).astype(np.float64)
    return (g * np.exp(0.5 * t)).reshape(shape).astype(np.float32)


def case(seed, B, D, H, N, M, gain=1.0):
    """q (B,D,H,N), k, v (B,D,H,M), dout (B,D,H,N) fp32; q and k multiplied by the logit gain (the logits scale with its square)"""
    q = heavy(seed, "mha.q", (B, D, H, N)) * np.float32(gain)
    k = heavy(seed, "mha.k", (B, D, H, M)) * np.float32(gain)
    return q, k, heavy(seed, "mha.v", (B, D, H, M)), heavy(seed, "mha.dout", (B, D, H, N))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _counts(c, B, cap):
    return [cap] * B if c is None else [min(max(int(x), 0), cap) for x in np.asarray(c).reshape(-1)]


# ---------------------------------------------------------------------------------------------- the closed forms
def forward(q, k, v, nq=None, nk=None, dtype=torch.float64):
    """-> out (B,D,H,N), lse (B,H,N), float64 arrays whatever the dtype of the arithmetic"""
    q, k, v = _t(q, dtype), _t(k, dtype), _t(v, dtype)
    B, D, H, N = q.shape
    M = k.shape[3]
    out, lse = torch.zeros(B, D, H, N, dtype=dtype), torch.zeros(B, H, N, dtype=dtype)
    for b, (n, m) in enumerate(zip(_counts(nq, B, N), _counts(nk, B, M))):
        if n == 0 or m == 0:
            continue
        S = torch.einsum("dhn,dhm->hnm", q[b, :, :, :n], k[b, :, :, :m]) / D ** .5
        l = torch.logsumexp(S, -1)
        out[b, :, :, :n] = torch.einsum("hnm,dhm->dhn", torch.exp(S - l[..., None]), v[b, :, :, :m])
        lse[b, :, :n] = l
    return out.double().numpy(), lse.double().numpy()


def backward(q, k, v, dout, nq=None, nk=None, dtype=torch.float64):
    """-> dq (B,D,H,N), dk, dv (B,D,H,M): delta, P = exp(S - lse), dV = P^T dO, dP = dO V^T, dS = P o (dP - delta) scale, dQ = dS K,
    dK = dS^T Q; the forward's out and lse are recomputed here in the same dtype"""
    q, k, v, g = _t(q, dtype), _t(k, dtype), _t(v, dtype), _t(dout, dtype)
    B, D, H, N = q.shape
    M = k.shape[3]
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    scale = 1.0 / D ** .5
    for b, (n, m) in enumerate(zip(_counts(nq, B, N), _counts(nk, B, M))):
        if n == 0 or m == 0:
            continue
        qb, kb, vb, gb = q[b, :, :, :n], k[b, :, :, :m], v[b, :, :, :m], g[b, :, :, :n]
        S = torch.einsum("dhn,dhm->hnm", qb, kb) * scale
        P = torch.exp(S - torch.logsumexp(S, -1)[..., None])
        O = torch.einsum("hnm,dhm->dhn", P, vb)
        delta = (gb * O).sum(0)                                            # (H, n)
        dv[b, :, :, :m] = torch.einsum("hnm,dhn->dhm", P, gb)
        dP = torch.einsum("dhn,dhm->hnm", gb, vb)
        dS = P * (dP - delta[..., None]) * scale
        dq[b, :, :, :n] = torch.einsum("hnm,dhm->dhn", dS, kb)
        dk[b, :, :, :m] = torch.einsum("hnm,dhn->dhm", dS, qb)
    return dq.double().numpy(), dk.double().numpy(), dv.double().numpy()


def attention_einsum(query, key, value):
    """the written forward, as superglue_train.py:82-86 has it (restated; tests and tools differentiate it with torch.autograd)"""
    dim = query.shape[1]
    scores = torch.einsum("bdhn,bdhm->bhnm", query, key) / dim ** .5
    prob = torch.nn.functional.softmax(scores, dim=-1)
    return torch.einsum("bhnm,bdhm->bdhn", prob, value), prob


def autograd(q, k, v, dout, dtype=torch.float64, fn=attention_einsum):
    """the written forward differentiated by torch.autograd on full (unpadded) tensors -> out, dq, dk, dv as float64 arrays"""
    with torch.enable_grad():
        q, k, v = (_t(a, dtype).requires_grad_(True) for a in (q, k, v))
        out = fn(q, k, v)[0]
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), _t(dout, dtype))
    return tuple(a.detach().double().numpy() for a in (out, dq, dk, dv))


def batch_reference(q, k, v, dout, nq=None, nk=None, dtype=torch.float64):
    """everything the two entry points write, as a dict of float64 arrays"""
    out, lse = forward(q, k, v, nq, nk, dtype)
    dq, dk, dv = backward(q, k, v, dout, nq, nk, dtype)
    return {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
