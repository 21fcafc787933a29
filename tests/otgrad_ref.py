"""The project's own statement of what the kernels of csrc/otgrad.hip compute: the SuperGlue match loss
(superglue/models/superglue_train.py:267-299) through the unrolled log-domain Sinkhorn, its value and its derivative with respect to
the score matrix and bin_score, as the recursion of DESIGN.md section 13 written out in torch on the CPU (float64 or fp32) -- no
autograd in loss_grad(); loss_autograd() differentiates the same written loss with torch.autograd for the cross-check.  Held to the
fixtures the reference's own autograd wrote (tests/golden/make_golden_otgrad.py) by tests/test_otgrad_host.py; the kernels are held to
it and to those fixtures by tests/test_gpu_otgrad.py.  No bits are claimed between this file and the kernels: the fp32 mode runs torch's
summation orders, the kernels their own (fixed) ones."""
import numpy as np
import torch

from image_matching_amd import synth

FLAG_INDEX = 1


def bar(g64, ref32_minus_64=None):
    """the default bar, element-wise: max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|)"""
    b = 1e-4 + 1e-4 * np.abs(np.asarray(g64, np.float64))
    return b if ref32_minus_64 is None else np.maximum(b, 2.5 * np.abs(np.asarray(ref32_minus_64, np.float64)))


# ---------------------------------------------------------------------------------------------- seeded cases
def case_scores(seed, m, n, planted=None):
    """(scores (m,n) fp32, matches (2,L) int64): heavy-tailed scores of standard deviation about 5 (a normal times a log-normal, the
    statistics of the 't' weight set's score matrices) with `planted` correspondences raised by 15, and the list imx_gt_matches would
    write for them: the planted pairs, then every unmatched row against the dustbin column n, then every unmatched column against the
    dustbin row m.  Integer hashing only (image_matching_amd.synth), so the same seed gives the same bits everywhere."""
    g = synth.normal(seed, "otg.scores", m * n).astype(np.float64)
    tail = synth.normal(seed, "otg.tail", m * n).astype(np.float64)
    s = (3.9 * g * np.exp(0.5 * tail)).reshape(m, n)
    k = min(m, n) // 2 if planted is None else planted
    rows = np.argsort(synth.uniform(seed, "otg.rows", m), kind="stable")[:k]
    cols = np.argsort(synth.uniform(seed, "otg.cols", n), kind="stable")[:k]
    s[rows, cols] += 15.0
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    free_r = np.setdiff1d(np.arange(m), rows)
    free_c = np.setdiff1d(np.arange(n), cols)
    xs = np.concatenate([rows, free_r, np.full(len(free_c), m)])
    ys = np.concatenate([cols, np.full(len(free_r), n), free_c])
    return s.astype(np.float32), np.stack([xs, ys]).astype(np.int64)


# ---------------------------------------------------------------------------------------------- the recursion
def potentials(C, log_mu, log_nu, iters):
    """[u_0 .. u_T], [v_0 .. v_T] of the log-domain Sinkhorn on the coupling matrix C"""
    u, v = [torch.zeros_like(log_mu)], [torch.zeros_like(log_nu)]
    for _ in range(iters):
        u.append(log_mu - torch.logsumexp(C + v[-1][None, :], 1))
        v.append(log_nu - torch.logsumexp(C + u[-1][:, None], 0))
    return u, v


def coupling(scores, bin_score, dtype):
    S = torch.as_tensor(np.asarray(scores)).to(dtype)
    m, n = S.shape
    C = torch.full((m + 1, n + 1), float(bin_score), dtype=dtype)
    C[:m, :n] = S
    norm = -torch.tensor(float(m + n), dtype=dtype).log()
    log_mu = torch.cat([norm.expand(m), torch.tensor(float(n), dtype=dtype).log()[None] + norm])
    log_nu = torch.cat([norm.expand(n), torch.tensor(float(m), dtype=dtype).log()[None] + norm])
    return C, log_mu, log_nu, norm


def loss_grad(scores, bin_score, matches, iters, gout=1.0, dtype=torch.float64):
    """One pair: scores (m,n), matches (2,K) listed (x, y).  -> (loss, d scores (m,n), d bin_score, flag), float64 arrays whatever the
    dtype of the arithmetic.  A listed index outside [0,m] x [0,n] is flagged and contributes nothing (K still counts it); K = 0 gives
    0.  Where exp(Z) underflows the value is +inf and the derivative is that of -Z (the recursion never forms the exp of Z)."""
    C, log_mu, log_nu, norm = coupling(scores, bin_score, dtype)
    m, n = C.shape[0] - 1, C.shape[1] - 1
    xs, ys = (np.asarray(v, np.int64) for v in matches)
    K = len(xs)
    ok = (xs >= 0) & (xs <= m) & (ys >= 0) & (ys <= n)
    flag = 0 if ok.all() else FLAG_INDEX
    xs, ys = torch.from_numpy(xs[ok]), torch.from_numpy(ys[ok])
    u, v = potentials(C, log_mu, log_nu, iters)
    if K == 0:
        return 0.0, np.zeros((m, n)), 0.0, flag
    Z = C + u[-1][:, None] + v[-1][None, :] - norm
    loss = float((-torch.log(torch.exp(Z[xs, ys]))).sum() / K)
    w = torch.tensor(float(gout), dtype=dtype) / K
    G = torch.zeros_like(C)
    G.index_put_((xs, ys), -w.expand(len(xs)), accumulate=True)          # once per listing
    ub, vb, Cb = G.sum(1), G.sum(0), G.clone()
    for t in range(iters, 0, -1):
        Pc = torch.exp(C + u[t][:, None] + v[t][None, :] - log_nu[None, :])
        Cb = Cb - vb[None, :] * Pc
        ub = ub - Pc @ vb
        Pr = torch.exp(C + u[t][:, None] + v[t - 1][None, :] - log_mu[:, None])
        Cb = Cb - ub[:, None] * Pr
        vb = -(Pr.T @ ub)
        ub = torch.zeros_like(ub)
    gbin = Cb[m, :].sum() + Cb[:m, n].sum()
    return loss, Cb[:m, :n].double().numpy(), float(gbin), flag


def loss_autograd(scores, bin_score, matches, iters, dtype=torch.float64):
    """the same written loss differentiated by torch.autograd -> (loss, d scores, d bin_score); NaN where an exp underflows"""
    with torch.enable_grad():
        S = torch.as_tensor(np.asarray(scores)).to(dtype).requires_grad_(True)
        a = torch.tensor(float(bin_score), dtype=dtype, requires_grad=True)
        m, n = S.shape
        C = torch.cat([torch.cat([S, a.expand(m, 1)], 1), a.expand(1, n + 1)], 0)
        _, log_mu, log_nu, norm = coupling(S.detach(), bin_score, dtype)
        u, v = potentials(C, log_mu, log_nu, iters)
        Z = C + u[-1][:, None] + v[-1][None, :] - norm
        xs, ys = (torch.from_numpy(np.asarray(q, np.int64)) for q in matches)
        loss = (-torch.log(torch.exp(Z[xs, ys]))).mean()
        gs, ga = torch.autograd.grad(loss, (S, a))
    return float(loss.detach()), gs.double().numpy(), float(ga)


def batch_loss_grad(scores, bin_score, all_matches, n_all, iters, n0=None, n1=None, gout=None, dtype=torch.float64):
    """A padded batch as the entry point takes it: scores (B,N0,N1) (rows past n0[b] and columns past n1[b] never read), all_matches
    (B,2,L), n_all (B).  -> loss (B), grad_scores (B,N0,N1) with 0 on the padding, grad_bin (B), flag (B)."""
    scores = np.asarray(scores)
    B, N0, N1 = scores.shape
    loss, gbin, flag = np.zeros(B), np.zeros(B), np.zeros(B, np.int32)
    grad = np.zeros((B, N0, N1))
    for b in range(B):
        m = N0 if n0 is None else int(n0[b])
        n = N1 if n1 is None else int(n1[b])
        K = int(n_all[b])
        if m == 0 or n == 0 or K == 0:
            continue
        go = 1.0 if gout is None else float(gout[b])
        loss[b], grad[b, :m, :n], gbin[b], flag[b] = loss_grad(scores[b, :m, :n], bin_score, np.asarray(all_matches)[b][:, :K], iters, go, dtype)
    return loss, grad, gbin, flag
