"""The project's own statement of what the kernels of csrc/score_train.hip compute: the score product of SuperGlue's training step,
torch.einsum('bdn,bdm->bnm', mdesc0, mdesc1) / descriptor_dim ** .5 (superglue/models/superglue_train.py:267-268), and its derivative
with respect to both inputs, as the three closed forms of DESIGN.md section 17 written out in numpy float64 -- no autograd in
forward() / backward(); autograd() differentiates the written einsum with torch.autograd (float64 or fp32, on the CPU) for the
cross-check and for the second term of the default bar.  Held to torch's einsum and autograd by tests/test_scoregrad_host.py; the
kernels are held to it by tests/test_gpu_scoregrad.py.  No bits are claimed between this file and the kernels: torch runs its own
summation orders, the kernels their own (fixed) ones.

The second half restates the reference's training SuperGlue (superglue_train.py:174-307) in PyTorch, composed from the restated layers of
tests/lingrad_ref.py (AttentionalPropagation) and tests/bngrad_ref.py (KeypointEncoder), with seeded parameters and a seeded sample
(model_parameters, model_case): held to the fixture the reference's own model wrote (tests/golden/make_golden_sgmodel.py) by
tests/test_scoregrad_host.py; image_matching_amd.sgtrain_model.SuperGlueTrainable is held to that fixture and to this restatement by
tests/test_gpu_sgmodel.py.

Tensors are the reference's: a (B,D,N0), b (B,D,N1), scores and dscores (B,N0,N1).  n0 / n1 (B) counts or None: columns of a past
n0[b], columns of b past n1[b] and dscores outside [0,n0) x [0,n1) are never read (they may hold NaN), and every output is 0 there."""
import numpy as np
import torch

from image_matching_amd import synth
from tests import bngrad_ref, lingrad_ref
from tests.mhagrad_ref import heavy
from tests.otgrad_ref import bar  # noqa: F401  (the default bar, element-wise: max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|))


# ---------------------------------------------------------------------------------------------- seeded cases
def case(seed, B, D, N0, N1):
    """a (B,D,N0), b (B,D,N1), dscores (B,N0,N1) fp32, heavy-tailed: integer hashing only, the same bits everywhere"""
    return heavy(seed, "score.a", (B, D, N0)), heavy(seed, "score.b", (B, D, N1)), heavy(seed, "score.ds", (B, N0, N1))


def _counts(c, B, cap):
    return [cap] * B if c is None else [min(max(int(x), 0), cap) for x in np.asarray(c).reshape(-1)]


def default_scale(D):
    return float(D) ** -0.5


def ragged_pad(t, counts, frame, axes, fill=np.nan):
    """t (B, ..., n_i, ...) -> the same over `frame` on each of `axes`, `fill` past counts[k][b] on axes[k]"""
    shape = list(t.shape)
    for ax, fr in zip(axes, frame):
        shape[ax] = fr
    out = np.full(shape, fill, t.dtype)
    for b in range(t.shape[0]):
        idx = [b] + [slice(None)] * (t.ndim - 1)
        for ax, cnt in zip(axes, counts):
            idx[ax] = slice(0, int(cnt[b]))
        out[tuple(idx)] = t[tuple(idx)]
    return out


# ---------------------------------------------------------------------------------------------- the closed forms
def forward(a, b, n0=None, n1=None, scale=None):
    """-> scores (B,N0,N1) float64: S[n][m] = scale sum_d A[d][n] Bm[d][m] on the valid block, 0 elsewhere"""
    B, D, N0 = a.shape
    N1 = b.shape[2]
    scale = default_scale(D) if scale is None else float(scale)
    s = np.zeros((B, N0, N1), np.float64)
    for p, (c0, c1) in enumerate(zip(_counts(n0, B, N0), _counts(n1, B, N1))):
        if c0 and c1:
            s[p, :c0, :c1] = scale * (a[p, :, :c0].astype(np.float64).T @ b[p, :, :c1].astype(np.float64))
    return s


def backward(a, b, ds, n0=None, n1=None, scale=None):
    """-> da (B,D,N0), db (B,D,N1) float64: dA[d][n] = scale sum_m dS[n][m] Bm[d][m], dBm[d][m] = scale sum_n dS[n][m] A[d][n], the sums
    over the valid block only, 0 past the counts"""
    B, D, N0 = a.shape
    N1 = b.shape[2]
    scale = default_scale(D) if scale is None else float(scale)
    da, db = np.zeros((B, D, N0), np.float64), np.zeros((B, D, N1), np.float64)
    for p, (c0, c1) in enumerate(zip(_counts(n0, B, N0), _counts(n1, B, N1))):
        if c0 and c1:
            g = ds[p, :c0, :c1].astype(np.float64)
            da[p, :, :c0] = scale * (b[p, :, :c1].astype(np.float64) @ g.T)
            db[p, :, :c1] = scale * (a[p, :, :c0].astype(np.float64) @ g)
    return da, db


def batch_reference(a, b, ds, n0=None, n1=None, scale=None):
    """everything the two entry points write, as a dict of float64 arrays"""
    da, db = backward(a, b, ds, n0, n1, scale)
    return {"scores": forward(a, b, n0, n1, scale), "da": da, "db": db}


def score_einsum(mdesc0, mdesc1, scale=None):
    """the written forward, as the reference has it (restated; tests differentiate it with torch.autograd)"""
    s = torch.einsum("bdn,bdm->bnm", mdesc0, mdesc1)
    return s / mdesc0.shape[1] ** .5 if scale is None else s * scale


def autograd(a, b, ds, dtype=torch.float64, scale=None):
    """the written forward differentiated by torch.autograd on full (unpadded) tensors on the CPU -> dict of float64 arrays"""
    with torch.enable_grad():
        ta, tb = (torch.as_tensor(np.asarray(t)).to(dtype).requires_grad_(True) for t in (a, b))
        s = score_einsum(ta, tb, scale)
        ga, gb = torch.autograd.grad(s, [ta, tb], torch.as_tensor(np.asarray(ds)).to(dtype))
    return {"scores": s.detach().double().numpy(), "da": ga.double().numpy(), "db": gb.double().numpy()}


def ragged_autograd(a, b, ds, n0, n1, dtype=torch.float64, scale=None):
    """autograd() pair by pair on each pair's valid block, written into zero frames -> dict of float64 arrays"""
    B, D, N0 = a.shape
    N1 = b.shape[2]
    out = {"scores": np.zeros((B, N0, N1)), "da": np.zeros((B, D, N0)), "db": np.zeros((B, D, N1))}
    for p, (c0, c1) in enumerate(zip(_counts(n0, B, N0), _counts(n1, B, N1))):
        if c0 and c1:
            r = autograd(a[p:p + 1, :, :c0], b[p:p + 1, :, :c1], ds[p:p + 1, :c0, :c1], dtype, scale)
            out["scores"][p, :c0, :c1], out["da"][p, :, :c0], out["db"][p, :, :c1] = r["scores"][0], r["da"][0], r["db"][0]
    return out


# ---------------------------------------------------------------------------------------------- the training model, restated
MODEL_CONFIG = {"descriptor_dim": 64, "keypoint_encoder": [32, 64], "GNN_layers": ["self", "cross"], "sinkhorn_iterations": 20,
                "match_threshold": 0.2, "weights": ""}
MODEL_SAMPLE = {"N0": 48, "N1": 40, "H": 120, "W": 160, "planted": 30}
KINK = bngrad_ref.KINK


def transport(scores, bin_score, iters):
    """scores (m,n) -> Z (m+1,n+1): the log-domain Sinkhorn of superglue_train.py:138-167 on the score matrix bordered by bin_score, the
    marginals those of m + n points of which the dustbins take n and m; multiplied by m + n at the end"""
    m, n = scores.shape
    alpha = bin_score.reshape(1, 1).to(scores)
    C = torch.cat([torch.cat([scores, alpha.expand(m, 1)], 1), alpha.expand(1, n + 1)], 0)
    norm = -np.log(m + n)
    log_mu = torch.cat([scores.new_full((m,), norm), scores.new_full((1,), np.log(n) + norm)])
    log_nu = torch.cat([scores.new_full((n,), norm), scores.new_full((1,), np.log(m) + norm)])
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(C + v[None, :], 1)
        v = log_nu - torch.logsumexp(C + u[:, None], 0)
    return C + u[:, None] + v[None, :] - norm


def matches_of(Z, threshold):
    """Z (m+1,n+1) -> (matches0 (m), matches1 (n), matching_scores0, matching_scores1): mutual row / column maxima of the inner block whose
    exp exceeds the threshold, -1 elsewhere (superglue_train.py:276-286)"""
    inner = Z[:-1, :-1]
    v0, i0 = inner.max(1)
    _, i1 = inner.max(0)
    mutual0 = torch.arange(len(i0)) == i1[i0]
    mutual1 = torch.arange(len(i1)) == i0[i1]
    ms0 = torch.where(mutual0, v0.exp(), torch.zeros_like(v0))
    ms1 = torch.where(mutual1, ms0[i1], torch.zeros_like(ms0[i1]))
    valid0 = mutual0 & (ms0 > threshold)
    valid1 = mutual1 & valid0[i1]
    return torch.where(valid0, i0, torch.full_like(i0, -1)), torch.where(valid1, i1, torch.full_like(i1, -1)), ms0, ms1


def top_two_margins(Z):
    """the gap between the largest and the second largest entry of each row and each column of the inner block of Z -> (m), (n); a row or
    column of one entry has margin inf"""
    inner = Z[:-1, :-1]

    def gap(t, dim):
        if t.shape[dim] < 2:
            return torch.full((t.shape[1 - dim],), float("inf"), dtype=t.dtype)
        top = t.topk(2, dim).values
        return (top.select(dim, 0) - top.select(dim, 1))
    return gap(inner, 1), gap(inner, 0)


class _Layers(torch.nn.Module):
    def __init__(self, d, names):
        super().__init__()
        self.layers = torch.nn.ModuleList([lingrad_ref.AttentionalPropagation(d, 4) for _ in names])
        self.names = list(names)


class SuperGlue(torch.nn.Module):
    """The reference's training SuperGlue restated on a LIST of pairs.  Every module call of the reference (the keypoint encoder on side
    0, on side 1, each layer on side 0, on side 1, ...) runs per pair on that pair's own columns, except its BatchNorm, which sees the
    columns of all pairs concatenated -- the definition of a layer on a ragged batch (include/imx_train.h).  With one pair this is the
    reference's forward, module call by module call.  The parameter names are the reference's."""

    def __init__(self, config=None):
        super().__init__()
        self.config = {**MODEL_CONFIG, **(config or {})}
        d = self.config["descriptor_dim"]
        self.register_parameter("bin_score", torch.nn.Parameter(torch.tensor(1.)))
        self.kenc = bngrad_ref.KeypointEncoder(d, list(self.config["keypoint_encoder"]))
        self.gnn = _Layers(d, self.config["GNN_layers"])
        self.final_proj = torch.nn.Conv1d(d, d, kernel_size=1, bias=True)

    @staticmethod
    def _sequential(seq, xs):
        for m in seq:
            if isinstance(m, torch.nn.BatchNorm1d):
                xs = list(m(torch.cat(xs, 2)).split([x.shape[2] for x in xs], 2))
            else:
                xs = [m(x) for x in xs]
        return xs

    def _encode(self, kpts, scores, shapes):
        inputs = []
        for k, s, shape in zip(kpts, scores, shapes):
            size = k.new_tensor([float(shape[-1]), float(shape[-2])])
            k = (k - size / 2) / (size.max() * 0.7)
            inputs.append(torch.cat([k.transpose(1, 2), s.unsqueeze(1)], 1))
        return self._sequential(self.kenc.encoder, inputs)

    def _propagate(self, layer, xs, sources):
        return self._sequential(layer.mlp, [torch.cat([x, layer.attn(x, s, s)], 1) for x, s in zip(xs, sources)])

    def forward(self, pairs):
        """pairs: a list of dicts kpts0 (1,N0,2), scores0 (1,N0), desc0 (1,d,N0), the same of side 1, all_matches (2,L) int64, shape0,
        shape1 -> (losses: a list of 0-dim tensors, Zs: the list of (N0+1,N1+1) log-assignments)"""
        d0 = [p["desc0"] + e for p, e in zip(pairs, self._encode([p["kpts0"] for p in pairs], [p["scores0"] for p in pairs], [p["shape0"] for p in pairs]))]
        d1 = [p["desc1"] + e for p, e in zip(pairs, self._encode([p["kpts1"] for p in pairs], [p["scores1"] for p in pairs], [p["shape1"] for p in pairs]))]
        for layer, name in zip(self.gnn.layers, self.gnn.names):
            s0, s1 = (d1, d0) if name == "cross" else (d0, d1)
            delta0, delta1 = self._propagate(layer, d0, s0), self._propagate(layer, d1, s1)
            d0, d1 = [x + y for x, y in zip(d0, delta0)], [x + y for x, y in zip(d1, delta1)]
        losses, Zs = [], []
        for p, x0, x1 in zip(pairs, d0, d1):
            s = score_einsum(self.final_proj(x0), self.final_proj(x1), self.config["descriptor_dim"] ** -.5)
            Z = transport(s[0], self.bin_score, self.config["sinkhorn_iterations"])
            xs, ys = p["all_matches"][0], p["all_matches"][1]
            losses.append((-torch.log(torch.exp(Z[xs, ys]))).mean())
            Zs.append(Z)
        return losses, Zs


def model_parameters(seed, module):
    """seeded values for the 41 parameters of a training SuperGlue (the reference's, the restated one or SuperGlueTrainable: the names
    agree), name -> fp32 array: convolution weights 0.5 heavy / sqrt(fan-in) (the scale of PyTorch's default initialisation), biases
    0.1 heavy, BatchNorm weights 1 + 0.1 heavy, bin_score 1 + 0.1 heavy.  The buffers keep their initial values."""
    bn_weights = {name + ".weight" for name, m in module.named_modules() if isinstance(m, torch.nn.BatchNorm1d)}
    out = {}
    for name, p in module.named_parameters():
        h = heavy(seed, "model." + name, tuple(p.shape) or (1,)).astype(np.float64).reshape(tuple(p.shape))
        if p.dim() == 3:
            h = 0.5 * h / np.sqrt(p.shape[1])
        else:
            h = 0.1 * h + (1.0 if name in bn_weights or name == "bin_score" else 0.0)
        out[name] = np.asarray(h, np.float32)
    return out


def load_parameters(module, seed, dtype=torch.float32):
    """model_parameters(seed) into module (strict about the parameters, the buffers untouched) -> module.to(dtype)"""
    params = model_parameters(seed, module)
    assert set(params) == {n for n, _ in module.named_parameters()}
    missing = module.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    assert not missing.unexpected_keys and all(".running_" in k or k.endswith("num_batches_tracked") for k in missing.missing_keys)
    return module.to(dtype)


def model_case(seed, N0=MODEL_SAMPLE["N0"], N1=MODEL_SAMPLE["N1"], H=MODEL_SAMPLE["H"], W=MODEL_SAMPLE["W"], planted=MODEL_SAMPLE["planted"], d=64):
    """one sample as the reference's training loop hands it to the model, a dict of numpy arrays: descriptors{0,1} (d,1,N) unit columns,
    keypoints{0,1} (1,1,N,2) pixels in a W x H image, scores{0,1} (N,1) in (0,1), all_matches (2,1,L) int64 -- `planted` matches (row i
    against a hashed column, whose descriptor is the row's plus half as much noise), then every other row against the dustbin column
    N1, then every other column against the dustbin row N0 -- and image{0,1} (1,1,H,W) zeros (only their shape is read)"""
    unit = lambda a: a / np.linalg.norm(a, axis=0, keepdims=True)
    desc0 = unit(heavy(seed, "model.desc0", (d, N0)).astype(np.float64))
    desc1 = unit(heavy(seed, "model.desc1", (d, N1)).astype(np.float64))
    cols = np.argsort(synth.uniform(seed, "model.cols", N1), kind="stable")[:planted]
    rows = np.arange(planted)
    desc1[:, cols] = unit(desc0[:, rows] + 0.5 * unit(heavy(seed, "model.noise", (d, planted)).astype(np.float64)))
    wh = np.array([W, H], np.float64)
    kpts0 = synth.uniform(seed, "model.kpts0", 2 * N0).astype(np.float64).reshape(N0, 2) * wh
    kpts1 = synth.uniform(seed, "model.kpts1", 2 * N1).astype(np.float64).reshape(N1, 2) * wh
    free_r, free_c = np.setdiff1d(np.arange(N0), rows), np.setdiff1d(np.arange(N1), cols)
    xs = np.concatenate([rows, free_r, np.full(len(free_c), N0)])
    ys = np.concatenate([cols, np.full(len(free_r), N1), free_c])
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return {"descriptors0": f(desc0[:, None, :]), "descriptors1": f(desc1[:, None, :]), "keypoints0": f(kpts0[None, None]), "keypoints1": f(kpts1[None, None]),
            "scores0": f(synth.uniform(seed, "model.scores0", N0)[:, None]), "scores1": f(synth.uniform(seed, "model.scores1", N1)[:, None]),
            "all_matches": np.stack([xs, ys])[:, None, :].astype(np.int64), "image0": np.zeros((1, 1, H, W), np.float32),
            "image1": np.zeros((1, 1, H, W), np.float32)}


def as_pair(sample, dtype=torch.float64):
    """a sample of model_case (numpy or torch) -> the dict SuperGlue.forward takes, floating tensors in dtype"""
    t = lambda a: torch.as_tensor(a)
    return {"kpts0": t(sample["keypoints0"]).reshape(1, -1, 2).to(dtype), "kpts1": t(sample["keypoints1"]).reshape(1, -1, 2).to(dtype),
            "scores0": t(sample["scores0"]).transpose(0, 1).to(dtype), "scores1": t(sample["scores1"]).transpose(0, 1).to(dtype),
            "desc0": t(sample["descriptors0"]).transpose(0, 1).to(dtype), "desc1": t(sample["descriptors1"]).transpose(0, 1).to(dtype),
            "all_matches": t(sample["all_matches"])[:, 0, :], "shape0": tuple(sample["image0"].shape), "shape1": tuple(sample["image1"].shape)}


def model_step(module, pairs):
    """zero_grad, the mean of the pairs' losses, backward -> (losses (P) float64 array, {name: gradient as a float64 array}, Zs)"""
    module.zero_grad()
    with torch.enable_grad():
        losses, Zs = module(pairs)
        torch.stack(losses).mean().backward()
    grads = {n: p.grad.detach().cpu().double().numpy().copy() for n, p in module.named_parameters()}
    return np.array([l.item() for l in losses]), grads, [Z.detach().cpu() for Z in Zs]


def model_buffers(module):
    """name -> float64 array of every BatchNorm buffer"""
    return {n: b.detach().cpu().double().numpy().copy() for n, b in module.named_buffers()}


def adam_losses(module, pairs, steps, lr):
    """the loss before each of `steps` consecutive torch.optim.Adam steps on the same pairs -> (steps) float64 array"""
    opt, out = torch.optim.Adam(module.parameters(), lr=lr), []
    for _ in range(steps):
        with torch.enable_grad():
            losses, _ = module(pairs)
            loss = torch.stack(losses).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        out.append(loss.item())
    return np.array(out)
