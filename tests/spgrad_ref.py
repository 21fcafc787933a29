"""The project's own statement of what the gradient kernels (csrc/spgrad.hip) compute: the two SuperPoint training losses as
differentiable torch functions in a chosen dtype, differentiated by torch.autograd.grad.  The detector loss in its conditioned form
(the arithmetic rule of imx_detector_loss, whose derivative the library returns) and in its written form (softmax, then BCELoss);
the descriptor loss as tests/sptrain_ref.py: desc_loss states it, kept as tensors.  Held to the fixtures the reference's own autograd
wrote (tests/golden/make_golden_spgrad.py) by tests/test_spgrad_host.py; the kernels are held to it and to those fixtures by
tests/test_gpu_spgrad.py."""
import numpy as np
import torch

from tests import sptrain_ref as R


def bar(g64, ref32_minus_64=None):
    """the default bar, element-wise: max(1e-4 + 1e-4 |g64|, 2.5 |ref32 - g64|)"""
    b = 1e-4 + 1e-4 * np.abs(np.asarray(g64, np.float64))
    return b if ref32_minus_64 is None else np.maximum(b, 2.5 * np.abs(np.asarray(ref32_minus_64, np.float64)))


def detector_loss_t(x, labels, mask, conditioned=True):
    """detector_loss(loss_type='softmax') (Train_model_heatmap.py:72-81) on the tensor x (B,65,Hc,Wc), in x's dtype, as a tensor"""
    dtype = x.dtype
    t, m = R.cell_targets(labels, dtype).to(x.device), R.cell_masks(mask, dtype).to(x.device)
    if conditioned:
        mx = x.max(1, keepdim=True).values.detach()
        e = torch.exp(x - mx)
        S = e.sum(1, keepdim=True)
        nlp = torch.clamp((mx - x) + torch.log(S), max=100)
        others = torch.stack([e[:, [k for k in range(65) if k != c]].sum(1) for c in range(65)], 1)
        nl1p = torch.clamp(torch.log(S) - torch.log(others), min=0, max=100)
    else:
        p = torch.softmax(x, 1)
        nlp, nl1p = -torch.clamp(torch.log(p), min=-100), -torch.clamp(torch.log(1 - p), min=-100)
    cell = (t * nlp + (1 - t) * nl1p).sum(1)
    return (cell * m).sum() / (m.sum() + 1e-10)


def detector_grad(semi, labels, mask, dtype=torch.float64, conditioned=True, gout=1.0):
    """-> (loss, d loss / d semi as a float64 array)"""
    with torch.enable_grad():                                            # (whatever an imported module left as the global mode)
        x = torch.as_tensor(np.asarray(semi)).to(dtype).requires_grad_(True)
        loss = detector_loss_t(x, labels, mask, conditioned)
        (g,) = torch.autograd.grad(loss * gout, x)
    return float(loss.detach()), g.double().numpy()


def detector_grad_closed(semi, labels, mask, gout=1.0):
    """The rule of imx_detector_loss_grad written out in float64, no autograd: dL/dx_j = (m / D) (q_j - p_j sum_c q_c) with
    q_c = -t_c [-log p_c <= 100] + (1 - t_c) [-log(1 - p_c) <= 100] e_c / (sum of the other exponentials), the products that carry the
    maximum's ratio multiplied out (ratio_k (1 - p_k) = 1 / S, p_j ratio_k = (e_j / S_rest) / S) so that nothing overflows."""
    x = np.asarray(semi, np.float64)
    t, m = R.cell_targets(labels).numpy(), R.cell_masks(mask).numpy()
    k = x.argmax(1)[:, None]
    mx = np.take_along_axis(x, k, 1)
    e = np.exp(x - mx)
    S = e.sum(1, keepdims=True)
    is_k = np.arange(65)[None, :, None, None] == k
    rest = np.where(is_k, 0.0, e).sum(1, keepdims=True)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        nlp = (mx - x) + np.log(S)
        nl1p = np.where(is_k, np.log(S) - np.log(rest), -np.log1p(-np.where(is_k, 0.0, e) / S))
        tn = np.where(nlp <= 100, t, 0.0)
        r = np.where(nl1p <= 100, 1 - t, 0.0)
        ratio = np.where(is_k, 0.0, e / (S - e))                        # the maximum's own ratio never appears
        rk = np.where(is_k, r, 0.0).sum(1, keepdims=True)
        A = tn.sum(1, keepdims=True)
        Brest = np.where(is_k, 0.0, r * ratio).sum(1, keepdims=True)
        uk = np.where(rk != 0, rk / np.where(rest > 0, rest, 1.0), 0.0)
        g = -tn + np.where(is_k, rk / S, r * ratio - uk * e / S) - (e / S) * (Brest - A)
    return g * (gout * m[:, None] / (m.sum() + 1e-10))


def _sample(desc, cells, Hc, Wc):
    """tests/sptrain_ref.py: _sample on desc's device"""
    uv = torch.stack([torch.as_tensor(cells % Wc), torch.as_tensor(cells // Wc)], 1).to(desc.device, desc.dtype)
    g = uv / torch.tensor([Wc, Hc], dtype=desc.dtype, device=desc.device) * 2 - 1
    out = torch.nn.functional.grid_sample(desc[None], g[None, :, None], mode="bilinear", align_corners=True)
    return out[0, :, :, 0].t()


def desc_loss_t(da, db, pair_a, pair_b, choice, nonmatch_b, lamda_d=250., margin=0.2, method="1d"):
    """tests/sptrain_ref.py: desc_loss on tensors (d,Hc,Wc) in their dtype -> the total lamda_d match + non_match as a tensor"""
    d, Hc, Wc = da.shape
    ia, ib = np.asarray(pair_a, np.int64)[choice], np.asarray(pair_b, np.int64)[choice]
    fa, fb = da.reshape(d, -1).t(), db.reshape(d, -1).t()
    a1 = fa[ia]
    if method == "2d":
        ma, mb = _sample(da, ia, Hc, Wc), _sample(db, ib, Hc, Wc)
    else:
        ma, mb = a1, fb[ib]
    match = torch.clamp(1 - (ma * mb).sum(-1), min=0).sum() / len(ia)
    prod = (a1[:, None, :] * fb[torch.as_tensor(np.asarray(nonmatch_b, np.int64)).to(da.device)]).sum(-1)
    # the non-match hinge is strict (imx_train.h): an entry with v = 0 exactly is no hard negative and carries no gradient.  (torch's
    # clamp(min=0) would pass the gradient there; the fixtures hold no product within 1e-5 of the margin, so the two cannot differ on them.)
    v = torch.where(prod - margin > 0, prod - margin, torch.zeros_like(prod))
    hard = int((v != 0).sum())                                           # a constant of the derivative
    return lamda_d * match + v.sum() / (hard + 1)


def desc_grad(desc_a, desc_b, pair_a, pair_b, choice, nonmatch_b, lamda_d=250., margin=0.2, method="1d", dtype=torch.float64, gout=1.0):
    """one image -> (total, d total / d desc_a, d total / d desc_b), the gradients as float64 arrays (d,Hc,Wc)"""
    with torch.enable_grad():
        da = torch.as_tensor(np.asarray(desc_a)).to(dtype).requires_grad_(True)
        db = torch.as_tensor(np.asarray(desc_b)).to(dtype).requires_grad_(True)
        loss = desc_loss_t(da, db, pair_a, pair_b, choice, nonmatch_b, lamda_d, margin, method)
        ga, gb = torch.autograd.grad(loss * gout, (da, db))
    return float(loss.detach()), ga.double().numpy(), gb.double().numpy()


def match_products(desc_a, desc_b, pair_a, pair_b, choice, method="1d"):
    """<a_m, b_m> of every match in float64 (the hinge's argument is 1 minus this)"""
    da, db = torch.as_tensor(np.asarray(desc_a)).double(), torch.as_tensor(np.asarray(desc_b)).double()
    d, Hc, Wc = da.shape
    ia, ib = np.asarray(pair_a, np.int64)[choice], np.asarray(pair_b, np.int64)[choice]
    if method == "2d":
        ma, mb = _sample(da, ia, Hc, Wc), _sample(db, ib, Hc, Wc)
    else:
        ma, mb = da.reshape(d, -1).t()[ia], db.reshape(d, -1).t()[ib]
    return (ma * mb).sum(-1).numpy()


def cell_l1(g):
    """per-cell L1 norm over the channel axis: (..., C, Hc, Wc) -> (..., Hc, Wc)"""
    return np.abs(np.asarray(g, np.float64)).sum(-3)
